"""Reference-compatible ``losses`` package (gfx950 backend: sfa_hip).  Evaluation only."""

from sfa_hip import dropin as _dropin

__path__ = _dropin.package_path(__path__, __name__)
