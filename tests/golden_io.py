"""Golden fixtures on disk: ``<name>.npz`` and, where the arrays need more than one file of
MAX_FILE_BYTES, ``<name>.part1.npz``, ``<name>.part2.npz`` ...  ``load`` gives all parts back as
one mapping (key -> array, ``.files`` like numpy's NpzFile); ``save`` is what the generators under
tests/golden/ write with, so no committed fixture file outgrows the limit."""
import glob
import os

import numpy as np

MAX_FILE_BYTES = 1 << 20
_RAW_BYTES_PER_PART = 960_000  # incompressible floats + the zip directory stay under MAX_FILE_BYTES


class Golden(dict):
    @property
    def files(self):
        return list(self)


def _parts(directory, name):
    more = glob.glob(os.path.join(glob.escape(directory), f"{name}.part[0-9]*.npz"))
    return sorted(more, key=lambda p: int(os.path.basename(p)[len(name) + 5:-4]))


def load(directory, name):
    out = Golden()
    for path in [os.path.join(directory, f"{name}.npz")] + _parts(directory, name):
        with np.load(path) as z:
            for k in z.files:
                assert k not in out, (path, k)
                out[k] = z[k]
    return out


def save(directory, name, arrays):
    for old in _parts(directory, name):
        os.remove(old)
    groups, size = [{}], 0
    for k, v in arrays.items():
        v = np.asarray(v)
        if groups[-1] and size + v.nbytes > _RAW_BYTES_PER_PART:
            groups.append({})
            size = 0
        groups[-1][k] = v
        size += v.nbytes
    for i, g in enumerate(groups):
        path = os.path.join(directory, f"{name}.npz" if i == 0 else f"{name}.part{i}.npz")
        np.savez_compressed(path, **g)
        assert os.path.getsize(path) <= MAX_FILE_BYTES, (path, os.path.getsize(path))
