"""The bytes of the host weight pack, pinned: for every case of pack_cases.digest_cases the packed buffer
sfa_pack_weights(_ex) writes has the SHA-256 that tests/golden/pack_digests.json recorded at the commit it names
(tests/golden/gen_pack_digests.py).  CPU only: the host pack touches no device."""
import json
import os

import pytest

import pack_cases

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "pack_digests.json")))
_CASES = pack_cases.digest_cases()


def test_every_case_is_recorded():
    assert len(GOLDEN["commit"]) == 40
    assert sorted(GOLDEN["cases"]) == sorted(_CASES)
    assert len(_CASES) == len(pack_cases.CASES) + 2 * len(pack_cases.DIGEST_SEEDS) * len(pack_cases.hc.SETS)


@pytest.mark.parametrize("cid", list(_CASES))
def test_host_pack_bytes_are_the_recorded_ones(cid):
    arch, state = _CASES[cid]
    want = GOLDEN["cases"][cid]
    state_sha, packed_sha = pack_cases.digests(arch, state())
    assert state_sha == want["state_sha256"], f"{cid}: the INPUT state differs from the recorded one, not the pack"
    assert packed_sha == want["packed_sha256"], f"{cid}: the packed bytes differ from commit {GOLDEN['commit'][:12]}"
