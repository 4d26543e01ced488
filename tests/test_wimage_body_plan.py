"""The body convs' weight images (csrc/conv_wimage.h: the strip K order of conv_h3s_kernel, split-K slices, the
body plan): the stand-alone host check under ASan + UBSan (tools/wimage_body_check.cpp: its own main, no
preloading) and the strip order against an independent numpy restatement of "the LDS image of K-tile kt"."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "wimage_body_check.cpp")


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    """tools/wimage_body_check built with the host sanitizers, once for the module."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("wimage_body") / "wimage_body_check")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r


def test_self_check_under_host_sanitizers(helper):
    r = run(helper)
    assert r.returncode == 0 and " checks, 0 bad" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def swzB(R):
    """conv_h3s_kernel.h: the 16-B quad q of LDS row R is stored at quad q ^ swzB(R)."""
    return ((R >> 2) & 3) ^ ((((R & 15) + 4) >> 3) & 1)


def strip_k0(t, C):
    """conv_h3s_kernel.h: k-step t of the sweep is tap kw = t % 3 of super-step s = t // 3 = (kh, 32-channel
    chunk), and its W tile starts at weight column (kh * 3 + kw) * C + chunk * 32."""
    nchunk = C // 32
    s, kw = divmod(t, 3)
    kh, chunk = divmod(s, nchunk)
    return (kh * 3 + kw) * C + chunk * 32


def lds_image(terms_arr, N, C, BN):
    """For every column tile and k-step of the strip sweep, the bytes the kernel wants in its W stage: per
    term, BN rows of 64 B, source quad q of row R at quad q ^ swzB(R).  uint16 [N / BN][9 C / 32][2][BN][32]."""
    K = 9 * C
    out = np.zeros((N // BN, K // 32, 2, BN, 32), np.uint16)
    for nt in range(N // BN):
        for t in range(K // 32):
            k0 = strip_k0(t, C)
            for R in range(BN):
                for q in range(4):
                    p = q ^ swzB(R)
                    out[nt, t, :, R, 8 * p:8 * p + 8] = terms_arr[:, nt * BN + R, k0 + 8 * q:k0 + 8 * q + 8]
    return out


# (name, N, C, BN): layer1's tile, a 128-wide tile, BN = 48 (6 pieces)
CASES = [("layer1_128x64", 64, 64, 64), ("layer2_128x128", 128, 128, 128), ("odd_pieces_bn48", 96, 32, 48)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_strip_order_matches_lds_restatement(helper, case):
    _, N, C, BN = case
    K = 9 * C
    r = run(helper, "dump", N, K, K, 0, BN, 2, 0, C, 1)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    nbytes = int(lines[0].split()[1])
    tab = np.array([l.split() for l in lines[1:]], dtype=np.int64)  # offset term n k src
    assert nbytes == 2 * N * K * 2 and tab.shape == (nbytes // 16, 5)
    assert np.array_equal(tab[:, 0], 16 * np.arange(nbytes // 16))
    rng = np.random.default_rng(11)
    ids = rng.permutation(2 * N * K).astype(np.uint32)  # every element distinct: equal images, equal index maps
    for arr in ((ids & 0xffff).astype(np.uint16).reshape(2, N, K), (ids >> 16).astype(np.uint16).reshape(2, N, K)):
        got = arr.reshape(-1)[tab[:, 4][:, None] + np.arange(8)[None, :]].reshape(-1)  # the builder: 8 fp16 from src
        assert np.array_equal(got, lds_image(arr, N, C, BN).reshape(-1))
    assert np.array_equal(tab[:, 4], (tab[:, 1] * N + tab[:, 2]) * K + tab[:, 3])
    assert tab[:, 3].min() == 0 and tab[:, 3].max() == K - 8


def test_split_k_slices_are_contiguous_runs_of_the_one_image(helper):
    """Slice kz of nsplit sweeps super-steps kz * nsl .. : its K-tiles are the contiguous tiles 3 kz nsl .. of
    the conv's image, and the slices' columns partition the conv's."""
    N, C, BN, nsplit = 64, 128, 64, 2
    K = 9 * C
    r = run(helper, "dump", N, K, K, 0, BN, 2, 0, C, 1)
    tab = np.array([l.split() for l in r.stdout.splitlines()[1:]], dtype=np.int64)
    tile_units = 2 * BN * 64 // 16
    k_of_tile = tab[:, 3].reshape(K // 32, tile_units).min(axis=1)  # first column of each K-tile (one column tile)
    nsl = 3 * (C // 32) // nsplit
    cols = []
    for kz in range(nsplit):
        want = [strip_k0(3 * s + kw, C) for s in range(kz * nsl, (kz + 1) * nsl) for kw in range(3)]
        assert list(k_of_tile[3 * kz * nsl:3 * (kz + 1) * nsl]) == want
        cols += want
    assert sorted(cols) == list(range(0, K, 32))


def test_the_other_orders_refuse_the_flag(helper):
    assert run(helper, "dump", 64, 640, 640, 0, 64, 2, 0, 64, 1).returncode == 2   # a tail segment
    assert run(helper, "dump", 64, 576, 576, 0, 64, 2, 18, 64, 1).returncode == 2  # chunk-major and strip


def test_symbols_declared_and_bound():
    sys.path.insert(0, os.path.join(REPO, "lidar-image_object-detection_-fpn_resnet-yolov8_amd", "sfa"))
    from sfa_hip import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sfa_hip.h")).read(), flags=re.S)
    sym = "sfa_model_body_weight_image_bytes"
    assert re.search(r"\b" + sym + r"\s*\(", header)
    assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), sym)
    assert re.search(r"SFA_OPT_BODY_W_IMAGES\s*=\s*%d\b" % _lib.OPT_BODY_W_IMAGES, header)
    assert _lib.OPT_BODY_W_IMAGES in _lib.OPTION_KEYS and _lib.OPT_BODY_W_IMAGES == _lib.OPT_W_IMAGES + 1
