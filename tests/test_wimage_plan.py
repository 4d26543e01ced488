"""Pre-tiled weight images (csrc/conv_wimage.h): the index function (geometry, column tile, K-tile, piece,
lane) -> source (term, n, k) against an independent numpy restatement of "the LDS image of K-tile kt", and
the stand-alone host check under ASan + UBSan (tools/wimage_plan_check.cpp: its own main, no preloading)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "wimage_plan_check.cpp")


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    """tools/wimage_plan_check built with the host sanitizers, once for the module."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("wimage") / "wimage_plan_check")
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
    """conv_r3_kernel.h / conv_h3_kernel.h: the 16-B quad q of LDS row R is stored at quad q ^ swzB(R)."""
    return ((R >> 2) & 3) ^ ((((R & 15) + 4) >> 3) & 1)


def kcol(kt, cmaj_tiles, C):
    """First weight column of K-tile kt: chunk-major (tap kt % 9 of 32-channel chunk kt // 9) over the first
    cmaj_tiles tiles, kt * 32 after them and in a tap-major kernel."""
    if kt < cmaj_tiles:
        return (kt % 9) * C + (kt // 9) * 32
    return kt * 32


def lds_image(terms_arr, N, K, wstride, wk0, BN, terms, cmaj_tiles, C):
    """The restatement: for every column tile and K-tile, the bytes the kernel wants in its LDS slot — per
    term, BN rows of 64 B (32 fp16 K columns), source quad q of row R at quad position q ^ swzB(R) — laid
    end to end.  terms_arr: uint16 [terms][N][wstride].  Returns uint16 [N / BN][K / 32][terms][BN][32]."""
    out = np.zeros((N // BN, K // 32, terms, BN, 32), np.uint16)
    for nt in range(N // BN):
        for kt in range(K // 32):
            k0 = wk0 + kcol(kt, cmaj_tiles, C)
            for R in range(BN):
                for q in range(4):
                    p = q ^ swzB(R)
                    out[nt, kt, :, R, 8 * p:8 * p + 8] = terms_arr[:, nt * BN + R, k0 + 8 * q:k0 + 8 * q + 8]
    return out


# (name, N, K, wstride, wk0, BN, terms, cmaj_tiles, C): one shape per kernel family that stages W by
# LDS-DMA; the heads' chunk-major tile, a conv + downsample (chunk-major 3x3 then a tap-major tail), the
# same conv tap-major, a wk0 / wstride slice, and BN = 48 (6 pieces: not a multiple of 4 or 8 waves)
CASES = [
    ("heads_L2_conv_r3_256x320", 320, 576, 576, 0, 320, 2, 18, 64),
    ("conv_r3_128x128_cmaj_two_segments", 128, 640, 640, 0, 128, 2, 18, 64),
    ("conv_h3s_128x128_tap_major", 128, 640, 640, 0, 128, 2, 0, 64),
    ("conv_h3_128x64_fpn_slice", 128, 128, 384, 256, 64, 2, 0, 128),
    ("odd_pieces_bn48", 96, 288, 288, 0, 48, 2, 9, 32),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_index_function_matches_lds_restatement(helper, case):
    _, N, K, wstride, wk0, BN, terms, cmaj, C = case
    r = run(helper, "dump", N, K, wstride, wk0, BN, terms, cmaj, C)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    nbytes = int(lines[0].split()[1])
    tab = np.array([l.split() for l in lines[1:]], dtype=np.int64)  # offset term n k src
    assert nbytes == terms * N * K * 2 and tab.shape == (nbytes // 16, 5)
    # image order: offsets 0, 16, 32, ..
    assert np.array_equal(tab[:, 0], 16 * np.arange(nbytes // 16))
    # every element of the terms array distinct, so equal images mean equal index maps
    rng = np.random.default_rng(7)
    total = terms * N * wstride
    assert total < 2 ** 32
    ids = rng.permutation(total).astype(np.uint32)
    lo = (ids & 0xffff).astype(np.uint16).reshape(terms, N, wstride)
    hi = (ids >> 16).astype(np.uint16).reshape(terms, N, wstride)
    for arr in (lo, hi):
        flat = arr.reshape(-1)
        got = flat[tab[:, 4][:, None] + np.arange(8)[None, :]].reshape(-1)  # the builder: 8 fp16 from src
        want = lds_image(arr, N, K, wstride, wk0, BN, terms, cmaj, C).reshape(-1)
        assert np.array_equal(got, want)
    # src is the element index of (term, n, k) in [terms][N][wstride]
    assert np.array_equal(tab[:, 4], (tab[:, 1] * N + tab[:, 2]) * wstride + tab[:, 3])
    # only the slice's columns are read
    assert tab[:, 3].min() == wk0 and tab[:, 3].max() == wk0 + K - 8


def test_chunk_major_and_tap_major_hold_the_same_tiles_in_another_order(helper):
    """The two K orders of one conv: K-tile kt of the chunk-major image is K-tile kcol(kt) / 32 of the
    tap-major one, byte for byte."""
    N, K, BN, C = 128, 576, 128, 64
    a = run(helper, "dump", N, K, K, 0, BN, 2, 18, C)
    b = run(helper, "dump", N, K, K, 0, BN, 2, 0, C)
    ta = np.array([l.split() for l in a.stdout.splitlines()[1:]], dtype=np.int64)[:, 4].reshape(18, -1)
    tb = np.array([l.split() for l in b.stdout.splitlines()[1:]], dtype=np.int64)[:, 4].reshape(18, -1)
    for kt in range(18):
        assert np.array_equal(ta[kt], tb[kcol(kt, 18, C) // 32])
    assert not np.array_equal(ta, tb)


def test_restatement_matches_the_kernel_fragment_formula():
    """The kernels' fragment read (conv_r3_kernel.h bfo): lane (c16 = l & 15, g = l >> 4) of column block ni
    reads 16 B at c16 * 64 + ((g ^ swzB(c16)) << 4) + ni * 1024 of a term's rows and must get
    k = 8 g .. 8 g + 7 of row 16 ni + c16."""
    N = BN = 64
    K = 64
    terms_arr = np.arange(2 * N * K, dtype=np.uint16).reshape(2, N, K)
    img = lds_image(terms_arr, N, K, K, 0, BN, 2, 0, 32)
    for kt in range(K // 32):
        for t in range(2):
            slot = img[0, kt, t].reshape(-1)  # BN rows of 32 fp16
            for ni in range(BN // 16):
                for lane in range(64):
                    c16, g = lane & 15, lane >> 4
                    assert swzB(16 * ni + c16) == swzB(c16)  # the lane part is the same for every piece
                    bfo = c16 * 64 + ((g ^ swzB(c16)) << 4) + ni * 16 * 64
                    frag = slot[bfo // 2:bfo // 2 + 8]
                    assert np.array_equal(frag, terms_arr[t, 16 * ni + c16, 32 * kt + 8 * g:32 * kt + 8 * g + 8])


def test_symbols_declared_and_bound():
    import re
    import sys
    sys.path.insert(0, os.path.join(REPO, "lidar-image_object-detection_-fpn_resnet-yolov8_amd", "sfa"))
    from sfa_hip import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sfa_hip.h")).read(), flags=re.S)
    for sym in ("sfa_model_create_twin", "sfa_model_refresh_weight_images", "sfa_model_weight_image_bytes"):
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), sym)
    assert re.search(r"SFA_OPT_W_IMAGES\s*=\s*%d\b" % _lib.OPT_W_IMAGES, header)
    assert _lib.OPT_W_IMAGES in _lib.OPTION_KEYS and _lib.OPT_W_IMAGES >= 8  # outside the dense 0 .. 7 range
