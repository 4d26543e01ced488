"""The plain resnet_18 family (models/resnet.py; SFA_BACKBONE_DECONV) on the host: the extended C ABI
(sfa_arch_ex and the *_ex entry points), its state layout against the reference's, the packing of the
transposed convolutions into four 2 x 2 phase matrices (restated in f64 numpy against
torch.nn.functional.conv_transpose2d + BatchNorm), and the drop-in module.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import golden_cases as gc
import golden_io
from conftest import GOLDEN
from sfa_hip import _lib
from sfa_hip.runtime import pack_state_dict


class Cfg(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def rg():
    return golden_io.load(GOLDEN, "resnet_golden")


@pytest.fixture(scope="module")
def arch():
    return _lib.make_arch(gc.HEADS, backbone=_lib.BACKBONE_DECONV)


@pytest.fixture(scope="module")
def state(rg):
    return gc.state_dict_np(rg)


def test_state_layout_matches_reference(rg, arch):
    layout = _lib.state_layout(arch)
    assert [n for n, _ in layout] == [str(n) for n in rg["state_names"]]
    assert [s for _, s in layout] == [s for _, s in gc.state_spec(rg)]
    names = [n for n, _ in layout]
    assert dict(layout)["deconv_layers.0.weight"] == (512, 256, 4, 4)  # (Cin, Cout, kh, kw)
    assert dict(layout)["deconv_layers.6.weight"] == (256, 256, 4, 4)
    assert names.index("deconv_layers.7.running_var") < names.index("cen_offset.0.weight") < names.index("z_coor.2.bias")


def test_ex_kfpn_case_equals_the_old_entry_points(golden):
    L = _lib.lib()
    old = _lib.make_arch(gc.HEADS)
    ex = _lib.make_arch(gc.HEADS, backbone=_lib.BACKBONE_KFPN)
    assert isinstance(old, _lib.SfaArch) and isinstance(ex, _lib.SfaArchEx)
    assert L.sfa_state_count_ex(ctypes.byref(ex)) == L.sfa_state_count(ctypes.byref(old)) == 186
    assert _lib.state_layout(ex) == _lib.state_layout(old)
    assert L.sfa_state_floats_ex(ctypes.byref(ex)) == L.sfa_state_floats(ctypes.byref(old))
    assert L.sfa_packed_floats_ex(ctypes.byref(ex)) == L.sfa_packed_floats(ctypes.byref(old))
    sd = gc.state_dict_np(golden.model)
    a, b = pack_state_dict(sd, old), pack_state_dict(sd, ex)
    assert a.tobytes() == b.tobytes()


def test_bad_descriptors_are_refused(arch):
    L = _lib.lib()
    bad = _lib.make_arch(gc.HEADS, backbone=_lib.BACKBONE_DECONV)
    bad.reserved[3] = 1
    assert L.sfa_state_count_ex(ctypes.byref(bad)) == -1 and b"reserved" in L.sfa_last_error_string()
    buf, shape, nd = ctypes.create_string_buffer(128), (ctypes.c_int64 * 4)(), ctypes.c_int()
    assert L.sfa_state_entry_ex(ctypes.byref(bad), 0, buf, 128, shape, ctypes.byref(nd)) == -1
    assert L.sfa_state_floats_ex(ctypes.byref(bad)) == 0 and L.sfa_packed_floats_ex(ctypes.byref(bad)) == 0
    ws = ctypes.create_string_buffer(16)
    p = ctypes.cast(ws, ctypes.c_void_p)
    h = ctypes.c_void_p()
    assert L.sfa_model_create_ex(ctypes.byref(bad), p, ctypes.byref(h)) == -1
    assert L.sfa_pack_weights_ex(ctypes.byref(bad), p, 4, p) == -1
    unk = _lib.make_arch(gc.HEADS, backbone=2)
    assert L.sfa_state_count_ex(ctypes.byref(unk)) == -1 and b"backbone" in L.sfa_last_error_string()
    # depths other than 18 and head_conv != 64 stay refused in this family too
    deep = _lib.make_arch(gc.HEADS, num_layers=34, backbone=_lib.BACKBONE_DECONV)
    assert L.sfa_state_count_ex(ctypes.byref(deep)) == -1 and b"resnet_18" in L.sfa_last_error_string()
    assert b"fpn_resnet_18" not in L.sfa_last_error_string()
    assert L.sfa_packed_floats_ex(ctypes.byref(_lib.make_arch(gc.HEADS, head_conv=32, backbone=1))) == 0
    junk = np.zeros(10, np.float32)
    assert L.sfa_pack_weights_ex(ctypes.byref(arch), junk.ctypes.data, 10, junk.ctypes.data) == -1
    assert b"state floats" in L.sfa_last_error_string()


def _plan_offsets(num_heads=5):
    """The packed layout of the deconv family, recomputed independently (mirror of pack_plan.h make_plan):
    the shared backbone as tests/test_abi.py, then per transposed conv w [4][256][4 C], b [256],
    wh [4][2][256][4 C] fp16, winv [4][256], then the one head level."""
    cur = 0
    out = {}

    def take(n):
        nonlocal cur
        o = cur
        cur = (cur + n + 15) // 16 * 16
        return o

    def conv(N, K):
        Kp = (K + 15) // 16 * 16
        take(N * Kp), take(N), take((3 * N * Kp + 1) // 2), take(N * Kp), take(N)

    conv(64, 196)
    inpl = 64
    for li in range(4):
        planes = 64 << li
        for bi in range(2):
            conv(planes, 9 * (inpl if bi == 0 else planes))
            conv(planes, 9 * planes + (inpl if bi == 0 and li > 0 else 0))
        inpl = planes
    for i, C in enumerate((512, 256, 256)):
        K = 4 * C
        out[i] = dict(C=C, K=K, w=take(4 * 256 * K), b=take(256), wh=take(4 * 256 * K), winv=take(4 * 256))
    N, K = num_heads * 64, 9 * 256
    out["heads"] = dict(w3=take(N * K), b3=take(N), w1=take(num_heads * 256), b1=take(num_heads * 4),
                        wx=take((3 * N * K + 1) // 2), wh=take(N * K), winv=take(N))
    return out, cur


@pytest.fixture(scope="module")
def packed(state, arch):
    return pack_state_dict(state, arch)


def test_packed_size_and_heads(packed, state, arch):
    offs, total = _plan_offsets()
    assert packed.size == total == _lib.lib().sfa_packed_floats_ex(ctypes.byref(arch))
    hp = offs["heads"]
    W3 = packed[hp["w3"]:hp["w3"] + 320 * 2304].reshape(5, 64, 3, 3, 256)
    for j, name in enumerate(gc.HEADS):  # forward order, OHWI
        np.testing.assert_array_equal(W3[j], state[f"{name}.0.weight"].transpose(0, 2, 3, 1))
        np.testing.assert_array_equal(packed[hp["b3"] + 64 * j: hp["b3"] + 64 * j + 64], state[f"{name}.0.bias"])
        ch = gc.HEADS[name]
        np.testing.assert_array_equal(packed[hp["w1"] + 256 * j: hp["w1"] + 256 * j + 64 * ch].reshape(ch, 64),
                                      state[f"{name}.2.weight"][:, :, 0, 0])
        np.testing.assert_array_equal(packed[hp["b1"] + 4 * j: hp["b1"] + 4 * j + ch], state[f"{name}.2.bias"])


@pytest.mark.parametrize("layer", [0, 1, 2])
def test_phase_matrices_restate_conv_transpose(packed, state, layer):
    """y[b][2q + py][2r + px][n] = sum_{dy, dx, c} W_ph[n][(2 dy + dx) C + c] x[b][q - 1 + py + dy][r - 1 + px + dx][c]
    + bias[n] (out-of-range inputs contribute zero), in f64 from the packed f32 phase matrices, against
    conv_transpose2d + BatchNorm (eps 1e-5) of the same state in f64."""
    offs, _ = _plan_offsets()
    d = offs[layer]
    C, K = d["C"], d["K"]
    Wp = packed[d["w"]:d["w"] + 4 * 256 * K].reshape(4, 256, 2, 2, C).astype(np.float64)
    bias = packed[d["b"]:d["b"] + 256].astype(np.float64)
    pre = f"deconv_layers.{3 * layer + 1}."
    w = torch.from_numpy(state[f"deconv_layers.{3 * layer}.weight"]).double()
    g, beta, mu, var = (torch.from_numpy(state[pre + k]).double() for k in ("weight", "bias", "running_mean",
                                                                            "running_var"))
    rng = np.random.default_rng(100 + layer)
    for h, wd in ((1, 1), (2, 3), (3, 3)):
        x = rng.standard_normal((2, C, h, wd))
        ref = torch.nn.functional.conv_transpose2d(torch.from_numpy(x), w, stride=2, padding=1)
        ref = torch.nn.functional.batch_norm(ref, mu, var, g, beta, training=False, eps=1e-5).numpy()
        assert ref.shape == (2, 256, 2 * h, 2 * wd)
        xp = np.zeros((2, h + 2, wd + 2, C))
        xp[:, 1:-1, 1:-1] = x.transpose(0, 2, 3, 1)
        got = np.zeros_like(ref)
        for py in range(2):
            for px in range(2):
                for q in range(h):
                    for r in range(wd):
                        win = xp[:, q + py: q + py + 2, r + px: r + px + 2, :]  # rows q - 1 + py + dy
                        got[:, :, 2 * q + py, 2 * r + px] = np.einsum("byxc,nyxc->bn", win, Wp[2 * py + px]) + bias
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())


@pytest.mark.parametrize("layer", [0, 1, 2])
def test_phase_matrices_fp16_terms(packed, layer):
    """As tests/test_abi.py does for the convs: per phase and row, W 2^(13 - e) = hi + lo in fp16."""
    offs, _ = _plan_offsets()
    d = offs[layer]
    K = d["K"]
    W = packed[d["w"]:d["w"] + 4 * 256 * K].reshape(4, 256, K)
    winv = packed[d["winv"]:d["winv"] + 4 * 256].reshape(4, 256)
    hl = packed[d["wh"]:d["wh"] + 4 * 256 * K].view(np.float16).reshape(4, 2, 256, K)
    e = np.floor(np.log2(np.abs(W).max(2)))
    np.testing.assert_array_equal(winv, np.exp2(e - 13).astype(np.float32))
    scaled = W * (1.0 / winv[:, :, None])
    assert np.abs(scaled).max() < 2.0 ** 14
    np.testing.assert_array_equal(hl[:, 0], scaled.astype(np.float16))
    np.testing.assert_array_equal(hl[:, 1], (scaled - hl[:, 0].astype(np.float32)).astype(np.float16))
    rel = np.abs(hl[:, 0].astype(np.float64) + hl[:, 1] - scaled) / np.abs(scaled).max(2, keepdims=True)
    assert rel.max() <= 2.0 ** -22


def test_create_model_resnet_18(rg, capsys):
    from models import resnet
    from models.model_utils import create_model
    m = create_model(Cfg(arch="resnet_18", heads=dict(gc.HEADS), head_conv=64, imagenet_pretrained=False))
    assert "using ResNet architecture\n" == capsys.readouterr().out
    assert isinstance(m, resnet.PoseResNet)
    sd = m.state_dict()
    assert list(sd) == [str(n) for n in rg["state_names"]]
    assert [tuple(v.shape) for v in sd.values()] == [s for _, s in gc.state_spec(rg)]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in gc.state_dict_np(rg).items()}, strict=True)
    assert resnet.get_pose_net is not None and resnet.resnet_spec[18][1] == [2, 2, 2, 2]
    with pytest.raises(_lib.SfaNativeError):
        m(torch.zeros(1, 3, 32, 32))  # no CPU path


def test_create_model_refusals():
    from models.model_utils import create_model
    for kw in (dict(arch="resnet_34", head_conv=64), dict(arch="resnet_18", head_conv=32),
               dict(arch="fpn_resnet_34", head_conv=64)):
        with pytest.raises(NotImplementedError):
            create_model(Cfg(heads=dict(gc.HEADS), imagenet_pretrained=False, **kw))
    with pytest.raises(RuntimeError):
        create_model(Cfg(arch="resnet_18", heads=dict(gc.HEADS), head_conv=64, imagenet_pretrained=True))


def test_synthetic_conditioning_of_the_new_names():
    from sfa_hip import synthetic
    w = synthetic.synthetic_tensor("deconv_layers.3.weight", (256, 256, 4, 4))
    assert np.abs(w).max() <= np.sqrt(6.0 / (4 * 256)) and np.abs(w).max() > 0.99 * np.sqrt(6.0 / (4 * 256))
    g = synthetic.synthetic_tensor("deconv_layers.4.weight", (256,))
    assert g.min() >= 0.5 and g.max() <= 1.0
    v = synthetic.synthetic_tensor("deconv_layers.7.running_var", (256,))
    assert v.min() >= 0.5 and v.max() <= 2.0
    assert synthetic.synthetic_tensor("deconv_layers.1.num_batches_tracked", ()).dtype == np.int64


def test_model_handle_batch_ceiling_and_views(arch):
    """A handle needs no device memory: the per-model pass size (64 H W bytes per frame for the deconv
    family's widest conv input: 90 frames at 608 x 608; 181 for KFPN), the workspace sized for a pass,
    the family's buffer views, the math modes, and side streams as a no-op."""
    L = _lib.lib()
    ws = ctypes.create_string_buffer(16)
    p = ctypes.cast(ws, ctypes.c_void_p)
    h, hk = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.sfa_model_create_ex(ctypes.byref(arch), p, ctypes.byref(h)) == 0
    kf = _lib.make_arch(gc.HEADS)
    assert L.sfa_model_create(ctypes.byref(kf), p, ctypes.byref(hk)) == 0
    try:
        assert L.sfa_model_forward_max_batch(h, 608, 608) == 90 == ((1 << 31) - 1) // (64 * 608 * 608)
        assert L.sfa_model_forward_max_batch(hk, 608, 608) == 181 == L.sfa_forward_max_batch(608, 608)
        assert L.sfa_model_forward_max_batch(h, 64, 64) == ((1 << 31) - 1) // (64 * 64 * 64)
        assert L.sfa_model_forward_max_batch(None, 608, 608) == 0
        assert L.sfa_model_forward_max_batch(h, 8192, 8192) == 0
        one = L.sfa_forward_workspace_size(h, 90, 608, 608)
        assert one > 0 and L.sfa_forward_workspace_size(h, 91, 608, 608) == one
        assert L.sfa_forward_workspace_size(h, 89, 608, 608) < one
        outs = (ctypes.c_void_p * 5)(*([p.value] * 5))
        assert L.sfa_model_forward(h, p, _lib.IN_NCHW3, 100, 608, 608, outs, p, one - 1, None) == -4
        for which in range(0, 4):
            assert L.sfa_forward_buffer_offset(h, 2, 64, 64, which) >= 0
        for which in range(4, 10):  # UP_LEVEL*, HEADS_L*: KFPN only
            assert L.sfa_forward_buffer_offset(h, 2, 64, 64, which) == -1
            assert L.sfa_forward_buffer_offset(hk, 2, 64, 64, which) >= 0
        d = [L.sfa_forward_buffer_offset(h, 2, 64, 64, _lib.BUF_DECONV1 + i) for i in range(3)]
        assert d[0] > L.sfa_forward_buffer_offset(h, 2, 64, 64, 3) and d[0] < d[1] < d[2]
        assert d[1] - d[0] >= 2 * 4 * 4 * 256 * 4 and d[2] - d[1] >= 2 * 8 * 8 * 256 * 4
        for i in range(3):
            assert L.sfa_forward_buffer_offset(hk, 2, 64, 64, _lib.BUF_DECONV1 + i) == -1
        assert L.sfa_forward_buffer_offset(h, 2, 64, 64, 13) == -1
        # arithmetic: fp16x3 only
        assert L.sfa_model_get_math(h) == _lib.MATH_FP16X3
        for mode in (_lib.MATH_F32, _lib.MATH_BF16X6, _lib.MATH_FP16):
            assert L.sfa_model_set_math(h, mode) == -2 and b"FP16X3 only" in L.sfa_last_error_string()
            assert L.sfa_model_get_math(h) == _lib.MATH_FP16X3
        assert L.sfa_model_set_math(h, _lib.MATH_FP16X3) == 0 and L.sfa_model_set_math(h, 7) == -1
        assert L.sfa_model_set_side_streams(h, 1) == 0 and L.sfa_model_set_side_streams(h, 0) == 0
    finally:
        L.sfa_model_destroy(h)
        L.sfa_model_destroy(hk)
