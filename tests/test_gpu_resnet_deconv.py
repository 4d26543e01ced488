"""GPU parity of the plain resnet_18 forward (models/resnet.py; SFA_BACKBONE_DECONV: the fp16x3
transposed-convolution kernel, deconv_h3_kernel.h, and the fused heads on its 256-channel map) against
the reference fixtures (tests/golden/gen_resnet_golden.py).

Bound: |gpu - ref| <= 1e-4 * max(1, |ref|) on logits and stage maps (tests/test_gpu_model.py TOL).
"""
import numpy as np
import pytest
import torch

import golden_cases as gc
import golden_io
from conftest import GOLDEN
from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu

TOL = 1e-4
# case -> (B, H, W, input seed), as tests/golden/gen_resnet_golden.py CASES
CASES = {"b2_96": (2, 96, 96, 31), "b1_160x128": (1, 160, 128, 32), "b3_32": (3, 32, 32, 33),
         "b1_64": (1, 64, 64, 34)}


class Cfg(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def rg():
    return golden_io.load(GOLDEN, "resnet_golden")


def _input(case):
    B, H, W, seed = CASES[case]
    return synthetic.hash_uniform(seed, 7, B * 3 * H * W).astype(np.float32).reshape(B, 3, H, W)


def _make_model(rg, device, seed=0):
    from models.model_utils import create_model
    model = create_model(Cfg(arch="resnet_18", heads=dict(gc.HEADS), head_conv=64, imagenet_pretrained=False))
    sd = gc.state_dict_np(rg, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model.to(device).eval()


@pytest.fixture(scope="module")
def model(rg, gpu):
    return _make_model(rg, gpu)


def _err(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.mark.parametrize("case", list(CASES))
def test_forward_small_inputs(rg, gpu, model, case):
    """96 x 96 (3 x 3 layer4, two frames), 160 x 128 (5 x 4), 32 x 32 (layer4 is 1 x 1: every deconv
    neighbour is out of range; three frames in one tile) and 64 x 64."""
    with torch.no_grad():
        out = model(torch.from_numpy(_input(case)).to(gpu))
    assert list(out) == list(gc.HEADS), "output dict must follow heads insertion order"
    for h in gc.HEADS:
        ref = rg[f"{case}/{h}"]
        got = out[h].cpu().numpy()
        assert got.shape == ref.shape
        e = _err(got, ref)
        print(f"resnet_18 {case} {h}: max rel err {e:.3g}")
        assert e <= TOL, (h, e)


def test_deconv_stages(rg, gpu, model):
    """SFA_BUF_DECONV1..3 at (1, 64, 64) against the reference's deconv_layers[2], [5], [8] outputs."""
    eng = model._engine(gpu)
    x = torch.from_numpy(_input("b1_64")).to(gpu)
    ws = eng.workspace(1, 64, 64)
    eng.forward_into(x, eng.alloc_outputs(1, 64, 64), workspace=ws)
    views = eng.debug_views(ws, 1, 64, 64)
    assert "up_level2" not in views and "levels" not in views
    for i in range(3):
        ref = rg[f"b1_64/deconv{i + 1}"]
        got = views[f"deconv{i + 1}"].cpu().numpy()
        assert got.shape == ref.shape == (1, 256, 4 << i, 4 << i)
        e = _err(got, ref)
        print(f"resnet_18 deconv{i + 1}: max rel err {e:.3g}, max |ref| {np.abs(ref).max():.3g}")
        assert e <= TOL, (i, e)
        assert got.min() >= 0.0  # ReLU


@pytest.mark.parametrize("shape", [(3, 32, 32), (2, 96, 96)])
def test_batch_invariance_mixed_amplitude(gpu, model, shape):
    """Per-frame scales: every frame of a batch whose frames differ in amplitude by 1e3 is bit-equal
    to the same frame run alone."""
    B, H, W = shape
    x = synthetic.synthetic_bev(B, H, W, seed=61)
    x[1] *= 1e3
    xt = torch.from_numpy(x).to(gpu)
    with torch.no_grad():
        full = {h: v.cpu().numpy() for h, v in model(xt).items()}
        for b in range(B):
            one = model(xt[b:b + 1].contiguous())
            for h in gc.HEADS:
                np.testing.assert_array_equal(full[h][b:b + 1], one[h].cpu().numpy(), err_msg=f"{h}: frame {b}")


def test_other_math_modes_refused(gpu, model):
    """The transposed convolutions have an fp16x3 kernel only: F32 / BF16X6 are SFA_E_UNSUPPORTED, and
    so is FP16 until its error on this architecture is budgeted (include/sfa_hip.h sfa_math)."""
    eng = model._engine(gpu)
    L = _lib.lib()
    for mode in (_lib.MATH_F32, _lib.MATH_BF16X6, _lib.MATH_FP16):
        assert L.sfa_model_set_math(eng._h, mode) == -2
        with pytest.raises(_lib.SfaNativeError):
            eng.set_math(mode)
    assert L.sfa_model_get_math(eng._h) == _lib.MATH_FP16X3 == eng.math
    with pytest.raises(_lib.SfaNativeError):
        model.set_math("bf16x6")
    assert eng.max_batch(608, 608) == 90


def test_forward_608_end_to_end(rg, gpu):
    """cloud -> HIP BEV -> HIP forward -> _sigmoid -> decode on the fixture's tie-free frame: sampled
    logits within the bound, all 50 detections at the reference's pixel and class, every column within
    1e-4."""
    from data_process.kitti_bev_utils import makeBEVMap
    from data_process.kitti_data_utils import get_filtered_lidar
    from utils.evaluation_utils import decode
    from utils.torch_utils import _sigmoid
    model = _make_model(rg, gpu, int(rg["e2e/weight_seed"]))
    cloud = synthetic.synthetic_point_cloud(1)
    bev = makeBEVMap(get_filtered_lidar(cloud, gc.BOUNDARY), gc.BOUNDARY)
    with torch.no_grad():
        out = model(torch.from_numpy(bev[None]).to(gpu).float())
    ys, xs = rg["e2e/sample_yx"]
    for h in gc.HEADS:
        got = out[h].cpu().numpy()[0][:, ys, xs]
        e = _err(got, rg[f"e2e/{h}/samples"])
        print(f"resnet_18 608 {h}: max rel err over 4096 samples {e:.3g}")
        assert e <= TOL, (h, e)
    print(f"fixture min top-51 gap {float(rg['e2e/min_gap'][0]):.3g}")
    hm = _sigmoid(out["hm_cen"])
    off = _sigmoid(out["cen_offset"])
    dets = decode(hm, off, out["direction"], out["z_coor"], out["dim"], K=50).cpu().numpy()
    ref = rg["e2e/dets"]
    assert dets.shape == ref.shape == (1, 50, 10)
    print(f"detections: max |d| {float(np.max(np.abs(dets - ref))):.3g}")
    np.testing.assert_array_equal(dets[..., 9], ref[..., 9])
    np.testing.assert_array_equal(np.floor(dets[..., 1:3]), np.floor(ref[..., 1:3]))  # the pixel (xs, ys)
    np.testing.assert_allclose(dets, ref, rtol=0, atol=TOL)


def test_graph_capture_replays_bit_equal(gpu, model):
    """One forward captured with torch.cuda.graph and replayed twice == the eager run, bit for bit (every
    launch of this topology is on the capturing stream; the amax words are re-zeroed by a kernel node)."""
    eng = model._engine(gpu)
    B, H, W = 2, 96, 96
    x = torch.from_numpy(synthetic.synthetic_bev(B, H, W, seed=71)).to(gpu)
    eager = {h: v.clone() for h, v in eng.forward(x).items()}
    torch.cuda.synchronize()
    outs = eng.alloc_outputs(B, H, W)
    ws = torch.empty(eng.workspace_bytes(B, H, W), dtype=torch.uint8, device=gpu)
    side = torch.cuda.Stream(gpu)
    with torch.cuda.stream(side):  # warm-up on the side stream, as torch.cuda.graph asks
        eng.forward_into(x, outs, workspace=ws)
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.forward_into(x, outs, workspace=ws)
    for rep in range(2):
        for v in outs.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for h in gc.HEADS:
            assert torch.equal(outs[h], eager[h]), (h, rep)


def test_weight_reload_repacks(rg, gpu):
    model = _make_model(rg, gpu)
    x = torch.from_numpy(_input("b3_32")).to(gpu)
    with torch.no_grad():
        a = model(x)["dim"].clone()
        model.deconv_layers[4].bias.add_(0.5)
        b = model(x)["dim"]
    assert not torch.equal(a, b)
