"""Derived weight images (csrc/conv_wimage.h): the fp16x3 heads reading W from their pre-tiled
LDS images give the bits of the row-major path (SFA_OPT_W_IMAGES 1 / 0).  The smallest model sizes whose
level widths are 40 / 20 / 10 and 48 / 24 / 12 (160 and 192 inputs), B = 2 and 3: the small maps' 256-row
tiles span frames and the last M tile is partly filled.  Every map the forward leaves is compared — the
per-level head maps, the five outputs, the detections, and the backbone / FPN maps in front of them (the
stride-2, conv + downsample, split-K and FPN skip convs run their row-major kernels under either setting:
only the heads have an image form) — then the writers of weights: an optimiser step through
heads_trainable(), an in-place re-upload + sfa_model_refresh_weight_images, and engines, a twin() and their
captured graphs interleaved with eager forwards."""
import numpy as np
import pytest
import torch

from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu

ON, OFF = 1, 0


def _packed(arch, seed):
    return runtime.pack_state_dict(synthetic.synthetic_state_dict(_lib.state_layout(arch), seed), arch)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _forward_all(eng, x, images):
    """One forward with the images on / off: the outputs, every intermediate map and the detections."""
    eng.set_option(_lib.OPT_W_IMAGES, images)
    B, _, H, W = x.shape
    ws = torch.empty(eng.workspace_bytes(B, H, W), dtype=torch.uint8, device=x.device)
    outs = eng.forward_into(x, eng.alloc_outputs(B, H, W), _lib.IN_NCHW3, ws)
    views = eng.debug_views(ws, B, H, W)
    got = {f"out.{n}": t.clone() for n, t in outs.items()}
    for k, v in views.items():
        if k == "levels":
            for n, lv in v.items():
                for f, t in enumerate(lv):
                    got[f"level{f}.{n}"] = t.clone()
        else:
            got[k] = v.clone()
    hm, off = runtime.sigmoid_clamp_(outs["hm_cen"].clone()), runtime.sigmoid_clamp_(outs["cen_offset"].clone())
    got["dets"] = runtime.decode(hm, off, outs["direction"], outs["z_coor"], outs["dim"], K=20).clone()
    torch.cuda.synchronize()
    return got


@pytest.fixture(scope="module")
def engine(gpu):
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    return runtime.KfpnEngine(arch, _packed(arch, 0), gpu)


def test_handle_has_images_and_the_option(engine):
    # the five default heads: 2 terms x 320 x 9 (256 + 128 + 64) fp16 = the size of the heads' terms again
    assert engine.weight_image_bytes() == 2 * 320 * 9 * (256 + 128 + 64) * 2
    assert engine.get_option(_lib.OPT_W_IMAGES) in (ON, OFF)
    for v in (OFF, ON):
        engine.set_option(_lib.OPT_W_IMAGES, v)
        assert engine.get_option(_lib.OPT_W_IMAGES) == v
    with pytest.raises(Exception):
        engine.set_option(_lib.OPT_W_IMAGES, 2)


@pytest.mark.parametrize("size", [160, 192])
@pytest.mark.parametrize("B", [2, 3])
def test_image_path_bit_equal_to_row_major(gpu, engine, size, B):
    x = torch.from_numpy(synthetic.synthetic_bev(B, size, size, seed=5 + B)).to(gpu)
    off = _forward_all(engine, x, OFF)
    on = _forward_all(engine, x, ON)
    assert set(on) == set(off) and len([k for k in on if k.startswith("level")]) == 15
    assert float(on["level0.hm_cen"].abs().max()) > 0
    bad = [k for k in on if not _bits(on[k], off[k])]
    assert not bad, bad


def test_deconv_family_heads(gpu):
    """resnet_18: its one head level runs the same 256 x 320 heads kernel (Cin 256)."""
    arch = _lib.make_arch(runtime.DEFAULT_HEADS, backbone=_lib.BACKBONE_DECONV)
    eng = runtime.KfpnEngine(arch, _packed(arch, 0), gpu)
    assert eng.weight_image_bytes() == 2 * 320 * 9 * 256 * 2
    x = torch.from_numpy(synthetic.synthetic_bev(2, 160, 160, seed=4)).to(gpu)
    outs = {}
    for v in (OFF, ON):
        eng.set_option(_lib.OPT_W_IMAGES, v)
        outs[v] = {n: t.clone() for n, t in eng.forward(x).items()}
    torch.cuda.synchronize()
    assert all(_bits(outs[ON][n], outs[OFF][n]) for n in outs[ON])


def test_reupload_and_refresh(gpu):
    """The packed buffer is the caller's: after an in-place change, refresh_weight_images re-derives the images
    on the stream, and the forward equals a freshly created engine's on the new weights (its row-major path)."""
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    p0, p1 = _packed(arch, 0), _packed(arch, 1)
    x = torch.from_numpy(synthetic.synthetic_bev(2, 160, 160, seed=9)).to(gpu)
    eng = runtime.KfpnEngine(arch, p0, gpu)
    eng.set_option(_lib.OPT_W_IMAGES, ON)
    before = {n: t.clone() for n, t in eng.forward(x).items()}
    eng.weights.copy_(torch.from_numpy(p1).to(gpu))
    eng.refresh_weight_images()
    after = {n: t.clone() for n, t in eng.forward(x).items()}
    fresh = runtime.KfpnEngine(arch, p1, gpu)
    fresh.set_option(_lib.OPT_W_IMAGES, OFF)
    want = {n: t.clone() for n, t in fresh.forward(x).items()}
    torch.cuda.synchronize()
    assert all(_bits(after[n], want[n]) for n in want)
    assert not all(_bits(after[n], before[n]) for n in want)


def test_forward_after_a_head_training_step(gpu):
    """heads_trainable(): after an optimiser step the model's forward (a new handle over the repacked weights,
    images on) equals a freshly created model's forward on the updated weights with the images off."""
    from models.fpn_resnet import get_pose_net

    def make():
        m = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False)
        sd = synthetic.synthetic_state_dict(_lib.state_layout(m._arch), 4)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
        return m.to(gpu).eval()

    model = make()
    x = torch.from_numpy(synthetic.synthetic_bev(2, 160, 160, seed=3)).to(gpu)
    model.heads_trainable()
    opt = torch.optim.SGD(model.head_parameters(), lr=1e-2)
    with torch.enable_grad():  # whatever grad mode an earlier test left behind
        before = {n: t.detach().clone() for n, t in model(x).items()}
        sum((t * t).mean() for t in model(x).values()).backward()
    opt.step()
    eng = model._engine(x.device)
    assert eng.weight_image_bytes() > 0
    eng.set_option(_lib.OPT_W_IMAGES, ON)
    with torch.no_grad():
        after = {n: t.clone() for n, t in model(x).items()}
    fresh = make()
    fresh.load_state_dict(model.state_dict())
    fresh._engine(x.device).set_option(_lib.OPT_W_IMAGES, OFF)
    with torch.no_grad():
        want = {n: t.clone() for n, t in fresh(x).items()}
    torch.cuda.synchronize()
    assert all(_bits(after[n], want[n]) for n in want)
    assert not all(_bits(after[n], before[n]) for n in want)  # the step moved the heads


# ---- engines, a twin and their graphs (the pattern of tests/test_gpu_graphs.py) ----
GB, GS = 2, 160


def _pipe(eng, x):
    p = runtime.DetectorPipeline(eng, GB, GS, GS, K=20)
    p.x.copy_(x)
    return p


def _fwd(p):
    p.engine.forward_into(p.x, p.outs, _lib.IN_NCHW3, p.ws, _lib.stream_ptr(p.dev))


def _capture(p):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _fwd(p)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _fwd(p)
    return g


def _snap(p):
    torch.cuda.synchronize()
    return {h: p.outs[h].clone() for h in p.outs}


@pytest.mark.parametrize("side", [False, True])
def test_twin_shares_images_and_graphs_replay(gpu, side):
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    packed = _packed(arch, 0)
    x = torch.from_numpy(synthetic.synthetic_bev(GB, GS, GS, seed=1)).to(gpu)
    e1 = runtime.KfpnEngine(arch, packed, gpu, side_streams=side)
    e1.set_option(_lib.OPT_W_IMAGES, OFF)
    ref_pipe = _pipe(e1, x)
    _fwd(ref_pipe)
    ref = _snap(ref_pipe)  # eager, row-major
    e1.set_option(_lib.OPT_W_IMAGES, ON)
    tw = e1.twin()
    e2 = runtime.KfpnEngine(arch, packed, gpu, side_streams=side)
    e2.set_option(_lib.OPT_W_IMAGES, ON)
    assert tw.get_option(_lib.OPT_W_IMAGES) == ON and tw.weight_image_bytes() == e1.weight_image_bytes() > 0
    a, t, b = _pipe(e1, x), _pipe(tw, x), _pipe(e2, x)
    ga, gt, gb = _capture(a), _capture(t), _capture(b)
    seq = []
    for name, act, p in (("replay a", ga.replay, a), ("replay twin", gt.replay, t), ("replay b", gb.replay, b),
                         ("eager twin", lambda: _fwd(t), t), ("replay a after eager twin", ga.replay, a),
                         ("eager b", lambda: _fwd(b), b), ("replay twin after eager b", gt.replay, t),
                         ("eager a", lambda: _fwd(a), a), ("replay b after eager a", gb.replay, b)):
        for h in p.outs:
            p.outs[h].zero_()
        act()
        got = _snap(p)
        seq.append((name, all(_bits(got[h], ref[h]) for h in ref)))
    assert all(ok for _, ok in seq), seq
    del e1, a, ga, ref_pipe  # the twin keeps the shared images alive
    torch.cuda.synchronize()
    for h in t.outs:
        t.outs[h].zero_()
    gt.replay()
    got = _snap(t)
    assert all(_bits(got[h], ref[h]) for h in ref)
