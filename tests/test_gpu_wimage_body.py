"""The residual layers' weight images (csrc/conv_wimage.h strip order, h3sopt::W_IMAGE): the
fp16x3 strip convs reading W from their pre-tiled LDS images give the bits of the row-major path
(SFA_OPT_BODY_W_IMAGES 1 / 0).  160 and 192 inputs, B = 2 and 3, as tests/test_gpu_wimage.py: partial M tiles
and tiles that span two frames in layer1 / 2 (and layer3 at 192; maps of under 128 rows per frame take conv_h3,
which reads no image).  The split-K layer4 strip convs need maps of 128 rows: one 384 input (12 x 12) runs all
ten strip convs on their images, tickets on and off.  Then the other math modes (they ignore the images), the
writers of weights (in-place re-upload + refresh, an optimiser step through the Python model), and engines, a
twin and their captured graphs interleaved with eager forwards."""
import numpy as np
import pytest
import torch

from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu

ON, OFF = 1, 0
BODY = _lib.OPT_BODY_W_IMAGES
HEADS_IMAGE_BYTES = 2 * 320 * 9 * (256 + 128 + 64) * 2


def _packed(arch, seed):
    return runtime.pack_state_dict(synthetic.synthetic_state_dict(_lib.state_layout(arch), seed), arch)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _forward_all(eng, x, body_images):
    """One forward with the body images on / off (the heads' stay on): the outputs, every backbone / FPN / head
    map from the stage views and the detections."""
    eng.set_option(_lib.OPT_W_IMAGES, ON)
    eng.set_option(BODY, body_images)
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


def _on_off_equal(eng, x):
    off = _forward_all(eng, x, OFF)
    on = _forward_all(eng, x, ON)
    assert set(on) == set(off) and len(on) > 20
    assert float(on["out.hm_cen"].abs().max()) > 0
    bad = [k for k in on if not _bits(on[k], off[k])]
    assert not bad, bad


def body_plan_bytes():
    """csrc/conv_wimage.h wimage_plan over the ten strip convs (all four of layer1, block 1's two of layers
    2 - 4): 2 terms x N x 9 C fp16 each, 256-B aligned."""
    total = 0
    for li in range(4):
        c = 64 << li
        for _ in range(4 if li == 0 else 2):
            total = (total + 2 * c * 9 * c * 2 + 255) // 256 * 256
    return total


@pytest.fixture(scope="module")
def engine(gpu):
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    return runtime.KfpnEngine(arch, _packed(arch, 0), gpu)


def test_size_query_and_option(engine):
    assert engine.body_weight_image_bytes() == body_plan_bytes()
    assert engine.weight_image_bytes() == HEADS_IMAGE_BYTES  # the heads' plan alone, as before
    for v in (OFF, ON):
        engine.set_option(BODY, v)
        assert engine.get_option(BODY) == v
    with pytest.raises(Exception):
        engine.set_option(BODY, 2)


@pytest.mark.parametrize("size", [160, 192])
@pytest.mark.parametrize("B", [2, 3])
def test_body_images_bit_equal_to_row_major(gpu, engine, size, B):
    x = torch.from_numpy(synthetic.synthetic_bev(B, size, size, seed=5 + B)).to(gpu)
    _on_off_equal(engine, x)


@pytest.mark.parametrize("tickets", [ON, OFF])
def test_split_k_strip_convs(gpu, engine, tickets):
    """384 x 384: layer4 is 12 x 12 = 144 rows per frame, the smallest map its split-K 2 strip instance takes;
    B = 3 leaves its last 128-row tile partly filled and two tiles spanning frames."""
    x = torch.from_numpy(synthetic.synthetic_bev(3, 384, 384, seed=11)).to(gpu)
    engine.set_option(_lib.OPT_SPLITK_TICKETS, tickets)
    try:
        _on_off_equal(engine, x)
    finally:
        engine.set_option(_lib.OPT_SPLITK_TICKETS, ON)


@pytest.mark.parametrize("tickets", [ON, OFF])
def test_split_k_tickets_small_maps(gpu, engine, tickets):
    x = torch.from_numpy(synthetic.synthetic_bev(2, 192, 192, seed=2)).to(gpu)
    engine.set_option(_lib.OPT_SPLITK_TICKETS, tickets)
    try:
        _on_off_equal(engine, x)
    finally:
        engine.set_option(_lib.OPT_SPLITK_TICKETS, ON)


def test_resnet_18_arch(gpu):
    """The plain resnet_18 has the same residual layers: the same images."""
    arch = _lib.make_arch(runtime.DEFAULT_HEADS, backbone=_lib.BACKBONE_DECONV)
    eng = runtime.KfpnEngine(arch, _packed(arch, 0), gpu)
    assert eng.body_weight_image_bytes() == body_plan_bytes()
    assert eng.weight_image_bytes() == 2 * 320 * 9 * 256 * 2
    x = torch.from_numpy(synthetic.synthetic_bev(2, 192, 192, seed=4)).to(gpu)
    outs = {}
    for v in (OFF, ON):
        eng.set_option(BODY, v)
        outs[v] = {n: t.clone() for n, t in eng.forward(x).items()}
    torch.cuda.synchronize()
    assert all(_bits(outs[ON][n], outs[OFF][n]) for n in outs[ON])


@pytest.mark.parametrize("math", [_lib.MATH_FP16, _lib.MATH_BF16X6])
def test_other_math_modes_ignore_the_images(gpu, math):
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    eng = runtime.KfpnEngine(arch, _packed(arch, 0), gpu, math=math)
    x = torch.from_numpy(synthetic.synthetic_bev(2, 192, 192, seed=6)).to(gpu)
    outs = {}
    for v in (OFF, ON):
        eng.set_option(BODY, v)
        outs[v] = {n: t.clone() for n, t in eng.forward(x).items()}
    torch.cuda.synchronize()
    assert all(_bits(outs[ON][n], outs[OFF][n]) for n in outs[ON])
    assert float(outs[ON]["hm_cen"].abs().max()) > 0


def test_w_images_off_turns_both_off(gpu, engine):
    """SFA_OPT_W_IMAGES = 0 with the body option left on: the row-major bits."""
    x = torch.from_numpy(synthetic.synthetic_bev(2, 192, 192, seed=8)).to(gpu)
    want = _forward_all(engine, x, OFF)
    engine.set_option(BODY, ON)
    engine.set_option(_lib.OPT_W_IMAGES, OFF)
    got = {n: t.clone() for n, t in engine.forward(x).items()}
    engine.set_option(_lib.OPT_W_IMAGES, ON)
    torch.cuda.synchronize()
    assert all(_bits(got[n], want[f"out.{n}"]) for n in got)


def test_reupload_and_refresh(gpu):
    """After an in-place change of the packed buffer, refresh_weight_images re-derives both sets of images on
    the stream: the forward equals a freshly created engine's row-major forward on the new weights."""
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    p0, p1 = _packed(arch, 0), _packed(arch, 1)
    x = torch.from_numpy(synthetic.synthetic_bev(2, 192, 192, seed=9)).to(gpu)
    eng = runtime.KfpnEngine(arch, p0, gpu)
    eng.set_option(BODY, ON)
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


def test_forward_after_an_optimiser_step(gpu):
    """An optimiser step through the Python model: its next forward (a new handle over the repacked weights,
    images on) equals a freshly created model's forward on the updated weights with every image off."""
    from models.fpn_resnet import get_pose_net

    def make():
        m = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False)
        sd = synthetic.synthetic_state_dict(_lib.state_layout(m._arch), 4)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
        return m.to(gpu).eval()

    model = make()
    x = torch.from_numpy(synthetic.synthetic_bev(2, 192, 192, seed=3)).to(gpu)
    model.heads_trainable()
    opt = torch.optim.SGD(model.head_parameters(), lr=1e-2)
    with torch.enable_grad():
        before = {n: t.detach().clone() for n, t in model(x).items()}
        sum((t * t).mean() for t in model(x).values()).backward()
    opt.step()
    eng = model._engine(x.device)
    assert eng.body_weight_image_bytes() > 0
    eng.set_option(_lib.OPT_W_IMAGES, ON)
    eng.set_option(BODY, ON)
    with torch.no_grad():
        after = {n: t.clone() for n, t in model(x).items()}
    fresh = make()
    fresh.load_state_dict(model.state_dict())
    fresh._engine(x.device).set_option(_lib.OPT_W_IMAGES, OFF)
    with torch.no_grad():
        want = {n: t.clone() for n, t in fresh(x).items()}
    torch.cuda.synchronize()
    assert all(_bits(after[n], want[n]) for n in want)
    assert not all(_bits(after[n], before[n]) for n in want)


# ---- engines, a twin and their graphs (the pattern of tests/test_gpu_graphs.py) ----
GB, GS = 2, 192


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
    e1.set_option(BODY, OFF)
    ref_pipe = _pipe(e1, x)
    _fwd(ref_pipe)
    ref = _snap(ref_pipe)  # eager, row-major body
    e1.set_option(BODY, ON)
    tw = e1.twin()
    e2 = runtime.KfpnEngine(arch, packed, gpu, side_streams=side)
    e2.set_option(BODY, ON)
    assert tw.get_option(BODY) == ON and tw.body_weight_image_bytes() == e1.body_weight_image_bytes() > 0
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
