"""Forward parity for every head set the model descriptor admits (tests/headset_cases.py): one to eight heads
of one to four channels, insertion order unlike sorted() order, offsets unlike 0, 3, 5, 7, 8.

Head counts other than five run other kernels (csrc/conv.hip: conv_x6g<256, 64> in fp16x3, conv_x6<128, 64> in
bf16x6, conv_kernel<128, 64> with grid.y = heads in f32, no W image, fp16 mode falling back to fp16x3), and a
five-head set with a 4-channel head runs the production conv_r3<256, 320> through the o = 3 branch of its packed
head epilogue, which the production set (ch <= 3) never enters.  The fused combine and the resnet_18 relayout
read the same offset tables (csrc/aux_kernels.hip).

Every stage check is the one of test_gpu_model_stages.py: the GPU's per-level head maps and outputs against
the f64 oracle stage evaluated on the GPU's own stage inputs, per frame, at stage_cases.GATE.  The premises
that make it sharp (distinct channels, live ReLU, nonzero biases) are asserted on the oracle's side only, here
and in tests/test_headsets_host.py, which also shows that the checker fails on the errors this file is for.
Measured worst stage errors: DESIGN.md §3.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp16_emulation as emu
import golden_cases as gc
import golden_io
import headset_cases as hc
import stage_cases as sc
from conftest import GOLDEN
from sfa_hip import _lib

pytestmark = pytest.mark.gpu

TOL = 1e-4  # tests/test_gpu_model.py: whole forward against the reference fixture
FP16_GATE = 1e-5  # tests/test_gpu_math_fp16.py: the heads kernel against the emulation on identical inputs
MATHS = ("f32", "bf16x6", "fp16x3")
PARITY_CASES = [(n, "3x64x96") for n in hc.SETS] + [("one", "5x32x32"), ("eight_full", "5x32x32")]
ON, OFF = 1, 0

_MODELS = {}


def model_of(gpu, arch, name):
    """(model, numpy state dict, engine, f64 head state) of one set, built once; the engine is handed out in
    fp16x3 with its weight images on."""
    if (arch, name) not in _MODELS:
        heads = hc.SETS[name]
        model, sd = hc.make_model(arch, heads, gpu)
        _MODELS[arch, name] = (model, sd, model._engine(gpu), hc.head_state_f64(sd, heads, arch))
    model, sd, eng, sd64 = _MODELS[arch, name]
    assert model._engine(gpu) is eng
    eng.set_math(_lib.MATH_FP16X3)
    eng.set_option(_lib.OPT_W_IMAGES, ON)
    return model, sd, eng, sd64


def same_bits(a, b, what, sel=None):
    for k in a:
        if k == "x":
            continue
        ta = a[k] if sel is None else a[k][sel]
        assert ta.shape == b[k].shape, (what, k)
        same = torch.equal(ta.contiguous().view(torch.int32), b[k].contiguous().view(torch.int32))
        assert same, f"{what}: {k} differs, max |d| {float((ta - b[k]).abs().max()):.3g}"


def check_head_stages(maps, sd64, heads, title):
    """heads0..2 and out of `maps` (CPU) against the f64 oracle stages on the maps' own inputs: the premises on
    the oracle's side, the table, the gate."""
    with torch.no_grad():
        ref = sc.run_stages(sd64, maps, heads, only=hc.GROUPS)
    hc.assert_output_premises(ref, heads, title)
    hc.assert_relu_live(sd64, maps, heads, title)
    rows = sc.compare(maps, ref, heads, per_frame=True)
    print(sc.format_rows(f"{title}: GPU stage vs f64 oracle stage on the GPU's inputs", rows, heads))
    bad = sc.failures(rows)
    assert not bad, f"{title}: " + "; ".join(bad)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name,batch", PARITY_CASES)
def test_heads_stage_parity(gpu, name, batch, math):
    """Every set in every arithmetic on the 3 x 64 x 96 mixed batch (M = 72, 288, 1152 per level), the smallest
    and the largest set also on 5 x 32 x 32 (one tile spans five frames with five fp16x3 scales)."""
    heads = hc.SETS[name]
    model, _, eng, sd64 = model_of(gpu, "fpn_resnet_18", name)
    x = hc.BATCHES[batch]()
    B, _, H, W = x.shape
    maps = hc.to_cpu(hc.gpu_maps(eng, x, heads, math))
    hc.assert_layout(maps, heads, B, H, W)
    with torch.no_grad():
        out = model(torch.from_numpy(x).to(gpu))  # the public forward: the same dict, the same bits
    assert list(out) == list(heads), "the forward emits the heads in insertion order"
    same_bits({f"out/{h}": v.cpu() for h, v in out.items()}, maps, f"{name} {math}: model(x) vs forward_into")
    check_head_stages(maps, sd64, heads, f"{math} {name} {batch}")


@pytest.mark.parametrize("case", list(gc.MODEL_CASES))
@pytest.mark.parametrize("name", ["five_wide", "five_ones"])
def test_fp16_mode_one_product_heads(gpu, name, case):
    """Five heads run the TERMS = 1 twin of the production heads kernel: the assertion of
    test_gpu_math_fp16.test_heads_kernel_on_identical_inputs, on its inputs, with another head set.  The
    emulation at one product and at three differ by more than ten gates (emulation only), so a kernel that
    ran fp16x3 here would not pass."""
    heads = hc.SETS[name]
    _, sd, eng, _ = model_of(gpu, "fpn_resnet_18", name)
    maps = hc.to_cpu(hc.gpu_maps(eng, gc.model_input(case), heads, "fp16"))
    sdt = {k: torch.from_numpy(v) for k, v in sd.items() if k.startswith("fpn")}
    apart = 0.0
    with torch.no_grad():
        for level in range(3):
            inp = maps[f"up_level{level + 2}"].to(torch.float64)
            want = emu.head_level(sdt, inp, level, heads, 1)
            three = emu.head_level(sdt, inp, level, heads, 2)
            for h in heads:
                e = emu.rel_err(maps[f"heads{level}/{h}"].numpy(), want[h].numpy())
                apart = max(apart, emu.rel_err(three[h].numpy(), want[h].numpy()))
                print(f"{name} {case} level {level} {h}: heads kernel vs emulation {e:.3g}")
                assert e <= FP16_GATE, (level, h, e)
    assert apart > 10 * FP16_GATE, apart


@pytest.mark.parametrize("name", ["one", "three", "eight_full"])
def test_fp16_mode_fallback_heads(gpu, name):
    """Other head counts have no one-product heads kernel: whatever the body runs, the heads run fp16x3
    (include/sfa_hip.h), so on the GPU's own up_level maps they meet the gate of every other mode."""
    heads = hc.SETS[name]
    _, _, eng, sd64 = model_of(gpu, "fpn_resnet_18", name)
    x = hc.BATCHES["3x64x96"]()
    maps = hc.to_cpu(hc.gpu_maps(eng, x, heads, "fp16"))
    assert eng.math == _lib.MATH_FP16
    hc.assert_layout(maps, heads, *x.shape[:1], *x.shape[2:])
    check_head_stages(maps, sd64, heads, f"fp16 (heads fp16x3) {name} 3x64x96")


@pytest.mark.parametrize("name", ["five_wide", "one", "eight_full"])
def test_wimage_on_off_bit_equal(gpu, name):
    """Five heads (N = 320) have the pre-tiled W images and read them by default; other counts have none and the
    option is accepted without effect.  Either way SFA_OPT_W_IMAGES changes no bit of any head map."""
    heads = hc.SETS[name]
    _, _, eng, _ = model_of(gpu, "fpn_resnet_18", name)
    if len(heads) == 5:
        assert eng.weight_image_bytes() == 2 * 320 * 9 * (256 + 128 + 64) * 2
    else:
        assert eng.weight_image_bytes() == 0
    x = hc.BATCHES["3x64x96"]()
    off = hc.to_cpu(hc.gpu_maps(eng, x, heads, options={_lib.OPT_W_IMAGES: OFF}))
    assert eng.get_option(_lib.OPT_W_IMAGES) == OFF
    on = hc.to_cpu(hc.gpu_maps(eng, x, heads, options={_lib.OPT_W_IMAGES: ON}))
    assert eng.get_option(_lib.OPT_W_IMAGES) == ON
    assert float(on[f"heads0/{next(iter(heads))}"].abs().max()) > 0
    same_bits(on, off, f"{name}: W images on vs off")


@pytest.mark.parametrize("name", ["five_wide", "eight_full"])
def test_batch_invariance(gpu, name):
    """fp16x3: two runs of the mixed batch are bit-identical, and frame 1 (scaled 2^-6 between frames scaled 1
    and 2^9) run alone has the bits it has in the batch."""
    heads = hc.SETS[name]
    _, _, eng, _ = model_of(gpu, "fpn_resnet_18", name)
    x = hc.BATCHES["3x64x96"]()
    full = hc.to_cpu(hc.gpu_maps(eng, x, heads))
    again = hc.to_cpu(hc.gpu_maps(eng, x, heads))
    same_bits(full, again, f"{name}: two runs")
    one = hc.to_cpu(hc.gpu_maps(eng, x[1:2], heads))
    same_bits(full, one, f"{name}: frame 1 in the batch vs alone", slice(1, 2))


@pytest.mark.parametrize("name", ["five_wide", "eight_full"])
def test_resnet_18_heads(gpu, name):
    """The plain resnet_18 (fp16x3, its only mode) runs the KFPN level-0 heads instance on its 256-channel
    deconv3 map, then relays the channel-planar block out into the caller's per-head NCHW buffers
    (launch_heads_relayout, the same offset table).  Those buffers against conv3x3 + bias -> ReLU ->
    conv1x1 + bias in f64 on the GPU's own deconv3 map: heads kernel and relayout in one check."""
    heads = hc.SETS[name]
    model, _, eng, sd64 = model_of(gpu, "resnet_18", name)
    x = hc.BATCHES["3x64x96"]()
    B, _, H, W = x.shape
    xt = torch.from_numpy(x).to(gpu)
    ws = torch.empty(eng.workspace_bytes(B, H, W), dtype=torch.uint8, device=gpu)
    outs = eng.forward_into(xt, eng.alloc_outputs(B, H, W), workspace=ws)
    torch.cuda.synchronize()
    assert list(outs) == list(heads)
    inp = eng.debug_views(ws, B, H, W)["deconv3"].contiguous().cpu().to(torch.float64)
    assert tuple(inp.shape) == (B, 256, H // 4, W // 4)
    got, ref = {}, {}
    with torch.no_grad():
        for h, c in heads.items():
            hd = F.relu(F.conv2d(inp, sd64[h + ".0.weight"], sd64[h + ".0.bias"], 1, 1))
            assert bool((hd == 0).any()) and bool((hd > 0).any()), h
            ref[f"out/{h}"] = F.conv2d(hd, sd64[h + ".2.weight"], sd64[h + ".2.bias"])
            got[f"out/{h}"] = outs[h].cpu()
            assert tuple(got[f"out/{h}"].shape) == (B, c, H // 4, W // 4), h
        pub = model(xt)
    assert list(pub) == list(heads)
    same_bits({f"out/{h}": v.cpu() for h, v in pub.items()}, got, f"resnet_18 {name}: model(x) vs forward_into")
    hc.assert_output_premises(ref, heads, f"resnet_18 {name}")
    rows = sc.compare(got, ref, heads, per_frame=True)
    print(sc.format_rows(f"resnet_18 fp16x3 {name} 3x64x96: heads + relayout vs f64 on the GPU's deconv3", rows, heads))
    bad = sc.failures(rows)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("arch,name", hc.FIXTURE_CASES)
def test_reference_fixture(gpu, arch, name):
    """The whole forward against the reference's own get_pose_net(18, heads, 64) on the same weights and input
    (tests/golden/gen_headsets_golden.py), at the bound of tests/test_gpu_model.py."""
    g = golden_io.load(GOLDEN, "headsets_golden")
    heads = hc.SETS[name]
    model, _, _, _ = model_of(gpu, arch, name)
    with torch.no_grad():
        out = model(torch.from_numpy(hc.fixture_input()).to(gpu))
    assert list(out) == [str(k) for k in g[f"{arch}/{name}/heads"]] == list(heads)
    for h in heads:
        ref = g[f"{arch}/{name}/{h}"]
        got = out[h].cpu().numpy()
        assert got.shape == ref.shape
        e = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
        print(f"{arch} {name} {h}: max rel err {e:.3g}")
        assert e <= TOL, (h, e)
