"""Bit-comparison of two builds of libsfa_hip.so on the same forwards (round-4 prune check).

    SFA_HIP_LIB=<lib> [SFA_ABI_EXPECT=1] python tools/ab_lib_bits.py run out.npz
    SFA_HIP_LIB=<lib> python tools/ab_lib_bits.py grads out.npz
    python tools/ab_lib_bits.py compare a.npz b.npz

`run` packs the synthetic weights and saves every head map of the forward under each configuration of
CONFIGS below: every math mode, every kernel-choice option off, no side streams, the serial probe, the
three input layouts and the resnet_18 family, at sizes with more than one tile per map at every level;
and fp16x3 / fp16 with default options at 608 x 608 with 10 frames, which covers every kernel path of the
bench (r3 heads, strip convs, r3 body convs, FPN skip convs, split-K layer4, the patch stem). A
configuration that the library lacks (an older build) is reported and left out. `grads` saves the forwards
and every gradient of the neck, block and stem operators on seeded inputs at the cases of GRAD_CASES below,
once with all outputs wanted and once with only the data gradient. `compare` asserts that the two files
hold the same maps, bit-identical."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lidar-image_object-detection_-fpn_resnet-yolov8_amd", "sfa"))

SMALL = [(2, 96, 96), (3, 160, 192)]  # multiples of 32 with more than one tile per map at every level
BIG = (10, 608, 608)  # the big-M conv_r3 body tiles and the tile_rows >= 50000 branches
L4STRIP = (1, 384, 384)  # the smallest input whose layer4 maps (144 rows) take the strip kernel: split-K 2 and its tickets
# (tag, setup, cases): setup is a list of (what, argument), applied to a fresh engine through the
# runtime's public setters. The default-option fp16x3 maps keep their bare keys.
CONFIGS = [
    ("", [], SMALL + [BIG, L4STRIP]),
    ("fp16/", [("math", "MATH_FP16")], SMALL + [BIG, L4STRIP]),
    ("bf16x6/", [("math", "MATH_BF16X6")], SMALL),
    ("f32/", [("math", "MATH_F32")], SMALL),
    ("stem_patch=0/", [("option", ("OPT_STEM_PATCH", 0))], SMALL),
    ("fpn_commute=0/", [("option", ("OPT_FPN_COMMUTE", 0))], SMALL),
    ("fpn_commute=5/", [("option", ("OPT_FPN_COMMUTE", 5))], SMALL),  # a commuted and a concat level in one pass
    ("fpn_gemm=0/", [("option", ("OPT_FPN_GEMM", 0))], SMALL),
    ("splitk_tickets=0/", [("option", ("OPT_SPLITK_TICKETS", 0))], SMALL + [L4STRIP]),
    ("side_streams=0/", [("side_streams", False)], SMALL[1:]),
    ("probe_serial/", [("probe", ("PROBE_HEADS", "PROBE_SERIAL"))], SMALL[1:]),
    ("nhwc4/", [("layout", "IN_NHWC4")], SMALL[:1]),
    ("flip_hw/", [("layout", "IN_NCHW3_FLIP_HW")], SMALL[:1]),
    ("stem_patch=0,nhwc4/", [("option", ("OPT_STEM_PATCH", 0)), ("layout", "IN_NHWC4")], SMALL[:1]),
    ("stem_patch=0,flip_hw/", [("option", ("OPT_STEM_PATCH", 0)), ("layout", "IN_NCHW3_FLIP_HW")], SMALL[:1]),
    ("resnet_18/", [("deconv", None)], SMALL),
    ("resnet_18,probe/", [("deconv", None), ("probe", ("PROBE_HEADS",))], SMALL[:1]),
]


def run(out):
    import torch
    from sfa_hip import _lib, runtime, synthetic
    _lib.ABI_VERSION = int(os.environ.get("SFA_ABI_EXPECT", _lib.ABI_VERSION))
    import ctypes
    probe = ctypes.CDLL(_lib.LIB_PATH)  # an older build lacks the newer entry points: bind what it has
    for name in [n for n in _lib._PROTOS if not hasattr(probe, n)]:
        print("not in", _lib.LIB_PATH, ":", name)
        del _lib._PROTOS[name]
    dev = torch.device("cuda", 0)
    inputs, packed = {}, {}

    def bev(case):
        if case not in inputs:
            B, H, W = case
            inputs[case] = torch.from_numpy(synthetic.synthetic_bev(B, H, W, seed=B + H)).to(dev)
        return inputs[case]

    def engine(setup):
        """(engine, input layout, probe pairs to read) of one configuration."""
        what = dict(setup)
        backbone = _lib.BACKBONE_DECONV if "deconv" in what else None
        if backbone not in packed:
            arch = _lib.make_arch(runtime.DEFAULT_HEADS, backbone=backbone)
            sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), 0)
            packed[backbone] = (arch, runtime.pack_state_dict(sd, arch))
        eng = runtime.KfpnEngine(*packed[backbone], dev, math=getattr(_lib, what.get("math", "MATH_FP16X3")))
        if "option" in what:
            eng.set_option(getattr(_lib, what["option"][0]), what["option"][1])
        if "side_streams" in what:
            eng.set_side_streams(what["side_streams"])
        if "probe" in what:
            eng.set_probe(sum(getattr(_lib, f) for f in what["probe"]))
        return eng, getattr(_lib, what.get("layout", "IN_NCHW3")), (4 if backbone else 3) if "probe" in what else 0

    res = {}
    for tag, setup, cases in CONFIGS:
        try:
            eng, layout, pairs = engine(setup)
        except (AttributeError, _lib.SfaNativeError) as e:
            print("not in", _lib.LIB_PATH, ":", tag, setup, "--", e)
            continue
        for case in cases:
            x = bev(case)
            if layout == _lib.IN_NHWC4:
                x4 = torch.zeros((x.shape[0], x.shape[2], x.shape[3], 4), dtype=torch.float32, device=dev)
                x4[..., :3] = x.permute(0, 2, 3, 1)
                x = x4
            elif layout == _lib.IN_NCHW3_FLIP_HW:
                x = torch.flip(x, [2, 3]).contiguous()
            o = eng.forward(x, layout)
            if pairs:  # every probe event of the forward was recorded
                assert all(t > 0 for t in eng.probe_times(pairs)), tag
            for h, v in o.items():
                res["%s%dx%dx%d/%s" % ((tag,) + case + (h,))] = v.cpu().numpy()
    np.savez(out, **res)
    print("saved", out, len(res))


# The smallest cases at which the pieces the three operators share can go wrong.  neck (B, h4, w4, cap): a short last
# chunk, a chunk that is no multiple of 16, one-pixel tiles, dW1 written in two column ranges.  block (layer, block, B,
# h, w, cap): the identity skip; the stride-2 downsample at odd sizes with its one-tap fold; cout 512, whose bias grid
# has a second axis of 2.  stem (B, H, W, cap).
GRAD_CASES = {"neck": [(2, 2, 3, 7), (1, 1, 3, 3), (1, 1, 1, 0)],
              "block": [(1, 0, 2, 5, 7, 17), (2, 0, 2, 5, 7, 7), (4, 1, 1, 3, 3, 0)],
              "stem": [(2, 12, 20, 17), (1, 7, 9, 3)]}


def grads(out):
    import torch
    from sfa_hip import _lib, runtime, synthetic
    dev = torch.device("cuda", 0)
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), 0)
    eng = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), dev)
    gen = torch.Generator().manual_seed(7)
    rnd = lambda shape: torch.randn(tuple(shape), generator=gen).to(dev)  # noqa: E731
    res = {}

    def keep(tag, names, tensors):
        for n, t in zip(names, tensors):
            if t is not None:
                res[f"{tag}/{n}"] = t.cpu().numpy()

    for B, h4, w4, cap in GRAD_CASES["neck"]:
        tag = f"neck/{B}x{h4}x{w4}/cap{cap}"
        sh = eng._neck_shapes(B, h4, w4)
        ls = [rnd(s) for s in sh[:4]]
        us = eng.neck_forward(*ls)
        keep(tag, ("u2", "u3", "u4"), us)
        gs = [rnd(s) for s in sh[4:]]
        for part, wp in (("all", (True,) * 6), ("data", (False,) * 6)):
            dl, dp = eng.neck_grad(*gs, layers=ls, ups=us[:2], want_params=wp, max_chunk_pixels=cap)
            keep(f"{tag}/{part}", ("d_l1", "d_l2", "d_l3", "d_l4", "dW1", "db1", "dW2", "db2", "dW3", "db3"), dl + dp)
    for layer, block, B, h, w, cap in GRAD_CASES["block"]:
        tag = f"block/layer{layer}.{block}/{B}x{h}x{w}/cap{cap}"
        x = rnd((B, h, w, eng.block_shape(layer, block)[0]))
        mid, y = eng.block_forward(layer, block, x)
        keep(tag, ("mid", "y"), (mid, y))
        gy = rnd(y.shape)
        for part, wp in (("all", (True,) * 5), ("data", (False,) * 5)):
            dx, dp = eng.block_grad(layer, block, x, mid, y, gy, want_params=wp, max_chunk_pixels=cap)
            keep(f"{tag}/{part}", ("dx", "dW1", "db1", "dW2", "db2", "dWd"), [dx] + dp)
    for B, H, W, cap in GRAD_CASES["stem"]:
        tag = f"stem/{B}x{H}x{W}/cap{cap}"
        x = rnd((B, 3, H, W))
        a, pooled = eng.stem_forward(x)
        keep(tag, ("a", "pooled"), (a, pooled))
        gp = rnd(pooled.shape)
        for part, wp in (("all", (True, True)), ("data", (False, False))):
            dx, dp = eng.stem_grad(x, a, gp, want_params=wp, max_chunk_pixels=cap)
            keep(f"{tag}/{part}", ("dx", "dW", "db"), [dx] + dp)
    torch.cuda.synchronize()
    np.savez(out, **res)
    print("saved", out, len(res))


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    for k in sorted(set(A.files) ^ set(Bz.files)):
        print("MISSING in", a if k not in A.files else b, ":", k)
    assert sorted(A.files) == sorted(Bz.files)
    bad = [k for k in A.files if not np.array_equal(A[k], Bz[k])]
    for k in bad:
        d = np.abs(A[k] - Bz[k])
        print("DIFF", k, float(d.max()))
    print("bit-identical" if not bad else f"{len(bad)} of {len(A.files)} maps differ")
    return 0 if not bad else 1


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    elif sys.argv[1] == "grads":
        grads(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
