"""The gradient operators at their plans' own chunk, block and pass regimes: one table of cases shared by the host
proof (tests/test_grad_regimes_host.py) and the GPU test (tests/test_gpu_grad_regimes.py), and the regime predicates,
which read the plan fields tools/grad_plan_dump.cpp prints and restate no formula of the plans.

Regimes (every split-K one at max_chunk_pixels == 0, the plan's own chunk):
  S   split-K at the plan's own chunk: two or more chunks of K_c = 2048 pixels, a last chunk of more than 16 pixels
      that is no whole number of 16-pixel LDS steps (a whole step, then a short one), and the first chunk boundary
      inside an image row.
  Sf  S with the first chunk boundary in frame 1 (B = 2).
  S16 two or more chunks of K_c = 2048 with a short last chunk that IS a whole number of LDS steps (the neck's levels
      2 and 3, whose pixel counts are multiples of 16, can reach no other kind).
  O   stride 2 from odd input sizes: the last output row and column read the padding.
  Ps  per-block float64 partials of more than 64 pixels with a short last block.
  Pf  ... with exactly 256 full blocks.
  Ph  the heads' hidden-gradient partials of more than 32 pixels per block with a short last block.
  R   the heads' own whole-row chunks: two or more chunks per frame, the last of fewer rows, B = 2.
  G   the stem data gradient's second pass: at least two more passes than blocks (a whole second pass,
      then a short one), the second passes in frame 1 (B = 2).
  W   the workload's per-frame geometry (a 152 x 152 map; layer2.0 reads it at stride 2), with the plan fields the
      case states.
"""
import collections

Case = collections.namedtuple("Case", "op args shape cap regimes expect")

HEADS = 5  # the default architecture's head count (runtime.DEFAULT_HEADS)
LEVEL_CIN = (256, 128, 64)


def _c(op, args, shape, regimes, cap=0, **expect):
    return Case(op, tuple(args), tuple(shape), cap, frozenset(regimes.split()), expect)


CASES = (
    # S: stride 1 at every width, one frame and two
    [_c("block", (L, 1), (1, 35, 59), "S") for L in (1, 2, 3, 4)]
    + [_c("block", (1, 1), (2, 22, 47), "S Sf")]
    # S: stride 2 from odd sizes at every width, one frame and two
    + [_c("block", (L, 0), (1, 69, 117), "S O") for L in (2, 3, 4)]
    + [_c("block", (2, 0), (2, 43, 93), "S Sf O")]
    + [_c("block_train", (1, 1), (1, 35, 59), "S"), _c("block_train", (2, 0), (1, 69, 117), "S O")]
    + [_c("neck", (), (1, 11, 47), "S S16")]
    + [_c("stem", (), (1, 69, 117), "S")]
    # P
    + [_c("block", (1, 1), (1, 113, 145), "Ps"), _c("block", (1, 1), (1, 104, 160), "Pf"),
       _c("block_train", (1, 1), (1, 113, 145), "Ps"), _c("block_train", (1, 1), (1, 104, 160), "Pf"),
       _c("stem", (), (1, 225, 289), "Ps"), _c("heads", (2,), (1, 169, 194), "Ph")]
    # R at every level
    + [_c("heads", (lv,), (2, 57, 72), "R", rows_per_chunk=56, last_rows=1) for lv in (0, 1, 2)]
    # G
    + [_c("stem", (), (2, 476, 551), "G")]
    # W
    + [_c("block", (1, 1), (1, 152, 152), "W", **{"wg1.chunks": 12, "bs.pixels": 91}),
       _c("block", (2, 0), (1, 152, 152), "W", **{"wg1.chunks": 3, "bs.pixels": 64}),
       _c("block_train", (1, 1), (1, 152, 152), "W", **{"wg1.chunks": 12, "st.pixels": 91}),
       _c("block_train", (2, 0), (1, 152, 152), "W", **{"wg1.chunks": 3, "st.pixels": 64}),
       _c("heads", (2,), (1, 152, 152), "W", chunks_per_frame=6, rows_per_chunk=26, last_rows=22)]
)


def case_id(c):
    a = ".".join(map(str, c.args))
    return f"{c.op}{'-' + a if a else ''}-{'x'.join(map(str, c.shape))}-{'+'.join(sorted(c.regimes))}"


def query(op, args, shape, cap=0):
    """The line tools/grad_plan_dump.cpp reads for one case."""
    if op in ("block", "block_train"):
        return f"{op} {args[0]} {args[1]} {shape[0]} {shape[1]} {shape[2]} {cap}"
    if op == "heads":
        return f"heads {shape[0]} {shape[1]} {shape[2]} {LEVEL_CIN[args[0]]} {HEADS} {cap}"
    return f"{op} {shape[0]} {shape[1]} {shape[2]} {cap}"


def parse(line):
    """One output line of the dump as {key: int} (op stays a string)."""
    out = {}
    for word in line.split():
        k, v = word.split("=", 1)
        out[k] = v if k == "op" else int(v)
    return out


def _split(f, pre, row, frame):
    """The split-K regimes of the GEMM whose fields start with ``pre``; row / frame: pixels of one image row and of
    one frame of the map it sums over."""
    out = set()
    if f["cap"] != 0 or f[pre + ".chunks"] < 2 or f[pre + ".Kc"] != 2048 or f[pre + ".last"] == f[pre + ".Kc"]:
        return out
    if f[pre + ".last"] % 16 == 0:
        out.add("S16")
    elif f[pre + ".last"] > 16 and (f[pre + ".Kc"] % frame) % row != 0:
        out.add("S")
        if f[pre + ".Kc"] >= frame:
            out.add("Sf")
    return out


def _blocks(f, pre, least=64):
    if f[pre + ".pixels"] <= least:
        return set()
    if f[pre + ".last"] < f[pre + ".pixels"]:
        return {"Ps"}
    return {"Pf"} if f[pre + ".blocks"] == 256 else set()


def reached(f):
    """The regimes one parsed dump line reaches (W apart: that one is a statement about a shape, checked through the
    case's ``expect`` fields)."""
    if not f.get("ok"):
        return set()
    op = f["op"]
    out = set()
    if op in ("block", "block_train"):
        row, frame = f["ow"], f["oh"] * f["ow"]
        sets = [_split(f, "wg0", row, frame), _split(f, "wg1", row, frame)]
        if f["downsample"]:
            sets.append(_split(f, "wg2", row, frame))
        out |= set.intersection(*sets)  # every weight gradient of the block
        if out & {"S", "S16"} and f["stride"] == 2 and f["h"] % 2 and f["w"] % 2:
            out.add("O")
        if op == "block":
            out |= _blocks(f, "bs")
        else:
            out |= _blocks(f, "fst") & _blocks(f, "st")  # the forward's statistics and the backward's two sums
    elif op == "neck":
        # dW1b, dW2, dW3 over levels 1, 2, 3 (dW1a runs over level 0, a quarter of level 1)
        for i in (1, 2, 3):
            out |= _split(f, f"wg{i}", f["w4"] << i, f[f"npix{i}"] // f["B"])
        if not all(f[f"wg{i}.chunks"] >= 2 for i in (1, 2, 3)):
            out -= {"S", "S16", "Sf"}
        for i in (0, 1, 2):
            out |= _blocks(f, f"bs{i}")
    elif op == "stem":
        out |= _split(f, "wg", f["ow"], f["oh"] * f["ow"])
        out |= _blocks(f, "bs")
        if (f["dg.passes"] >= f["dg.blocks"] + 2 and f["dg.last"] < f["dg.pixels"] and f["B"] == 2
                and f["dg.blocks"] * f["dg.pixels"] >= f["H"] * f["W"]):
            out.add("G")
    elif op == "heads":
        if f["dh_pixels"] > 32 and f["dh_last"] < f["dh_pixels"]:
            out.add("Ph")
        if f["cap"] == 0 and f["chunks_per_frame"] >= 2 and f["last_rows"] < f["rows_per_chunk"] and f["B"] == 2:
            out.add("R")
    return out


# The search boxes of the minimality claim: per (operator, regime) the frames and the ranges of the two sizes (both
# ends included).  "Smallest" is by the pixels the regime's sums run over (output pixels of a block, level-0 pixels of
# the neck, conv-map pixels of the stem, image pixels for G, map pixels of the heads).
BOXES = {
    ("block", "S"): (1, (1, 72), (1, 72)), ("block", "Sf"): (2, (1, 72), (1, 72)),
    ("block2", "S"): (1, (1, 144), (1, 144)), ("block2", "Sf"): (2, (1, 144), (1, 144)),
    ("neck", "S"): (1, (1, 64), (1, 64)),
    ("stem", "S"): (1, (1, 144), (1, 144)),
    ("block", "Ps"): (1, (64, 160), (64, 160)), ("block", "Pf"): (1, (64, 160), (64, 160)),
    ("stem", "Ps"): (1, (128, 320), (128, 320)),
    ("heads", "Ph"): (1, (128, 200), (128, 200)),
    ("heads", "R"): (2, (1, 72), (1, 72)),
    ("stem", "G"): (2, (448, 576), (448, 576)),
}
