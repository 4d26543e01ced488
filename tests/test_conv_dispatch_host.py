"""The body-conv rule table (csrc/conv_plan.h body_conv_rule, which csrc/conv.hip launch_conv_h switches on) against
the GPU case table of tests/conv_dispatch_cases.py, on the CPU: tools/conv_plan_check --rules prints the rule of the
sixteen residual-layer convs at every input that is a multiple of 32 up to 2048 x 2048 (built as csrc/model.hip builds
them), --block those of block_forward's two launches on a caller's map (as csrc/block.hip builds them).  The walk
itself (every chosen instance's own check accepts the launch, strip_tile_bn agrees, the rule is the same at B = 1 and
B = 181 and in block_forward) runs under ASan + UBSan in tests/test_bev_plan_host.py."""
import os
import shutil
import subprocess

import pytest

import conv_dispatch_cases as cd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = [(L, b) for L in (1, 2, 3, 4) for b in (0, 1)]


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("conv_dispatch") / "conv_plan_check")
    r = subprocess.run([gxx, "-std=c++17", "-O1", os.path.join(REPO, "tools", "conv_plan_check.cpp"), "-pthread", "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _lines(tool, *args):
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    out = {}
    for line in r.stdout.splitlines():
        key, rule = line.split(" -> ")
        out[tuple(int(v) for v in key.split())] = rule  # (layer, block, conv, h, w)
    return out


@pytest.fixture(scope="module")
def model_rules(tool):
    rules = _lines(tool, "--rules")
    assert len(rules) == 16 * 64 * 64
    return rules


def _block_rules(tool, layer, block, h, w, B=cd.BATCH):
    got = _lines(tool, "--block", layer, block, B, h, w)
    return got[(layer, block, 1, h, w)], got[(layer, block, 2, h, w)]


def test_case_table_reaches_every_reachable_rule(tool, model_rules):
    reachable = set(model_rules.values())
    covered = set()
    for (layer, block, (h, w)), want in cd.BLOCK_CASES:
        got = _block_rules(tool, layer, block, h, w)
        assert got == want, (layer, block, h, w, got)
        assert got == _block_rules(tool, layer, block, h, w, B=1), "the rule depends on the batch"
        covered.update(got)
    print("reachable up to 2048 x 2048:", sorted(reachable))
    assert "none" not in reachable
    assert reachable <= covered, f"no GPU case runs {sorted(reachable - covered)}"
    # the whole-model cases run what the table says of them, and between them every rule only a large map reaches
    for (H, W), layers in cd.MODEL_CASES.items():
        for layer, want in layers.items():
            got = tuple(model_rules[(layer, k >> 1, (k & 1) + 1, H, W)] for k in range(4))
            assert got == want, (H, W, layer, got)
    small = {r for (_, _, _, H, W), r in model_rules.items() if H * W <= 608 * 608}
    large_only = reachable - small
    assert large_only == {"strip_128x128_ks2", "r3_body_ks2"}, large_only
    in_models = {r for layers in cd.MODEL_CASES.values() for want in layers.values() for r in want}
    assert large_only <= in_models


@pytest.mark.parametrize("layer,small,large", [(3, ("strip_64x128", "h3_128x128"), ("strip_128x128", "r3_body")),
                                               (4, ("strip_128x64_ks2", "h3_128x128_ks2"), ("strip_128x128_ks2", "r3_body_ks2"))])
def test_both_sides_of_the_map_size_threshold(tool, layer, small, large):
    """3125 = 25 x 125 pixels a frame take the large-map rule, 3124 = 44 x 71 the small-map one: block 1 (the strip
    instances) and block 0 (R3_BODY against conv_h3), at even and odd stride-2 inputs."""
    assert _block_rules(tool, layer, 1, 25, 125) == (large[0],) * 2
    assert _block_rules(tool, layer, 1, 44, 71) == (small[0],) * 2
    for h, w in ((50, 250), (49, 249), (50, 249)):
        assert _block_rules(tool, layer, 0, h, w) == (large[1],) * 2, (h, w)
    for h, w in ((88, 142), (87, 141)):
        assert _block_rules(tool, layer, 0, h, w) == (small[1],) * 2, (h, w)


def test_strip_minimum_of_128_rows(tool):
    for layer, at, below in ((1, "strip_128x64", "h3_256x64"), (2, "strip_128x128", "h3_128x128"),
                             (3, "strip_64x128", "h3_128x128"), (4, "strip_128x64_ks2", "h3_128x128_ks2")):
        assert _block_rules(tool, layer, 1, 8, 16) == (at,) * 2  # 128 rows
        assert _block_rules(tool, layer, 1, 7, 18) == (below,) * 2  # 126


def test_whole_model_thresholds(model_rules):
    """The layer3 map reaches 3125 pixels at H W >= 800,000 (896 x 896; 800 x 800 stays below), layer4's at 3,200,000
    (1792 x 1792); the rule of a conv depends on the map's pixel count alone, not on its aspect."""
    def rule(layer, k, H, W):
        return model_rules[(layer, k >> 1, (k & 1) + 1, H, W)]
    for (layer, block, conv, H, W), r in model_rules.items():
        pix = (H >> (layer + 1)) * (W >> (layer + 1))
        if layer == 1:
            assert r == ("strip_128x64" if pix >= 128 else "h3_256x64")
        elif block == 1:
            want = {2: ("strip_128x128",) * 2, 3: ("strip_64x128", "strip_128x128"),
                    4: ("strip_128x64_ks2", "strip_128x128_ks2")}[layer][pix >= 3125]
            assert r == (want if pix >= 128 else ("h3_128x128_ks2" if layer == 4 else "h3_128x128")), (layer, H, W, r)
        else:
            want = ("h3_128x128", "r3_body") if layer < 4 else ("h3_128x128_ks2", "r3_body_ks2")
            assert r == want[pix >= 3125], (layer, H, W, r)
    assert rule(3, 2, 864, 896) == "strip_64x128" and rule(3, 2, 896, 896) == "strip_128x128"
    assert rule(4, 2, 1760, 1792) == "strip_128x64_ks2" and rule(4, 2, 1792, 1792) == "strip_128x128_ks2"
