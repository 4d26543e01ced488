"""sfa_build_targets against the reference fixture (tests/golden/gen_loss_golden.py) and the numpy
restatement: indices, masks and status exactly, the 1.0 / 0.9999 / 0.0 cells the same cells, every float
within one float32 ulp (the device's float64 exp / sin / cos against glibc's, rounded to float32, can differ
only at a rounding midpoint; the count of non-identical values is printed)."""
import numpy as np
import pytest
import torch

import golden_io
import loss_restatement as lr
from conftest import GOLDEN
from sfa_hip import runtime, synthetic
from test_loss_host import C, CASES, M

pytestmark = pytest.mark.gpu
FLOAT_KEYS = ("hm_cen", "cen_offset", "direction", "z_coor", "dim")


@pytest.fixture(scope="module")
def g():
    return golden_io.load(GOLDEN, "loss_golden")


def _builder(gpu, hm_size, num_classes=C, max_objects=M):
    return runtime.TargetBuilder(gpu, lr.BOUNDARY, hm_size, num_classes, max_objects)


def _host(t):
    return {k: v.cpu().numpy() for k, v in t.items()}


def _compare(got, ref, what):
    np.testing.assert_array_equal(got["indices_center"], ref["indices_center"])
    np.testing.assert_array_equal(got["obj_mask"], ref["obj_mask"])
    for v in (np.float32(1.0), np.float32(0.9999), np.float32(0.0)):
        np.testing.assert_array_equal(got["hm_cen"] == v, ref["hm_cen"] == v)
    differ = 0
    for k in FLOAT_KEYS:
        a, b = got[k], ref[k]
        assert a.dtype == np.float32 and a.shape == b.shape, k
        differ += int((a.view(np.uint32) != b.view(np.uint32)).sum())
        assert np.all(np.abs(a.astype(np.float64) - b) <= np.spacing(np.abs(b))), k
    print(f"build_targets[{what}]: {differ} float32 values not bit-identical")


@pytest.mark.parametrize("name", CASES)
def test_targets_match_the_reference(g, gpu, name):
    tb = _builder(gpu, tuple(g[f"{name}/hm_size"]))
    got = tb(g[f"{name}/labels"], g[f"{name}/offsets"].tolist(), g[f"{name}/flips"].tolist())
    np.testing.assert_array_equal(tb.status.cpu().numpy().view(np.uint32), g[f"{name}/status"])
    _compare(_host(got), {k: g[f"{name}/t/{k}"] for k in lr.KEYS}, name)


def _labels_152():
    labels, offsets = synthetic.synthetic_labels(2, seed=5, max_per_frame=60)
    extra = np.float32([[1, 50.0, 3.0, -1.0, 1.5, 1.6, 3.9, 0.2],       # x == maxX: center_int[1] == hm_h
                        [0, 0.0, -25.0, -1.0, 1.5, 2.0, 4.5, 1.0]])     # the map's corner
    labels = np.concatenate([extra, labels])
    return labels, np.int64([0, offsets[1] + 2, offsets[2] + 2])


def test_full_size_map_matches_the_restatement(gpu):
    """152 x 152, B = 2, the production shape (C = 3, M = 50): 68 blocks per frame, one frame flipped."""
    labels, offsets = _labels_152()
    tb = _builder(gpu, (152, 152), 3, 50)
    got = _host(tb(labels, offsets.tolist(), [False, True]))
    ref, status = lr.build_targets_batch(labels, offsets, [False, True], hm_size=(152, 152), num_classes=3,
                                         max_objects=50)
    np.testing.assert_array_equal(tb.status.cpu().numpy().view(np.uint32), status)
    assert status[0] & 1 and ref["obj_mask"].sum() > 10 and (ref["hm_cen"] == np.float32(0.9999)).any()
    _compare(got, ref, "152x152")


def test_graph_replay_equals_eager(g, gpu):
    name = "misc2432"
    tb = _builder(gpu, tuple(g[f"{name}/hm_size"]))
    labels = torch.from_numpy(g[f"{name}/labels"]).to(gpu)
    offsets = torch.from_numpy(g[f"{name}/offsets"]).to(gpu)
    flips = g[f"{name}/flips"].tolist()
    eager = {k: v.clone() for k, v in tb(labels, offsets, flips).items()}
    out = tb.alloc(3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tb(labels, offsets, flips, out=out, verify=False)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tb(labels, offsets, flips, out=out, verify=False)
    for t in out.values():
        t.fill_(7)  # every byte is written by the call: nothing needs zeroing
    graph.replay()
    torch.cuda.synchronize()
    for k in lr.KEYS:
        assert torch.equal(out[k], eager[k]), k
    # new labels under the same graph: the offsets and rows are read on the device
    labels.copy_(labels.flip(0))
    graph.replay()
    again = tb(labels, offsets, flips)
    for k in lr.KEYS:
        assert torch.equal(out[k], again[k]), k


def test_out_of_map_centre_writes_nothing_out_of_range(g, gpu):
    """x == maxX (center_int[1] == hm_h) and a flipped y == maxY (center_int[0] == -1): status bit 0, the
    reference's index stored, and the guard words around every output untouched."""
    name = "outmap2432"
    H, W = (int(v) for v in g[f"{name}/hm_size"])
    B, G = 2, 1024
    tb = _builder(gpu, (H, W))
    shapes = tb.alloc(B)
    flat, out = {}, {}
    for k, t in shapes.items():
        sentinel = 77 if t.dtype != torch.float32 else -5.0
        flat[k] = torch.full((t.numel() + 2 * G,), sentinel, dtype=t.dtype, device=gpu)
        out[k] = flat[k][G:G + t.numel()].view(t.shape)
    tb(g[f"{name}/labels"], g[f"{name}/offsets"].tolist(), g[f"{name}/flips"].tolist(), out=out)
    torch.cuda.synchronize()
    assert tb.status.cpu().tolist() == [1, 1]
    for k, f in flat.items():
        sentinel = 77 if f.dtype != torch.float32 else -5.0
        assert bool((f[:G] == sentinel).all()) and bool((f[-G:] == sentinel).all()), k
    ind = out["indices_center"].cpu().numpy()
    np.testing.assert_array_equal(ind, g[f"{name}/t/indices_center"])
    assert ind[0, 1] >= H * W
    _compare(_host(out), {k: g[f"{name}/t/{k}"] for k in lr.KEYS}, name + " guarded")


def test_bad_class_sets_status_and_raises(gpu):
    rows = np.float32([[3, 10, 0, -1, 1.5, 1.6, 3.9, 0], [-5, 12, 1, -1, 1.5, 1.6, 3.9, 0],
                       [7, 60, 0, -1, 1.5, 1.6, 3.9, 0], [1, 20, 2, -1, 1.5, 1.6, 3.9, 0]])
    tb = _builder(gpu, (16, 16))
    out = tb(rows, [0, 2, 4], verify=False)  # frame 1: the bad class is outside the boundary, so never indexed
    assert tb.status.cpu().tolist() == [2, 0]
    assert int(out["obj_mask"][0].sum()) == 0 and int(out["obj_mask"][1].sum()) == 1
    assert float(out["hm_cen"][0].abs().max()) == 0.0
    with pytest.raises(IndexError, match="class id"):
        tb(rows, [0, 2, 4])
