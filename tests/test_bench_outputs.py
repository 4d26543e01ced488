"""bench.py's plain run and ``--dump-outputs``: a plain run prints the headline line only (what takes
runs of its own is behind ``--full``), and the dumped arrays are the last timed step's outputs."""
import json
import sys

import numpy as np
import pytest

import bench
from sfa_hip.runtime import DEFAULT_HEADS

TOL = 1e-4
FULL_ONLY = ("stages_ms", "roofline", "bev_roofline", "cpu_baseline", "parity")


def test_full_and_dump_outputs_are_off_by_default():
    args = bench.parse([])
    assert args.full is False and args.dump_outputs is None
    args = bench.parse(["--full", "--dump-outputs", "d", "--steps", "7"])
    assert args.full is True and args.dump_outputs == "d" and args.steps == 7


def test_write_outputs_float32_files(tmp_path):
    d = tmp_path / "a" / "b"
    bench.write_outputs(str(d), {"x": np.arange(6, dtype=np.int64).reshape(2, 3), "y": np.ones(4, np.float64)})
    x, y = np.load(d / "x.npy"), np.load(d / "y.npy")
    assert x.dtype == np.float32 and y.dtype == np.float32
    np.testing.assert_array_equal(x, np.arange(6).reshape(2, 3))
    assert sorted(p.name for p in d.iterdir()) == ["x.npy", "y.npy"]


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(gpu, golden_bench, tmp_path, monkeypatch, capsys):
    """``bench.py --steps 3 --warmup 1 --dump-outputs DIR`` in this process: one line with the headline
    fields and none of the ``--full`` ones; DIR holds the timed batch's detections and head maps, which
    match the reference's forward + decode of that batch (tests/golden/bench_golden: sampled logits
    within 1e-4 * max(1, |ref|), every frame's sorted scores within 1e-4)."""
    out = tmp_path / "dump"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                                      "--dump-outputs", str(out)])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    ln = lines[0]
    assert ln["metric"] == bench.METRIC and ln["unit"] == "frames/s" and ln["higher_is_better"] is True
    assert ln["steps"] == 3 and ln["warmup"] == 1 and ln["n_gpus"] == 1 and ln["dtype"] == bench.DTYPES["fp16x3"]
    assert ln["value"] > 0 and ln["ms_per_step"] > 0
    # value = frames / elapsed and ms_per_step = elapsed / steps describe the same 3 steps
    assert abs(ln["value"] * ln["ms_per_step"] / (16 * 1e3) - 1) < 1e-3
    assert not any(k in ln for k in FULL_ONLY), sorted(ln)
    assert sorted(p.name for p in out.iterdir()) == sorted(["dets.npy"] + [h + ".npy" for h in DEFAULT_HEADS])
    g = golden_bench
    ys, xs = g["sample_yx"]
    total = 0
    for h, c in DEFAULT_HEADS.items():
        o = np.load(out / f"{h}.npy")
        total += o.nbytes
        assert o.dtype == np.float32 and o.shape == (16, c, 152, 152)
        r = g[f"bench/{h}/samples"]
        assert float(np.max(np.abs(o[:, :, ys, xs] - r) / np.maximum(1.0, np.abs(r)))) <= TOL, h
    dets = np.load(out / "dets.npy")
    assert dets.dtype == np.float32 and dets.shape == (16, 50, 10)
    assert total + dets.nbytes <= 64 << 20
    ref = g["bench/dets"]
    assert float(np.max(np.abs(np.sort(dets[..., 0], axis=1) - np.sort(ref[..., 0], axis=1)))) <= TOL
