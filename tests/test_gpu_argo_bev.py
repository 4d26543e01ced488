"""GPU parity of the Argoverse BEV front end (sfa_argo_bev_voxelize, makeBVFeature of
argoverse_test2.py:198-257) against the reference fixtures and the CPU restatement.  Every operation
of the function is order-free (two maxima and a count per cell, one maximum per frame), so every
comparison here is equality of bits: no tolerance anywhere."""
import hashlib

import numpy as np
import pytest
import torch

import argo_bev_cases as ac
import argo_bev_restatement as ar
import golden_cases as gc
import golden_io
from conftest import GOLDEN
from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu

CASES = ac.cases()


@pytest.fixture(scope="module")
def golden_argo():
    return golden_io.load(GOLDEN, "argo_bev_golden")


def _pack(frames, gpu):
    """Frames of one column count packed back to back -> (device points, offsets)."""
    offs = np.cumsum([0] + [f.shape[0] for f in frames])
    return torch.from_numpy(np.concatenate(frames)).to(gpu), offs


def _vox(case, gpu, batch=1, **kw):
    return runtime.ArgoBevVoxelizer(gpu, case["boundary"], case["d"], batch, **kw)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _zero_half_clean(vox):
    """The scratch contract: the first half (the frames' maxima + the atomic path's cells) is zero
    again after every call; the second half (records) may stay dirty."""
    return int(vox.scratch[: vox.scratch.numel() // 2].count_nonzero()) == 0


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_bit_exact_nchw3(golden_argo, gpu, name):
    """The batch of the case's frames equals the reference's maps (bits for cases 1-6, SHA-256 for the
    two large ones), and every frame run alone equals its slot of the batch: nothing leaks between
    frames, the per-frame intensity maximum least of all."""
    case = CASES[name]
    frames = case["frames"]
    vox = _vox(case, gpu, len(frames))
    pts, offs = _pack(frames, gpu)
    got = vox(pts, offs).cpu().numpy()
    assert _zero_half_clean(vox)
    for k, f in enumerate(frames):
        ac.check_frame(golden_argo, f"{name}/{k}", got[k])
        if len(frames) > 1:
            alone = vox(torch.from_numpy(f).to(gpu), [0, f.shape[0]]).cpu().numpy()[0]
            np.testing.assert_array_equal(alone.view(np.uint32), got[k].view(np.uint32))


@pytest.mark.parametrize("name", ["edges", "three_columns", "ragged4", "blocks", "kitti_608"])
@pytest.mark.parametrize("atomic", [False, True])
def test_nhwc4_is_the_transposed_map(gpu, name, atomic):
    case = CASES[name]
    vox = _vox(case, gpu, len(case["frames"]), force_atomic=atomic)
    pts, offs = _pack(case["frames"], gpu)
    nchw = vox(pts, offs, layout=_lib.BEV_NCHW3_F32)
    nhwc = vox(pts, offs, layout=_lib.BEV_NHWC4_F32)
    assert nhwc.shape == (len(case["frames"]),) + tuple(case["shape"]) + (4,)
    np.testing.assert_array_equal(_bits(nhwc[..., :3].permute(0, 3, 1, 2).contiguous()), _bits(nchw))
    assert int(nhwc[..., 3].contiguous().view(torch.int32).count_nonzero()) == 0


@pytest.mark.parametrize("name", ["ragged4", "blocks", "edges", "inexact_d"])
def test_atomic_fallback_gives_the_record_paths_bits(golden_argo, gpu, name):
    case = CASES[name]
    vox = _vox(case, gpu, len(case["frames"]))
    pts, offs = _pack(case["frames"], gpu)
    rec = vox(pts, offs)
    assert _zero_half_clean(vox)
    atom = vox(pts, offs, force_atomic=True)
    assert _zero_half_clean(vox)
    np.testing.assert_array_equal(_bits(atom), _bits(rec))
    for k in range(len(case["frames"])):
        ac.check_frame(golden_argo, f"{name}/{k}", atom[k].cpu().numpy())


def test_records_that_do_not_fit_take_the_atomic_path(gpu):
    """A 32 x 32 map's scratch holds 256 + 12 KiB of records: 3,000 points (3 regions of 10 KiB + table)
    do not fit, so the call falls back to the atomics by itself: same bits as the restatement."""
    cloud = ac.random_cloud(31, 3000, ac.B32, i_lo=-1.0, i_hi=40.0)
    vox = runtime.ArgoBevVoxelizer(gpu, ac.B32, 0.1, 1)
    assert 3 * 1024 * 10 > vox.scratch.numel() // 2
    got = vox(torch.from_numpy(cloud).to(gpu), [0, 3000]).cpu().numpy()[0]
    assert _zero_half_clean(vox)
    np.testing.assert_array_equal(got.view(np.uint32), ar.make_bv_feature(cloud, 0.1, ac.B32).view(np.uint32))


def test_consecutive_calls_on_one_scratch(gpu):
    """Two calls on the same scratch give equal bits, also across batch sizes, paths and an
    interleaved different batch: each call leaves the scratch's zero half clean."""
    case = CASES["blocks"]
    vox = _vox(case, gpu, 2)
    pts, offs = _pack(case["frames"], gpu)
    one = torch.from_numpy(case["frames"][1]).to(gpu)
    a = vox(pts, offs)
    assert _zero_half_clean(vox)
    b = vox(pts, offs)
    assert _zero_half_clean(vox)
    c = vox(one, [0, one.shape[0]])
    d = vox(pts, offs, force_atomic=True)
    assert _zero_half_clean(vox)
    e = vox(pts, offs)
    for other in (b, d, e):
        np.testing.assert_array_equal(_bits(other), _bits(a))
    np.testing.assert_array_equal(_bits(c[0]), _bits(a[1]))


def test_random_clouds_equal_the_restatement(gpu):
    """Twenty seeded clouds at 64 x 64, 0 - 5,000 points, intensities in [-1, 300), as one ragged batch
    and (the first five) as single frames."""
    clouds = ac.random_clouds(20)
    assert clouds[0].shape[0] == 0 and max(c.shape[0] for c in clouds) > 2048
    exp = [ar.make_bv_feature(c, 0.1, ac.B64) for c in clouds]
    vox = runtime.ArgoBevVoxelizer(gpu, ac.B64, 0.1, len(clouds))
    pts, offs = _pack(clouds, gpu)
    got = vox(pts, offs).cpu().numpy()
    for k in range(len(clouds)):
        np.testing.assert_array_equal(got[k].view(np.uint32), exp[k].view(np.uint32), err_msg=f"cloud {k}")
    for k in range(5):
        alone = vox(torch.from_numpy(clouds[k]).to(gpu), [0, clouds[k].shape[0]]).cpu().numpy()[0]
        np.testing.assert_array_equal(alone.view(np.uint32), exp[k].view(np.uint32), err_msg=f"cloud {k} alone")


def test_dropin_make_bv_feature(golden_argo, gpu):
    """numpy in -> numpy out, GPU tensor in -> GPU tensor out, 3 and 5 columns, the reference's signature."""
    from data_process.argoverse_bev_utils import makeBVFeature, makeBVFeatureBatch
    for name in ("edges", "three_columns", "inexact_d"):
        case = CASES[name]
        cloud = case["frames"][0]
        m = makeBVFeature(cloud, case["d"], case["boundary"])
        assert isinstance(m, np.ndarray)
        ac.check_frame(golden_argo, f"{name}/0", m)
        t = makeBVFeature(torch.from_numpy(cloud).to(gpu), case["d"], case["boundary"])
        assert isinstance(t, torch.Tensor) and t.device.type == "cuda"
        ac.check_frame(golden_argo, f"{name}/0", t.cpu().numpy())
    case = CASES["edges"]
    wide = np.concatenate([case["frames"][0], np.full((case["frames"][0].shape[0], 2), 7.0, np.float32)], axis=1)
    ac.check_frame(golden_argo, "edges/0", makeBVFeature(wide, case["d"], case["boundary"]))
    b = makeBVFeatureBatch(torch.from_numpy(wide).to(gpu), [0, wide.shape[0]], case["d"], case["boundary"],
                           layout="nhwc4")
    ac.check_frame(golden_argo, "edges/0", b[0, ..., :3].permute(2, 0, 1).contiguous().cpu().numpy())


def test_graph_replay_equals_eager(gpu):
    """The call neither allocates nor synchronises: captured into a HIP graph, its replays (also after
    other work on the same scratch's zero half was done and undone) equal the eager result."""
    case = CASES["blocks"]
    vox = _vox(case, gpu, 2)
    pts, offs = _pack(case["frames"], gpu)
    out = torch.empty(vox.out_shape(2, _lib.BEV_NHWC4_F32), dtype=torch.float32, device=gpu)
    eager = vox(pts, offs, layout=_lib.BEV_NHWC4_F32).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vox(pts, offs, layout=_lib.BEV_NHWC4_F32, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vox(pts, offs, layout=_lib.BEV_NHWC4_F32, out=out)
    for _ in range(3):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(out), _bits(eager))
        assert _zero_half_clean(vox)


def _engine(gpu):
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    packed = runtime.pack_state_dict(synthetic.synthetic_state_dict(_lib.state_layout(arch), 0), arch)
    return runtime.KfpnEngine(arch, packed, gpu)


@pytest.mark.parametrize("bev_layout", ["nchw3", "nhwc4"])
def test_pipeline_argoverse(gpu, bev_layout):
    """DetectorPipeline(bev="argoverse") at 1 x 160 x 128: its BEV is the stand-alone voxeliser's bit for
    bit, its detections are decode of the same engine's forward on that map, eager and from its graph."""
    cloud = ac.random_cloud(41, 6000, ac.BPIPE, i_lo=-1.0, i_hi=255.0)
    eng = _engine(gpu)
    K = 50
    pipe = runtime.DetectorPipeline(eng, 1, 160, 128, K=K, with_bev=True, max_points=cloud.shape[0],
                                    bev="argoverse", boundary=ac.BPIPE, discretization=0.1, bev_layout=bev_layout)
    pipe.set_points([cloud])
    dets = pipe.run().clone()
    alone = runtime.ArgoBevVoxelizer(gpu, ac.BPIPE, 0.1, 1)(torch.from_numpy(cloud).to(gpu), [0, cloud.shape[0]])
    np.testing.assert_array_equal(alone.cpu().numpy()[0].view(np.uint32),
                                  ar.make_bv_feature(cloud, 0.1, ac.BPIPE).view(np.uint32))
    bev = pipe.bev if bev_layout == "nchw3" else pipe.bev[..., :3].permute(0, 3, 1, 2).contiguous()
    np.testing.assert_array_equal(_bits(bev), _bits(alone))
    if bev_layout == "nchw3":
        o = eng.forward(alone)
    else:  # the same input layout as the pipeline's forward
        o = eng.forward(runtime.ArgoBevVoxelizer(gpu, ac.BPIPE, 0.1, 1)(
            torch.from_numpy(cloud).to(gpu), [0, cloud.shape[0]], layout=_lib.BEV_NHWC4_F32), _lib.IN_NHWC4)
    exp = runtime.decode(o["hm_cen"], o["cen_offset"], o["direction"], o["z_coor"], o["dim"], K=K, apply_sigmoid=True)
    np.testing.assert_array_equal(_bits(dets), _bits(exp))
    pipe.capture()
    pipe.bev.fill_(float("nan"))
    pipe.dets.zero_()
    replayed = pipe.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(replayed), _bits(exp))
    bev = pipe.bev if bev_layout == "nchw3" else pipe.bev[..., :3].permute(0, 3, 1, 2).contiguous()
    np.testing.assert_array_equal(_bits(bev), _bits(alone))


def test_default_pipeline_is_still_kitti(golden, gpu):
    """A default (KITTI) pipeline built in the same process as an Argoverse one still gives the KITTI
    fixture's map: the f64 voxeliser's SHA is the fixture's, and the pipeline's f32 map is that map."""
    name, cloud = gc.bev_cases(golden.bev)[0]
    eng = _engine(gpu)
    argo = runtime.DetectorPipeline(eng, 1, 160, 128, with_bev=True, max_points=100, bev="argoverse",
                                    boundary=ac.BPIPE, discretization=0.1)
    argo.set_points([ac.random_cloud(42, 100, ac.BPIPE)])
    argo.run()
    pipe = runtime.DetectorPipeline(eng, 1, with_bev=True, max_points=cloud.shape[0])
    assert pipe.bev_kind == "kitti" and isinstance(pipe.vox, runtime.BevVoxelizer) and pipe.boundary == gc.BOUNDARY
    pipe.set_points([cloud])
    pipe.run()
    f64 = runtime.BevVoxelizer(gpu, 1)(torch.from_numpy(cloud).to(gpu), [0, cloud.shape[0]], gc.BOUNDARY,
                                       layout=_lib.BEV_NCHW3_F64).cpu().numpy()[0]
    assert hashlib.sha256(np.ascontiguousarray(f64).tobytes()).hexdigest() == str(golden.bev[f"{name}/map_sha"])
    np.testing.assert_array_equal(pipe.bev.cpu().numpy()[0], f64.astype(np.float32))
