"""The Argoverse scripts' own configuration end to end: +-40 m at 0.1 m cells is an 800 x 800 input
and a 200 x 200 heat map (40,000 cells), which the decode refused before the tiled form
("decode: H*W = 40000 exceeds 36864").  One synthetic sweep goes points -> makeBVFeature -> forward
-> decode on the device; every comparison is equality of bits."""
import numpy as np
import pytest
import torch

from oracle import decode_oracle
from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def test_pipeline_at_the_scripts_configuration(gpu):
    cloud = synthetic.synthetic_argoverse_sweep(5, 20_000)
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    packed = runtime.pack_state_dict(synthetic.synthetic_state_dict(_lib.state_layout(arch), 0), arch)
    eng = runtime.KfpnEngine(arch, packed, gpu)
    K = 50
    pipe = runtime.DetectorPipeline(eng, 1, 800, 800, K=K, with_bev=True, max_points=cloud.shape[0], bev="argoverse",
                                    boundary=runtime.ARGO_BOUNDARY, discretization=0.1)
    pipe.set_points([cloud])
    dets = pipe.run().clone()
    alone = runtime.ArgoBevVoxelizer(gpu, runtime.ARGO_BOUNDARY, 0.1, 1)(torch.from_numpy(cloud).to(gpu),
                                                                         [0, cloud.shape[0]])
    np.testing.assert_array_equal(_bits(pipe.bev), _bits(alone))
    o = {k: v.clone() for k, v in pipe.outs.items()}
    assert tuple(o["hm_cen"].shape) == (1, 3, 200, 200)
    hm = runtime.sigmoid_clamp_(o["hm_cen"].clone()).cpu().numpy()
    off = runtime.sigmoid_clamp_(o["cen_offset"].clone()).cpu().numpy()
    exp = decode_oracle.decode(hm, off, o["direction"].cpu().numpy(), o["z_coor"].cpu().numpy(),
                               o["dim"].cpu().numpy(), K=K)
    np.testing.assert_array_equal(dets.cpu().numpy(), exp)
    pipe.capture()
    pipe.bev.fill_(float("nan"))
    pipe.dets.zero_()
    replayed = pipe.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(pipe.bev), _bits(alone))
    np.testing.assert_array_equal(replayed.cpu().numpy(), exp)
