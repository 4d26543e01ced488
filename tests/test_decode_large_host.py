"""Host-side contract of the tiled decode (no GPU): the new symbols are exported, the map-aware
workspace size equals the old one wherever the old kernels serve the shape, grows with the map
above 36,864 cells, and is 0 for a shape sfa_decode refuses."""
import pytest

from sfa_hip import _lib

BAND_SHAPES = [(3, 3, 37, 29, 50), (2, 3, 10, 10, 50), (1, 1, 152, 152, 256), (2, 16, 24, 24, 256),
               (1, 3, 3, 4100, 40), (2, 3, 152, 152, 50)]  # test_gpu_decode.test_decode_band_split_shapes


def test_new_symbols_are_exported():
    L = _lib.lib()
    for name in ("sfa_decode_workspace_size_hw", "sfa_topk_workspace_size_hw", "sfa_argo_project_boxes",
                 "sfa_argo_project_points"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.sfa_abi_version() == 2


@pytest.mark.parametrize("B,C,H,W,K", BAND_SHAPES + [(16, 3, 152, 152, 50), (1, 1, 192, 192, 50)])
def test_size_is_the_old_one_where_the_old_kernels_serve(B, C, H, W, K):
    L = _lib.lib()
    assert L.sfa_decode_workspace_size_hw(B, C, H, W, K) == L.sfa_decode_workspace_size(B, C, K)
    assert L.sfa_topk_workspace_size_hw(B, C, H, W, K) == L.sfa_topk_workspace_size(B, C, K)


def test_size_grows_with_the_map_above_the_limit():
    L = _lib.lib()
    # the size follows the number of tiles: 193 x 192 and 200 x 200 are both 10 tiles of <= 20 rows
    sizes = [L.sfa_decode_workspace_size_hw(2, 3, H, W, 50) for H, W in ((193, 192), (200, 200), (304, 304), (512, 512))]
    assert 0 < sizes[0] <= sizes[1] < sizes[2] < sizes[3]
    assert sizes[3] > L.sfa_decode_workspace_size(2, 3, 50)  # which has no map size and cannot grow
    # tile lists (NT per class) + one class list, keys and indices: 200 x 200 is 10 tiles of 20 rows
    assert L.sfa_decode_workspace_size_hw(2, 3, 200, 200, 50) >= 2 * 3 * (10 + 1) * 50 * 8
    assert L.sfa_decode_workspace_size_hw(1, 1, 512, 512, 256) >= (64 + 1) * 256 * 8
    assert L.sfa_topk_workspace_size_hw(2, 3, 200, 200, 50) == L.sfa_decode_workspace_size_hw(2, 3, 200, 200, 50)
    # any aspect up to 512 x 512 cells
    for H, W in ((1, 40000), (40000, 1), (3, 16384), (16384, 3), (1, 262144), (262144, 1)):
        assert L.sfa_decode_workspace_size_hw(1, 2, H, W, 7) > 0


@pytest.mark.parametrize("B,C,H,W,K", [(1, 3, 513, 512, 50), (1, 3, 1024, 1024, 50), (1, 3, 200, 200, 257),
                                       (1, 17, 200, 200, 50), (0, 3, 200, 200, 50), (1, 3, 0, 200, 50),
                                       (1, 3, 2, 2, 5), (1, 3, 65536, 65536, 5)])
def test_size_is_zero_for_unsupported_shapes(B, C, H, W, K):
    assert _lib.lib().sfa_decode_workspace_size_hw(B, C, H, W, K) == 0
