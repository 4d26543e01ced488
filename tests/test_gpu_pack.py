"""sfa_pack_weights_device(_ex) on the GPU: the bytes of the host pack (pack_state_dict) for the same state, for
every unit kind and every rounding rule of the pack, written entirely (the buffer starts as 0xFF), the same
twice, through a captured graph after the state moved in place; argument errors write nothing.  Each case is
one whole-model pack: the architecture fixes the size."""
import ctypes

import numpy as np
import pytest
import torch

import headset_cases as hc
from pack_cases import CASES, edge_state
from sfa_hip import _lib, runtime

pytestmark = pytest.mark.gpu

E_INVALID = -1  # include/sfa_hip.h sfa_status

_SHARED = {}


def case(name, gpu):
    """(arch, state tensors on the GPU in layout order, the host pack as bytes), computed once per case."""
    if name not in _SHARED:
        family, heads = CASES[name]
        arch = hc.make_arch(heads, family)
        sd = edge_state(arch)
        tensors = [torch.zeros((), dtype=torch.int64, device=gpu) if n.endswith("num_batches_tracked")
                   else torch.from_numpy(np.ascontiguousarray(sd[n], np.float32)).to(gpu) for n, _ in _lib.state_layout(arch)]
        want = runtime.pack_state_dict(sd, arch).view(np.uint8)
        want.setflags(write=False)
        _SHARED[name] = (arch, tensors, want)
    return _SHARED[name]


def device_pack(arch, tensors, gpu):
    n = int(_lib.arch_fn(arch, "sfa_packed_floats")(ctypes.byref(arch)))
    out = torch.full((n * 4,), 0xFF, dtype=torch.uint8, device=gpu)  # an unwritten byte shows
    with torch.cuda.device(gpu):
        runtime._pack_on_device(arch, tensors, out.view(torch.float32), _lib.stream_ptr(gpu))
        torch.cuda.synchronize()
    return out.cpu().numpy()


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else (int(bad.size), int(bad[0]) // 4, got[bad[0] // 4 * 4:][:4].tolist(),
                                       want[bad[0] // 4 * 4:][:4].tolist())


def test_edge_state_is_in_contract():
    arch = hc.make_arch(*CASES["five"][::-1])
    sd = edge_state(arch)
    for n, v in sd.items():
        if not n.endswith("num_batches_tracked"):
            a = np.abs(np.asarray(v, np.float32))
            assert np.all(np.isfinite(a)) and np.all((a == 0) | (a >= np.finfo(np.float32).tiny)), n


@pytest.mark.parametrize("name", list(CASES))
def test_device_pack_is_the_host_pack_byte_for_byte(gpu, name):
    arch, tensors, want = case(name, gpu)
    got = device_pack(arch, tensors, gpu)
    assert got.size == want.size
    assert first_difference(got, want) is None, first_difference(got, want)


def test_two_packs_give_equal_bytes(gpu):
    arch, tensors, _ = case("five", gpu)
    assert np.array_equal(device_pack(arch, tensors, gpu), device_pack(arch, tensors, gpu))


def test_captured_repack_reads_the_state_at_replay(gpu):
    """A graph captured around KfpnEngine.repack, replayed after the state tensors changed in place, packs the
    new state; from_state gives the host pack too."""
    arch, tensors, want = case("five", gpu)
    tensors = [t.clone() for t in tensors]
    with torch.cuda.device(gpu):
        eng = runtime.KfpnEngine.from_state(arch, tensors, gpu)
        torch.cuda.synchronize()
        assert first_difference(eng.weights.cpu().numpy().view(np.uint8), want) is None
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            eng.repack(tensors)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            assert eng.repack(tensors) is eng
        layout = _lib.state_layout(arch)
        sd2 = {}
        for (n, _), t in zip(layout, tensors):
            if not n.endswith("num_batches_tracked"):
                t.mul_(1.25).add_(0.001)
                sd2[n] = t.cpu().numpy()
        eng.weights.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        got = eng.weights.cpu().numpy().view(np.uint8)
    want2 = runtime.pack_state_dict(sd2, arch).view(np.uint8)
    assert first_difference(got, want2) is None, first_difference(got, want2)
    assert first_difference(got, want) is not None


def test_argument_errors_write_nothing(gpu):
    arch, tensors, _ = case("five", gpu)
    L = _lib.lib()
    layout = _lib.state_layout(arch)
    n = len(layout)
    floats = int(L.sfa_packed_floats(ctypes.byref(arch)))
    out = torch.full((floats * 4 + 16,), 0xFF, dtype=torch.uint8, device=gpu)
    host = np.zeros(64 * 3 * 7 * 7, np.float32)
    nbt = next(i for i, (name, _) in enumerate(layout) if name.endswith("num_batches_tracked"))

    def table(**change):
        t = (ctypes.c_void_p * n)()
        for i, ((name, _), x) in enumerate(zip(layout, tensors)):
            t[i] = None if name.endswith("num_batches_tracked") else x.data_ptr()
        for i, v in change.items():
            t[int(i[1:])] = v
        return t

    with torch.cuda.device(gpu):
        st = _lib.stream_ptr(gpu)
        calls = {
            "count": (table(), n - 1, out.data_ptr()),
            "null weight": (table(i0=None), n, out.data_ptr()),
            "counter slot": (table(**{f"i{nbt}": tensors[0].data_ptr()}), n, out.data_ptr()),
            "host pointer": (table(i0=host.ctypes.data), n, out.data_ptr()),
            "misaligned": (table(), n, out.data_ptr() + 4),
        }
        for what, (t, count, dst) in calls.items():
            rc = L.sfa_pack_weights_device(ctypes.byref(arch), t, count, dst, st)
            assert rc == E_INVALID and len(L.sfa_last_error_string()) > 0, (what, rc)
        torch.cuda.synchronize()
        assert bool((out == 0xFF).all())
