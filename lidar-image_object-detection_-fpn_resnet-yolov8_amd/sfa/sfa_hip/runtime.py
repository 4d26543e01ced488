"""Host runtime over the C ABI: weight packing, engines, device buffers, streams.

torch is used only as plumbing (device memory, the current HIP stream, graph
capture); every computation on the hot path is a libsfa_hip kernel.
"""

from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import SfaNativeError, check, lib

DEFAULT_HEADS = {"hm_cen": 3, "cen_offset": 2, "direction": 2, "z_coor": 1, "dim": 3}
DEFAULT_BOUNDARY = {"minX": 0, "maxX": 50, "minY": -25, "maxY": 25, "minZ": -2.73, "maxZ": 1.27}
# config/kitti_config.py:35-42 boundary_back (demo_2_sides.py's rear view)
DEFAULT_BOUNDARY_BACK = {"minX": -50, "maxX": 0, "minY": -25, "maxY": 25, "minZ": -2.73, "maxZ": 1.27}


def _require_gpu_tensor(t: torch.Tensor, what: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise SfaNativeError(f"{what}: the HIP path needs a tensor on a GPU device "
                             f"(got {getattr(t, 'device', type(t))}); there is no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{what}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


def host_api_device(what: str, device=None) -> torch.device:
    """The GPU a numpy-in / numpy-out host API (makeBEVMap, get_filtered_lidar) runs on: ``device``
    or the current one. Raises SfaNativeError with the fix when no GPU is visible or when called in a
    process forked after HIP was initialised — a DataLoader worker of a caller that created its model
    first (test.py:112 then :120): HIP cannot be used there, and the drop-in's
    data_process.kitti_dataloader voxelises each batch in the main process instead."""
    if device is not None:
        return torch.device(device)
    if torch.cuda._is_in_bad_fork():
        raise SfaNativeError(
            f"{what} runs on the GPU (HIP), but this process was forked after HIP was initialised "
            "(a DataLoader worker): create the loader with the drop-in data_process.kitti_dataloader "
            "(create_test_dataloader / create_val_dataloader / create_train_dataloader: the workers only "
            "read files, the BEV maps are made per batch in the main process) or use num_workers=0")
    if not torch.cuda.is_available():
        raise SfaNativeError(f"{what} runs on the GPU (HIP); no GPU is visible")
    return torch.device("cuda", torch.cuda.current_device())


def _boundary_arr(boundary: dict):
    vals = [boundary[k] for k in ("minX", "maxX", "minY", "maxY", "minZ", "maxZ")]
    return (ctypes.c_double * 6)(*[float(v) for v in vals])


# ------------------------------------------------------------------ weights
def pack_state_dict(state: dict, arch) -> np.ndarray:
    """Reference-format state_dict (tensors or arrays) -> packed float32 host array."""
    layout = _lib.state_layout(arch)
    parts = []
    for name, shape in layout:
        if name.endswith("num_batches_tracked"):
            continue
        if name not in state:
            raise KeyError(f"state_dict is missing {name}")
        v = state[name]
        v = v.detach().to("cpu", torch.float32).numpy() if isinstance(v, torch.Tensor) else np.asarray(
            v, np.float32)
        if tuple(v.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(v.shape)} != {tuple(shape)}")
        parts.append(np.ascontiguousarray(v, np.float32).reshape(-1))
    flat = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    nfl = _lib.arch_fn(arch, "sfa_state_floats")(ctypes.byref(arch))
    if flat.size != nfl:
        raise ValueError(f"state has {flat.size} floats, expected {nfl}")
    packed = np.zeros(_lib.arch_fn(arch, "sfa_packed_floats")(ctypes.byref(arch)), np.float32)
    check(_lib.arch_fn(arch, "sfa_pack_weights")(ctypes.byref(arch), flat.ctypes.data, flat.size, packed.ctypes.data),
          "sfa_pack_weights")
    return packed


_LAYOUTS = {}  # descriptor bytes -> state layout (the descriptor is a plain struct)


def _cached_layout(arch):
    key = (type(arch).__name__, bytes(arch))
    lay = _LAYOUTS.get(key)
    if lay is None:
        lay = _LAYOUTS[key] = _lib.state_layout(arch)
    return lay


def state_entries(arch) -> int:
    """Entries of the reference state_dict of this descriptor (sfa_state_count(_ex))."""
    return len(_cached_layout(arch))


def device_packable(tensors, device) -> bool:
    """Every float state tensor is a contiguous float32 tensor on ``device`` (what sfa_pack_weights_device reads)."""
    device = torch.device(device)
    if device.type != "cuda":
        return False
    if device.index is None:  # "cuda": the current device, as a tensor's .device names it
        device = torch.device("cuda", torch.cuda.current_device())
    return all(
        not t.is_floating_point() or (t.dtype == torch.float32 and t.device == device and t.is_contiguous())
        for t in tensors)


def _pack_on_device(arch, tensors, packed: torch.Tensor, stream: int):
    """sfa_pack_weights_device(_ex) of the state ``tensors`` (layout order) into ``packed`` on ``stream``."""
    layout = _cached_layout(arch)
    if len(tensors) != len(layout):
        raise ValueError(f"state has {len(tensors)} tensors, the layout {len(layout)}")
    table = (ctypes.c_void_p * len(layout))()
    for i, ((name, shape), t) in enumerate(zip(layout, tensors)):
        if name.endswith("num_batches_tracked"):
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != packed.device:
            raise ValueError(f"{name}: the device pack reads contiguous float32 tensors on {packed.device}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(t.shape)} != {tuple(shape)}")
        table[i] = t.data_ptr()
    check(_lib.arch_fn(arch, "sfa_pack_weights_device")(ctypes.byref(arch), table, len(layout), packed.data_ptr(), stream),
          "sfa_pack_weights_device")


class KfpnEngine:
    """A device copy of the packed weights + an sfa_model handle + workspace cache.  ``arch`` is an
    SfaArch (fpn_resnet_18) or an SfaArchEx (either family: BACKBONE_DECONV is the plain resnet_18, which
    runs fp16x3 only and has no side streams)."""

    def __init__(self, arch, packed_host: np.ndarray, device, math=None, side_streams: bool = True):
        self._create(arch, torch.from_numpy(packed_host).to(torch.device(device)), device, math, side_streams)

    @classmethod
    def from_state(cls, arch, tensors, device, math=None) -> "KfpnEngine":
        """An engine from the state tensors where they live, without the host round trip: ``tensors`` is the
        state list in layout order (``_lib.state_layout(arch)``; contiguous float32 tensors on ``device``, the
        num_batches_tracked entries are skipped).  The packed buffer is allocated on the device and filled by
        sfa_pack_weights_device (the bytes of pack_state_dict); one wait, then sfa_model_create."""
        device = torch.device(device)
        eng = object.__new__(cls)
        n = int(_lib.arch_fn(arch, "sfa_packed_floats")(ctypes.byref(arch)))
        if n == 0:
            check(-1, "sfa_packed_floats")
        with torch.cuda.device(device):
            packed = torch.empty(n, dtype=torch.float32, device=device)
            _pack_on_device(arch, tensors, packed, _lib.stream_ptr(device))
            torch.cuda.current_stream(device).synchronize()
        eng._create(arch, packed, device, math, True)
        return eng

    def repack(self, tensors, stream: int = None) -> "KfpnEngine":
        """Pack the state ``tensors`` (layout order, as from_state) into ``self.weights`` in place and rebuild the
        derived weight images, on ``stream`` (default: the current one): stream-ordered and capturable.  The
        handle, its twins (they share the buffer and the images), the cached workspaces and graphs captured over
        this engine stay valid and read the new weights from then on."""
        st = _lib.stream_ptr(self.device) if stream is None else stream
        with torch.cuda.device(self.device):
            _pack_on_device(self.arch, tensors, self.weights, st)
        self.refresh_weight_images(st)
        return self

    def _create(self, arch, weights: torch.Tensor, device, math, side_streams):
        self.arch = arch
        self.deconv = _lib.is_ex(arch) and arch.backbone == _lib.BACKBONE_DECONV
        self.device = torch.device(device)
        self.heads = [(arch.head_names[j].value.decode(), int(arch.head_channels[j]))
                      for j in range(arch.num_heads)]
        self.weights = weights
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):  # the model's side stream lives on this device
            check(_lib.arch_fn(arch, "sfa_model_create")(ctypes.byref(arch), self.weights.data_ptr(), ctypes.byref(h)),
                  "sfa_model_create")
        self._h = h
        self._ws = {}
        self.side_streams = True
        self.set_math(_lib.math_from_env() if math is None else math)
        if not side_streams:
            self.set_side_streams(False)

    def set_math(self, math: int):
        """_lib.MATH_FP16X3 (default), _lib.MATH_BF16X6 or _lib.MATH_F32 for every convolution, or the opt-in
        reduced-precision _lib.MATH_FP16: one fp16 product per MAC in the residual layers' convolutions and the
        heads (stem and FPN stay fp16x3), logit error ~1e-3 instead of <= 1e-5 (include/sfa_hip.h)."""
        check(lib().sfa_model_set_math(self._h, int(math)), "sfa_model_set_math")
        self.math = int(math)

    def set_option(self, key: int, value: int):
        """Kernel-choice option of this handle (_lib.OPT_*, include/sfa_hip.h sfa_model_option):
        A/B runs and the kernel-equivalence tests; the defaults are the production kernels."""
        with torch.cuda.device(self.device):
            check(lib().sfa_model_set_option(self._h, int(key), int(value)), "sfa_model_set_option")

    def get_option(self, key: int) -> int:
        v = ctypes.c_int()
        check(lib().sfa_model_get_option(self._h, int(key), ctypes.byref(v)), "sfa_model_get_option")
        return int(v.value)

    def weight_image_bytes(self) -> int:
        """Device bytes of this handle's derived weight images (include/sfa_hip.h; shared with its twins), 0
        if it has none."""
        return int(lib().sfa_model_weight_image_bytes(self._h))

    def body_weight_image_bytes(self) -> int:
        """Device bytes of the derived weight images of the residual layers' strip convs (a second buffer,
        shared with the twins), 0 if the handle has none."""
        return int(lib().sfa_model_body_weight_image_bytes(self._h))

    def refresh_weight_images(self, stream: int = None):
        """Rebuild the derived weight images from ``self.weights`` on ``stream`` (default: the current one):
        after any in-place change of the packed device weights, before the next forward."""
        with torch.cuda.device(self.device):
            check(lib().sfa_model_refresh_weight_images(
                self._h, _lib.stream_ptr(self.device) if stream is None else stream),
                "sfa_model_refresh_weight_images")

    def set_side_streams(self, on: bool):
        """Side stream for the level-0 heads on (default) or off (sfa_model_set_side_streams):
        off when several forwards are kept in flight beside a copy stream, so the process's
        streams fit HIP's 4 hardware queues. Not while a forward of this engine is running."""
        with torch.cuda.device(self.device):
            check(lib().sfa_model_set_side_streams(self._h, 1 if on else 0), "sfa_model_set_side_streams")
        self.side_streams = bool(on)

    def twin(self) -> "KfpnEngine":
        """A second model handle over the SAME device weights and derived weight images
        (sfa_model_create_twin copies neither): its own side stream and events (or none, like this
        engine), so two forwards can be in flight (or captured in two graphs) on two streams.
        Workspaces are per engine / pipeline as usual."""
        t = object.__new__(KfpnEngine)
        t.arch, t.device, t.heads, t.weights = self.arch, self.device, self.heads, self.weights
        t.deconv = self.deconv
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().sfa_model_create_twin(self._h, ctypes.byref(h)), "sfa_model_create_twin")
        t._h = h
        t._ws = {}
        t.side_streams = True
        t.set_math(self.math)
        if not self.side_streams:
            t.set_side_streams(False)
        for key in _lib.OPTION_KEYS:  # the same kernel choices (every option key)
            if t.get_option(key) != self.get_option(key):
                t.set_option(key, self.get_option(key))
        return t

    def set_probe(self, flags: int):
        """Kernel probe (measurement only): _lib.PROBE_HEADS records timing events around each
        head-level launch of un-captured forwards; _lib.PROBE_SERIAL keeps every launch on the
        caller's stream. 0 turns it off."""
        check(lib().sfa_model_set_probe(self._h, int(flags)), "sfa_model_set_probe")

    def probe_times(self, levels: int = 3):
        """Durations (ms) of the head-level launches of the last probed forward (waits for them)."""
        ms = (ctypes.c_float * levels)()
        check(lib().sfa_model_probe_times(self._h, ms, levels), "sfa_model_probe_times")
        return [float(v) for v in ms]

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                lib().sfa_model_destroy(self._h)
        except Exception:
            pass

    def max_batch(self, H, W) -> int:
        """Frames one forward pass of this model holds (sfa_model_forward_max_batch); larger batches run
        in passes."""
        return int(lib().sfa_model_forward_max_batch(self._h, H, W))

    def workspace_bytes(self, B, H, W) -> int:
        return int(lib().sfa_forward_workspace_size(self._h, B, H, W))

    WORKSPACE_CACHE = 2  # streams whose forward workspace stays resident (LRU)

    def workspace(self, B, H, W, stream: int = None) -> torch.Tensor:
        """The forward workspace (activations + fp16x3 max slots) of forwards issued on
        ``stream`` without an explicit workspace.  Eager forwards on different streams get
        different buffers; the last ``WORKSPACE_CACHE`` streams keep theirs resident, and
        evicting or re-shaping an entry first waits for the device, so a forward still running
        on the old buffer never sees it reused.  Graph captures all issue on torch's capture
        stream, so graphs captured without an explicit workspace SHARE one buffer: two such
        graphs must not be replayed concurrently (DetectorPipeline owns its workspace instead)."""
        sk = int(stream) if stream is not None else _lib.stream_ptr(self.device)
        cur = self._ws.pop(sk, None)
        if cur is not None and cur[0] == (B, H, W):
            self._ws[sk] = cur  # most recently used last
            return cur[1]
        if cur is not None or len(self._ws) >= self.WORKSPACE_CACHE:
            torch.cuda.synchronize(self.device)
            del cur
            while len(self._ws) >= self.WORKSPACE_CACHE:
                self._ws.pop(next(iter(self._ws)))
        ws = torch.empty(self.workspace_bytes(B, H, W), dtype=torch.uint8, device=self.device)
        self._ws[sk] = ((B, H, W), ws)
        return ws

    def alloc_outputs(self, B, H, W):
        return {name: torch.empty((B, ch, H // 4, W // 4), dtype=torch.float32, device=self.device)
                for name, ch in self.heads}

    def forward_into(self, x: torch.Tensor, outs: dict, in_layout: int = _lib.IN_NCHW3,
                     workspace: torch.Tensor = None, stream: int = None) -> dict:
        if in_layout != _lib.IN_NHWC4:
            B, C, H, W = x.shape
            if C != 3:
                raise ValueError(f"expected (B, 3, H, W) input, got {tuple(x.shape)}")
        else:
            B, H, W, C = x.shape
            if C != 4:
                raise ValueError(f"expected (B, H, W, 4) input, got {tuple(x.shape)}")
        sp = stream if stream is not None else _lib.stream_ptr(self.device)
        ws = workspace if workspace is not None else self.workspace(B, H, W, sp)
        ptrs = (ctypes.c_void_p * len(self.heads))(*[outs[n].data_ptr() for n, _ in self.heads])
        check(lib().sfa_model_forward(self._h, x.data_ptr(), in_layout, B, H, W, ptrs, ws.data_ptr(),
                                      ws.numel(), sp), "sfa_model_forward")
        return outs

    def debug_views(self, ws: torch.Tensor, B, H, W) -> dict:
        """NCHW views of intermediate maps left in the workspace by the last forward (include/sfa_hip.h
        sfa_forward_buffer_offset says which reference tensor each one is).  A batch above
        sfa_forward_max_batch(H, W) runs in passes that share the workspace, so it has no such views:
        ValueError."""
        L = lib()
        bmax = self.max_batch(H, W)
        if B < 1 or B > bmax:
            raise ValueError(f"debug_views: batch {B} is outside 1..{bmax}, what one forward pass holds at "
                             f"{H}x{W}; the workspace keeps the maps of one pass only")

        def nhwc(which, h, w, c):
            off = int(L.sfa_forward_buffer_offset(self._h, B, H, W, which))
            t = ws[off: off + B * h * w * c * 4].view(torch.float32).view(B, h, w, c)
            return t.permute(0, 3, 1, 2)

        v = {f"layer{i + 1}": nhwc(i, H >> (i + 2), W >> (i + 2), 64 << i) for i in range(4)}
        if self.deconv:  # the three transposed-conv stage outputs (the last one is the heads' input)
            for i in range(3):
                v[f"deconv{i + 1}"] = nhwc(_lib.BUF_DECONV1 + i, H >> (4 - i), W >> (4 - i), 256)
            return v
        v["up_level2"] = nhwc(4, H // 8, W // 8, 256)
        v["up_level3"] = nhwc(5, H // 4, W // 4, 128)
        v["up_level4"] = nhwc(6, H // 4, W // 4, 64)
        nch = sum(c for _, c in self.heads)
        lv = []
        for k, (h, w) in enumerate(((H // 8, W // 8), (H // 4, W // 4), (H // 4, W // 4))):
            off = int(L.sfa_forward_buffer_offset(self._h, B, H, W, 7 + k))
            lv.append(ws[off: off + nch * B * h * w * 4].view(torch.float32).view(nch, B, h, w))
        levels, c0 = {}, 0
        for name, ch in self.heads:
            levels[name] = [t[c0:c0 + ch].permute(1, 0, 2, 3) for t in lv]
            c0 += ch
        v["levels"] = levels
        return v

    # ------------------------------------------------ head parameter gradients (sfa_model_heads_grad)
    def level_input(self, ws: torch.Tensor, B, H, W, level: int) -> torch.Tensor:
        """The NHWC (B, h, w, Cin) float32 view of the heads' input of KFPN ``level`` (SFA_BUF_UP_LEVEL2 / 3 / 4)
        that the last forward left in workspace ``ws``."""
        if self.deconv or level not in (0, 1, 2):
            raise ValueError(f"level_input: KFPN level {level!r} of a {'resnet_18' if self.deconv else 'KFPN'} model")
        if B < 1 or B > self.max_batch(H, W):
            raise ValueError(f"level_input: batch {B} is outside one forward pass at {H}x{W}")
        h, w, c = (H // 8, W // 8, 256) if level == 0 else (H // 4, W // 4, _lib.HEADS_LEVEL_CIN[level])
        off = int(lib().sfa_forward_buffer_offset(self._h, B, H, W, _lib.BUF_UP_LEVEL2 + level))
        return ws[off: off + B * h * w * c * 4].view(torch.float32).view(B, h, w, c)

    def heads_grad_chunk_pixels(self, level: int, B, h, w, max_chunk_pixels: int = 0) -> int:
        """K_c of :meth:`heads_param_grad`: the pixel count of its largest split-K chunk, the length of the
        float32 accumulation inside dW1 (0 for a shape the entry refuses)."""
        return int(lib().sfa_model_heads_grad_chunk_pixels(self._h, int(level), B, h, w, int(max_chunk_pixels)))

    def heads_grad_workspace_bytes(self, level: int, B, h, w, max_chunk_pixels: int = 0) -> int:
        return int(lib().sfa_model_heads_grad_workspace_size(self._h, int(level), B, h, w, int(max_chunk_pixels)))

    def heads_param_grad(self, level: int, x: torch.Tensor, grad_by_head: dict, out: dict = None,
                         want_hidden: bool = False, max_chunk_pixels: int = 0, workspace: torch.Tensor = None):
        """The parameter gradients of KFPN ``level``'s heads (sfa_model_heads_grad).  ``x``: the heads' input,
        float32 NHWC (B, h, w, Cin) on the GPU (Cin = 256 / 128 / 64; :meth:`level_input` after a forward, or any
        tensor); ``grad_by_head`` = {head: d total / d (the level's head output), (B, c, h, w)}, every head of the
        model.  Returns {head: (dW1 (64, Cin, 3, 3), db1 (64), dW2 (c, 64, 1, 1), db2 (c))}, every element written
        by the call; ``out`` (the same structure, contiguous tensors) receives them instead of fresh tensors.
        With ``want_hidden`` also returns Hd and dA, (B, h, w, 64 * heads) each, as the kernels used them.  The
        hidden activation is recomputed in fp16x3 whatever the engine's math mode is.  With ``out`` and
        ``workspace`` given the call only enqueues its launches (graph-capturable)."""
        x = _require_gpu_tensor(x, "heads_param_grad x")
        if x.dim() != 4 or level not in (0, 1, 2) or int(x.shape[3]) != _lib.HEADS_LEVEL_CIN[level]:
            raise ValueError(f"heads_param_grad: x {tuple(x.shape)} is not (B, h, w, Cin) of level {level!r}")
        B, h, w, cin = (int(v) for v in x.shape)
        names = [n for n, _ in self.heads]
        gs = []
        for n, c in self.heads:
            g = _require_gpu_tensor(grad_by_head[n], f"heads_param_grad grad[{n!r}]")
            if tuple(g.shape) != (B, c, h, w):
                raise ValueError(f"heads_param_grad grad[{n!r}]: {tuple(g.shape)} != {(B, c, h, w)}")
            gs.append(g)
        shapes = [((64, cin, 3, 3), (64,), (c, 64, 1, 1), (c,)) for _, c in self.heads]
        if out is None:
            res = [[torch.empty(s, dtype=torch.float32, device=x.device) for s in sh] for sh in shapes]
        else:
            res = [_kfpn_buffers(dict(enumerate(out[n])), range(4), sh, x, f"heads_param_grad out[{n!r}]")
                   for n, sh in zip(names, shapes)]
        hid = [torch.empty((B, h, w, 64 * len(names)), dtype=torch.float32, device=x.device) for _ in range(2)] \
            if want_hidden else None
        workspace = _workspace("heads_param_grad", f"B={B}, h={h}, w={w}, max_chunk_pixels={max_chunk_pixels}",
                               self.heads_grad_workspace_bytes(level, B, h, w, max_chunk_pixels), workspace, x.device)
        with torch.cuda.device(x.device):
            check(lib().sfa_model_heads_grad(self._h, level, x.data_ptr(), B, h, w, _ptr_array(gs),
                                             *(_ptr_array([r[k] for r in res]) for k in range(4)),
                                             *(_opt_ptr(t) for t in hid or (None, None)),
                                             int(max_chunk_pixels), workspace.data_ptr(), workspace.numel(),
                                             _lib.stream_ptr(x.device)), "sfa_model_heads_grad")
        grads = {n: tuple(r) for n, r in zip(names, res)}
        return (grads, hid[0], hid[1]) if want_hidden else grads

    # ------------------------------------------------ the heads as an operator (one level on a caller's x)
    def _level_nhwc(self, level, t, channels, what):
        t = _require_gpu_tensor(t, what)
        if self.deconv or level not in (0, 1, 2) or t.dim() != 4 or int(t.shape[3]) != channels(level):
            raise ValueError(f"{what}: {tuple(t.shape)} is not (B, h, w, {channels(level) if level in (0, 1, 2) else '?'})"
                             f" of KFPN level {level!r}")
        return t

    def heads_forward_workspace_bytes(self, level: int, B, h, w) -> int:
        return int(lib().sfa_model_heads_forward_workspace_size(self._h, int(level), B, h, w))

    def heads_forward(self, level: int, x: torch.Tensor, out: dict = None, want_hidden: bool = False,
                      workspace: torch.Tensor = None):
        """KFPN ``level``'s heads on a caller's ``x`` (sfa_model_heads_forward): float32 NHWC (B, h, w, Cin) on the
        GPU.  Returns {head: y (B, c, h, w)}; with ``want_hidden`` also Hd (B, h, w, 64 * heads), bit-equal to the
        Hd :meth:`heads_param_grad` recomputes for the same ``x``.  y is not promised bit-equal to the model's own
        fused forward (another kernel, another summation order).  With ``out`` ({head: contiguous tensor}) and
        ``workspace`` given the call only enqueues its launches (graph-capturable)."""
        x = self._level_nhwc(level, x, lambda f: _lib.HEADS_LEVEL_CIN[f], "heads_forward x")
        B, h, w, _ = (int(v) for v in x.shape)
        names = [n for n, _ in self.heads]
        ys = _kfpn_buffers(out, names, [(B, c, h, w) for _, c in self.heads], x, "heads_forward out")
        hid = torch.empty((B, h, w, 64 * len(names)), dtype=torch.float32, device=x.device) if want_hidden else None
        workspace = _workspace("heads_forward", f"B={B}, h={h}, w={w}",
                               self.heads_forward_workspace_bytes(level, B, h, w), workspace, x.device)
        with torch.cuda.device(x.device):
            check(lib().sfa_model_heads_forward(self._h, level, x.data_ptr(), B, h, w, _ptr_array(ys),
                                                _opt_ptr(hid), workspace.data_ptr(),
                                                workspace.numel(), _lib.stream_ptr(x.device)), "sfa_model_heads_forward")
        res = dict(zip(names, ys))
        return (res, hid) if want_hidden else res

    def heads_input_grad(self, level: int, dhidden: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """The gradient at the input of KFPN ``level``'s heads (sfa_model_heads_input_grad) from ``dhidden`` = dA,
        float32 (B, h, w, 64 * heads) on the GPU as :meth:`heads_param_grad` returns it with ``want_hidden``.
        Returns dX (B, h, w, Cin) NHWC, every element written; ``out`` (contiguous, that shape) receives it
        instead.  One launch on the current stream, no workspace (graph-capturable)."""
        d = self._level_nhwc(level, dhidden, lambda f: 64 * len(self.heads), "heads_input_grad dhidden")
        B, h, w, _ = (int(v) for v in d.shape)
        shape = (B, h, w, _lib.HEADS_LEVEL_CIN[level])
        gx = _kfpn_buffers(None if out is None else {0: out}, [0], [shape], d, "heads_input_grad out")[0]
        with torch.cuda.device(d.device):
            check(lib().sfa_model_heads_input_grad(self._h, level, d.data_ptr(), B, h, w, gx.data_ptr(),
                                                   _lib.stream_ptr(d.device)), "sfa_model_heads_input_grad")
        return gx

    # ------------------------------------------------ the FPN neck as an operator (four backbone maps in)
    def _neck_workspace(self, what, B, h4, w4, need, workspace, device):
        if self.deconv:
            raise ValueError(f"{what}: a resnet_18 model has no FPN neck")
        return _workspace(what, f"B={B}, h4={h4}, w4={w4}", need, workspace, device)

    @staticmethod
    def _neck_shapes(B, h4, w4):
        """NHWC shapes of l1..l4, then u2, u3, u4."""
        return ([(B, h4 << (3 - i), w4 << (3 - i), c) for i, c in enumerate(_lib.NECK_LAYER_C)]
                + [(B, 4 * h4, 4 * w4, 256), (B, 8 * h4, 8 * w4, 128), (B, 8 * h4, 8 * w4, 64)])

    def _neck_maps(self, what, maps, names, shapes, optional=False):
        out = []
        for t, n, s in zip(maps, names, shapes):
            if t is None and optional:
                out.append(None)
                continue
            t = _require_gpu_tensor(t, f"{what} {n}")
            if tuple(t.shape) != tuple(s):
                raise ValueError(f"{what} {n}: {tuple(t.shape)} is not the NHWC {tuple(s)}")
            out.append(t)
        return out

    def neck_forward_workspace_bytes(self, B, h4, w4) -> int:
        return 0 if self.deconv else int(lib().sfa_model_neck_forward_workspace_size(self._h, B, h4, w4))

    def neck_grad_workspace_bytes(self, B, h4, w4, max_chunk_pixels: int = 0) -> int:
        return 0 if self.deconv else int(lib().sfa_model_neck_grad_workspace_size(self._h, B, h4, w4, int(max_chunk_pixels)))

    def neck_grad_chunk_pixels(self, f: int, B, h4, w4, max_chunk_pixels: int = 0) -> int:
        """K_c of dW_f (f = 1, 2, 3) in :meth:`neck_grad`: the pixel count of its largest split-K chunk, the length
        of the float32 accumulation inside it (0 for a shape the entry refuses)."""
        return 0 if self.deconv else int(
            lib().sfa_model_neck_grad_chunk_pixels(self._h, int(f), B, h4, w4, int(max_chunk_pixels)))

    def neck_forward(self, l1, l2, l3, l4, out=None, workspace: torch.Tensor = None):
        """The FPN neck (models/fpn_resnet.py:197-210, sfa_model_neck_forward) on a caller's four backbone maps,
        float32 NHWC on the GPU: l4 (B, h4, w4, 512), l3 (B, 2 h4, 2 w4, 256), l2 (B, 4 h4, 4 w4, 128),
        l1 (B, 8 h4, 8 w4, 64).  Returns (u2, u3, u4) = up_level2 / 3 / 4, NHWC (B, 4 h4, 4 w4, 256),
        (B, 8 h4, 8 w4, 128), (B, 8 h4, 8 w4, 64); ``out`` (three contiguous tensors) receives them instead.  float32
        MFMA arithmetic: not promised bit-equal to the model's own fused fp16x3 FPN stage.  With ``out`` and
        ``workspace`` given the call only enqueues its launches (graph-capturable)."""
        l4 = _require_gpu_tensor(l4, "neck_forward l4")
        if l4.dim() != 4:
            raise ValueError(f"neck_forward l4: {tuple(l4.shape)} is not (B, h4, w4, 512)")
        B, h4, w4, _ = (int(v) for v in l4.shape)
        sh = self._neck_shapes(B, h4, w4)
        ls = self._neck_maps("neck_forward", (l1, l2, l3, l4), ("l1", "l2", "l3", "l4"), sh[:4])
        us = _kfpn_buffers(None if out is None else dict(enumerate(out)), range(3), sh[4:], l4, "neck_forward out")
        workspace = self._neck_workspace("neck_forward", B, h4, w4, self.neck_forward_workspace_bytes(B, h4, w4), workspace,
                                         l4.device)
        with torch.cuda.device(l4.device):
            check(lib().sfa_model_neck_forward(self._h, *(t.data_ptr() for t in ls), B, h4, w4,
                                               *(t.data_ptr() for t in us), workspace.data_ptr(), workspace.numel(),
                                               _lib.stream_ptr(l4.device)), "sfa_model_neck_forward")
        return tuple(us)

    def neck_grad(self, g2, g3, g4, layers=None, ups=None, want_layers=(True,) * 4, want_params=(True,) * 6, out=None,
                  max_chunk_pixels: int = 0, workspace: torch.Tensor = None):
        """The neck's gradients (sfa_model_neck_grad) from ``g2``, ``g3``, ``g4`` = d total / d u2, u3, u4 (NHWC,
        the shapes :meth:`neck_forward` returns; g2 and g3 may be None: zero).  ``layers`` = (l1, l2, l3, l4) and
        ``ups`` = (u2, u3) are what the weight gradients multiply (an entry may be None when no wanted dW reads
        it; both may be None when no dW is wanted).  Returns (d_layers, d_params): d_l1..d_l4 NHWC and dW1, db1, dW2,
        db2, dW3, db3 in torch's shapes, None where ``want_layers`` / ``want_params`` is False; every element of a
        wanted output is written.  ``out`` = (4 tensors or Nones, 6 tensors or Nones) receives them instead of
        fresh tensors.  With ``out`` and ``workspace`` given the call only enqueues its launches."""
        g4 = _require_gpu_tensor(g4, "neck_grad g4")
        if g4.dim() != 4 or g4.shape[1] % 8 or g4.shape[2] % 8:
            raise ValueError(f"neck_grad g4: {tuple(g4.shape)} is not (B, 8 h4, 8 w4, 64)")
        B, h4, w4 = int(g4.shape[0]), int(g4.shape[1]) // 8, int(g4.shape[2]) // 8
        sh = self._neck_shapes(B, h4, w4)
        gs = self._neck_maps("neck_grad", (g2, g3, g4), ("g2", "g3", "g4"), sh[4:], optional=True)
        ls = self._neck_maps("neck_grad", layers or (None,) * 4, ("l1", "l2", "l3", "l4"), sh[:4], optional=True)
        us = self._neck_maps("neck_grad", ups or (None,) * 2, ("u2", "u3"), sh[4:6], optional=True)
        want = list(want_layers) + list(want_params)
        shapes = sh[:4] + list(_lib.NECK_PARAM_SHAPES)
        res = _grad_outputs("neck_grad", want, shapes, out and (list(out[0]) + list(out[1])), g4)
        workspace = self._neck_workspace("neck_grad", B, h4, w4, self.neck_grad_workspace_bytes(B, h4, w4, max_chunk_pixels),
                                         workspace, g4.device)
        with torch.cuda.device(g4.device):
            check(lib().sfa_model_neck_grad(self._h, *(_opt_ptr(t) for t in ls + us + gs), B, h4, w4,
                                            *(_opt_ptr(t) for t in res[:4]), _dparams(res[4:]),
                                            int(max_chunk_pixels), workspace.data_ptr(), workspace.numel(),
                                            _lib.stream_ptr(g4.device)), "sfa_model_neck_grad")
        return res[:4], res[4:]

    # ------------------------------------------------ one BasicBlock as an operator (a caller's input in)
    @staticmethod
    def block_shape(layer: int, block: int):
        """(Cin, Cout, stride, has_downsample) of layer{layer}.{block}."""
        if layer not in (1, 2, 3, 4) or block not in (0, 1):
            raise ValueError(f"block: layer{layer!r}.{block!r} is outside layer1..4, block 0..1")
        cout = 64 << (layer - 1)
        ds = block == 0 and layer > 1
        return (cout // 2 if ds else cout), cout, (2 if ds else 1), ds

    def _block_dims(self, what, layer, block, x):
        if self.deconv:
            raise ValueError(f"{what}: the blocks of a resnet_18 model are not covered")
        cin, cout, s, ds = self.block_shape(layer, block)
        x = _require_gpu_tensor(x, f"{what} x")
        if x.dim() != 4 or int(x.shape[3]) != cin:
            raise ValueError(f"{what} x: {tuple(x.shape)} is not the NHWC (B, h, w, {cin}) of layer{layer}.{block}")
        B, h, w, _ = (int(v) for v in x.shape)
        return x, B, h, w, cin, cout, s, ds, (B, -(-h // s), -(-w // s), cout)

    def block_forward_workspace_bytes(self, layer, block, B, h, w) -> int:
        return 0 if self.deconv else int(lib().sfa_model_block_forward_workspace_size(self._h, layer, block, B, h, w))

    def block_grad_workspace_bytes(self, layer, block, B, h, w, max_chunk_pixels: int = 0) -> int:
        return 0 if self.deconv else int(
            lib().sfa_model_block_grad_workspace_size(self._h, layer, block, B, h, w, int(max_chunk_pixels)))

    def block_grad_chunk_pixels(self, layer, block, which: int, B, h, w, max_chunk_pixels: int = 0) -> int:
        """K_c of dW1' (which = 0), dW2' (1) or dWd' (2) in :meth:`block_grad`: the pixel count of its largest
        split-K chunk, the length of the float32 accumulation inside it (0 for what the entry refuses)."""
        return 0 if self.deconv else int(
            lib().sfa_model_block_grad_chunk_pixels(self._h, layer, block, int(which), B, h, w, int(max_chunk_pixels)))

    def block_forward(self, layer: int, block: int, x: torch.Tensor, out=None, workspace: torch.Tensor = None):
        """BasicBlock layer{layer}.{block} (sfa_model_block_forward) on a caller's ``x``, float32 NHWC (B, h, w, Cin)
        on the GPU, BatchNorm folded with the running statistics the engine was packed from.  Returns (mid, y),
        NHWC (B, ceil(h / s), ceil(w / s), Cout): the ReLU output of conv1 and the block's output; ``out`` (two
        contiguous tensors) receives them instead.  fp16x3 through the model's own convolution launches.  With ``out`` and ``workspace`` given the call only enqueues its
        launches (graph-capturable)."""
        x, B, h, w, _, _, _, _, osh = self._block_dims("block_forward", layer, block, x)
        mid, y = _kfpn_buffers(None if out is None else dict(enumerate(out)), range(2), [osh, osh], x, "block_forward out")
        workspace = _workspace("block_forward", f"B={B}, h={h}, w={w}",
                               self.block_forward_workspace_bytes(layer, block, B, h, w), workspace, x.device)
        with torch.cuda.device(x.device):
            check(lib().sfa_model_block_forward(self._h, layer, block, x.data_ptr(), B, h, w, mid.data_ptr(), y.data_ptr(),
                                                workspace.data_ptr(), workspace.numel(), _lib.stream_ptr(x.device)),
                  "sfa_model_block_forward")
        return mid, y

    def block_grad(self, layer: int, block: int, x, mid, y, gy, want_x: bool = True, want_params=(True,) * 5, out=None,
                   max_chunk_pixels: int = 0, workspace: torch.Tensor = None):
        """The gradients of layer{layer}.{block} (sfa_model_block_grad) from ``gy`` = d total / d y and the maps
        :meth:`block_forward` took and returned (float32 NHWC).  Returns (dx, [dW1', db1', dW2', db2', dWd']): the
        gradients at x and at the BN-folded parameters in torch's shapes, None where not wanted (dWd' is None on a
        block without a downsample whatever ``want_params[4]`` says); every element of a wanted output is written.
        ``out`` = (tensor or None, 5 tensors or Nones) receives them instead of fresh tensors.  With ``out`` and
        ``workspace`` given the call only enqueues its launches."""
        x, B, h, w, cin, cout, _, ds, osh = self._block_dims("block_grad", layer, block, x)
        maps = []
        for t, n in ((mid, "mid"), (y, "y"), (gy, "gy")):
            t = _require_gpu_tensor(t, f"block_grad {n}")
            if tuple(t.shape) != osh:
                raise ValueError(f"block_grad {n}: {tuple(t.shape)} is not the NHWC {osh}")
            maps.append(t)
        want = [bool(want_x)] + [bool(v) for v in want_params]
        want[5] = want[5] and ds
        shapes = [(B, h, w, cin), (cout, cin, 3, 3), (cout,), (cout, cout, 3, 3), (cout,), (cout, cin, 1, 1)]
        res = _grad_outputs("block_grad", want, shapes, out and ([out[0]] + list(out[1])), x)
        workspace = _workspace("block_grad", f"B={B}, h={h}, w={w}",
                               self.block_grad_workspace_bytes(layer, block, B, h, w, max_chunk_pixels), workspace, x.device)
        with torch.cuda.device(x.device):
            check(lib().sfa_model_block_grad(self._h, layer, block, x.data_ptr(), *(t.data_ptr() for t in maps), B, h, w,
                                             _opt_ptr(res[0]), _dparams(res[1:]), int(max_chunk_pixels),
                                             workspace.data_ptr(), workspace.numel(), _lib.stream_ptr(x.device)),
                  "sfa_model_block_grad")
        return res[0], res[1:]

    # ------------------------------------------------ the stem as an operator (a caller's image in)
    @staticmethod
    def stem_shapes(B, H, W):
        """NHWC shapes of a and pooled for a (B, 3, H, W) image."""
        oh, ow = -(-H // 2), -(-W // 2)
        return (B, oh, ow, 64), (B, -(-oh // 2), -(-ow // 2), 64)

    def _stem_dims(self, what, x):
        x = _require_gpu_tensor(x, f"{what} x")
        if x.dim() != 4 or int(x.shape[1]) != 3:
            raise ValueError(f"{what} x: {tuple(x.shape)} is not the NCHW (B, 3, H, W)")
        B, _, H, W = (int(v) for v in x.shape)
        return x, B, H, W

    def stem_forward_workspace_bytes(self, B, H, W) -> int:
        return int(lib().sfa_model_stem_forward_workspace_size(self._h, B, H, W))

    def stem_grad_workspace_bytes(self, B, H, W, max_chunk_pixels: int = 0) -> int:
        return int(lib().sfa_model_stem_grad_workspace_size(self._h, B, H, W, int(max_chunk_pixels)))

    def stem_grad_chunk_pixels(self, B, H, W, max_chunk_pixels: int = 0) -> int:
        """K_c of dW' in :meth:`stem_grad`: the pixel count of its largest split-K chunk, the length of the float32
        accumulation inside it (0 for what the entry refuses)."""
        return int(lib().sfa_model_stem_grad_chunk_pixels(self._h, B, H, W, int(max_chunk_pixels)))

    def stem_forward(self, x: torch.Tensor, out=None, workspace: torch.Tensor = None):
        """The stem (conv1 7x7 / 2, bn1 folded with the running statistics the engine was packed from, ReLU, max-pool;
        sfa_model_stem_forward) on a caller's ``x``, float32 NCHW (B, 3, H, W) on the GPU.  Returns (a, pooled), NHWC
        (B, ceil(H / 2), ceil(W / 2), 64) and (B, ceil(H / 4), ceil(W / 4), 64): the ReLU output and its 3x3 / 2
        max-pool; ``out`` (two contiguous tensors) receives them instead.  fp16x3 through the model's own unfused
        launches.  With ``out`` and ``workspace`` given the call only enqueues its launches (graph-capturable)."""
        x, B, H, W = self._stem_dims("stem_forward", x)
        a, pooled = _kfpn_buffers(None if out is None else dict(enumerate(out)), range(2), self.stem_shapes(B, H, W), x,
                                  "stem_forward out")
        workspace = _workspace("stem_forward", f"B={B}, H={H}, W={W}", self.stem_forward_workspace_bytes(B, H, W), workspace,
                               x.device)
        with torch.cuda.device(x.device):
            check(lib().sfa_model_stem_forward(self._h, x.data_ptr(), B, H, W, a.data_ptr(), pooled.data_ptr(),
                                               workspace.data_ptr(), workspace.numel(), _lib.stream_ptr(x.device)),
                  "sfa_model_stem_forward")
        return a, pooled

    def stem_grad(self, x, a, gp, want_x: bool = True, want_params=(True, True), out=None, max_chunk_pixels: int = 0,
                  workspace: torch.Tensor = None):
        """The stem's gradients (sfa_model_stem_grad) from ``gp`` = d total / d pooled (NHWC) and the ``x`` and ``a``
        :meth:`stem_forward` took and returned.  Returns (dx, [dW', db']): the gradient at the image (B, 3, H, W) and at
        the BN-folded parameters (64, 3, 7, 7), (64,), None where not wanted (dx is not computed then); every element
        of a wanted output is written.  ``out`` = (tensor or None, 2 tensors or Nones) receives them instead of fresh
        tensors.  With ``out`` and ``workspace`` given the call only enqueues its launches."""
        x, B, H, W = self._stem_dims("stem_grad", x)
        ash, psh = self.stem_shapes(B, H, W)
        maps = []
        for t, n, s in ((a, "a", ash), (gp, "gp", psh)):
            t = _require_gpu_tensor(t, f"stem_grad {n}")
            if tuple(t.shape) != s:
                raise ValueError(f"stem_grad {n}: {tuple(t.shape)} is not the NHWC {s}")
            maps.append(t)
        want = [bool(want_x)] + [bool(v) for v in want_params]
        shapes = [(B, 3, H, W), (64, 3, 7, 7), (64,)]
        res = _grad_outputs("stem_grad", want, shapes, out and ([out[0]] + list(out[1])), x)
        workspace = _workspace("stem_grad", f"B={B}, H={H}, W={W}", self.stem_grad_workspace_bytes(B, H, W, max_chunk_pixels),
                               workspace, x.device)
        with torch.cuda.device(x.device):
            check(lib().sfa_model_stem_grad(self._h, x.data_ptr(), *(t.data_ptr() for t in maps), B, H, W,
                                            _opt_ptr(res[0]), _dparams(res[1:]), int(max_chunk_pixels), workspace.data_ptr(),
                                            workspace.numel(), _lib.stream_ptr(x.device)), "sfa_model_stem_grad")
        return res[0], res[1:]

    def forward(self, x: torch.Tensor, in_layout: int = _lib.IN_NCHW3) -> dict:
        x = _require_gpu_tensor(x, "PoseResNet.forward")
        if in_layout != _lib.IN_NHWC4:
            B, _, H, W = x.shape
        else:
            B, H, W, _ = x.shape
        if H % 32 or W % 32:
            raise ValueError(f"input H, W must be multiples of 32, got {H}x{W}")
        with torch.cuda.device(self.device):
            outs = self.alloc_outputs(B, H, W)
            return self.forward_into(x, outs, in_layout)


# --------------------------------------------------------------------- BEV
class BevVoxelizer:
    """sfa_bev_voxelize with its (self-cleaning) scratch kept resident."""

    def __init__(self, device, max_batch: int = 16, force_atomic: bool = None, strip8: bool = None):
        """force_atomic: the global-atomic kernels instead of the binned ones (same bits; A/B),
        default from env SFA_BEV_ATOMIC read once here (flag SFA_BEV_FORCE_ATOMIC per call);
        strip8: the one-pass path with 8-row strips (round 3a; A/B), env SFA_BEV_STRIP8."""
        self.device = torch.device(device)
        if force_atomic is None:
            force_atomic = os.environ.get("SFA_BEV_ATOMIC", "0") not in ("", "0")
        if strip8 is None:
            strip8 = os.environ.get("SFA_BEV_STRIP8", "0") not in ("", "0")
        self.force_atomic = bool(force_atomic)
        self.strip8 = bool(strip8)
        self.max_batch = 0
        self.scratch = None
        self._grow(max_batch)

    def _grow(self, b):
        if b <= self.max_batch:
            return
        if b > _lib.SFA_BEV_MAX_BATCH:
            raise ValueError(f"BEV batch {b} > {_lib.SFA_BEV_MAX_BATCH}")
        self.scratch = torch.zeros(int(lib().sfa_bev_scratch_size(b)), dtype=torch.uint8,
                                   device=self.device)
        self.max_batch = b

    def __call__(self, points: torch.Tensor, offsets, boundary=DEFAULT_BOUNDARY,
                 layout: int = _lib.BEV_NHWC4_F32, flags: int = _lib.BEV_RAW, out=None,
                 stream: int = None) -> torch.Tensor:
        points = _require_gpu_tensor(points, "makeBEVMap")
        if points.ndim != 2 or points.shape[1] != 4:
            raise ValueError(f"points must be (N, 4), got {tuple(points.shape)}")
        offs = np.asarray(offsets, dtype=np.int64)
        B = offs.size - 1
        if B < 1 or offs[-1] > points.shape[0] or offs[0] < 0 or np.any(np.diff(offs) < 0):
            raise ValueError("bad frame offsets")
        self._grow(B)
        if out is None:
            if layout == _lib.BEV_NHWC4_F32:
                out = torch.empty((B, 608, 608, 4), dtype=torch.float32, device=self.device)
            else:
                dt = torch.float64 if layout == _lib.BEV_NCHW3_F64 else torch.float32
                out = torch.empty((B, 3, 608, 608), dtype=dt, device=self.device)
        offs_c = (ctypes.c_int64 * (B + 1))(*offs.tolist())
        if self.force_atomic:
            flags |= _lib.BEV_FORCE_ATOMIC
        if self.strip8:
            flags |= _lib.BEV_STRIP8
        check(lib().sfa_bev_voxelize(points.data_ptr() if points.numel() else None, offs_c, B,
                                     _boundary_arr(boundary), flags, layout, out.data_ptr(),
                                     self.scratch.data_ptr(), self.scratch.numel(),
                                     stream if stream is not None else _lib.stream_ptr(self.device)),
              "sfa_bev_voxelize")
        return out


_voxelizers = {}


def voxelizer(device) -> BevVoxelizer:
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    v = _voxelizers.get(device)
    if v is None:
        v = _voxelizers[device] = BevVoxelizer(device)
    return v


# argoverse_test2.py:37-47 (the scripts' boundary: +-40 m, 0.1 m cells -> 800 x 800)
ARGO_BOUNDARY = {"minX": -40, "maxX": 40, "minY": -40, "maxY": 40, "minZ": -3, "maxZ": 1}
ARGO_DISCRETIZATION = 0.1


def argo_bev_shape(boundary, discretization) -> tuple:
    """(H, W) of makeBVFeature's map (argoverse_test2.py:224-225), from the C side (host only)."""
    H, W = ctypes.c_int(), ctypes.c_int()
    check(lib().sfa_argo_bev_shape(_boundary_arr(boundary), float(discretization), ctypes.byref(H),
                                   ctypes.byref(W)), "sfa_argo_bev_shape")
    return H.value, W.value


class ArgoBevVoxelizer:
    """sfa_argo_bev_voxelize (argoverse_test2.py:198-257 makeBVFeature, bit-exact) for one boundary and
    discretization, with its (self-cleaning) scratch kept resident: a ragged batch of sweeps, packed
    back to back, into (B, 3, H, W) or the model's (B, H, W, 4)."""

    def __init__(self, device, boundary=ARGO_BOUNDARY, discretization: float = ARGO_DISCRETIZATION,
                 max_batch: int = 1, force_atomic: bool = False):
        """force_atomic: the global-atomic kernels instead of the record ones (same bits; A/B)."""
        self.device = torch.device(device)
        self.boundary = dict(boundary)
        self.discretization = float(discretization)
        self.H, self.W = argo_bev_shape(boundary, discretization)
        self.force_atomic = bool(force_atomic)
        self.max_batch = 0
        self.scratch = None
        self._grow(max_batch)

    def _grow(self, b):
        if b <= self.max_batch:
            return
        if b > _lib.SFA_BEV_MAX_BATCH:
            raise ValueError(f"BEV batch {b} > {_lib.SFA_BEV_MAX_BATCH}")
        self.scratch = torch.zeros(int(lib().sfa_argo_bev_scratch_size(b, self.H, self.W)), dtype=torch.uint8,
                                   device=self.device)
        self.max_batch = b

    def out_shape(self, B: int, layout: int) -> tuple:
        return (B, self.H, self.W, 4) if layout == _lib.BEV_NHWC4_F32 else (B, 3, self.H, self.W)

    def __call__(self, points: torch.Tensor, offsets, layout: int = _lib.BEV_NCHW3_F32, out=None,
                 stream: int = None, force_atomic: bool = None) -> torch.Tensor:
        """points: (N, 3) (intensity 0.5) or (N, >= 4) float32 GPU tensor; offsets: B + 1 frame starts in
        points.  ``out``: a contiguous float32 GPU tensor of out_shape(B, layout) to write into."""
        points = _require_gpu_tensor(points, "makeBVFeature")
        if points.ndim != 2 or points.shape[1] < 3:
            raise ValueError(f"Invalid point cloud shape: {tuple(points.shape)}")  # the reference's error (:207)
        if layout not in (_lib.BEV_NCHW3_F32, _lib.BEV_NHWC4_F32):
            raise ValueError("layout must be BEV_NCHW3_F32 or BEV_NHWC4_F32")
        offs = np.asarray(offsets, dtype=np.int64)
        B = offs.size - 1
        if B < 1 or offs[-1] > points.shape[0] or offs[0] < 0 or np.any(np.diff(offs) < 0):
            raise ValueError("bad frame offsets")
        self._grow(B)
        shape = self.out_shape(B, layout)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif (tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous()
              or out.device != points.device):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on {points.device}")
        offs_c = (ctypes.c_int64 * (B + 1))(*offs.tolist())
        if self.force_atomic if force_atomic is None else force_atomic:
            layout |= _lib.ARGO_BEV_FORCE_ATOMIC
        check(lib().sfa_argo_bev_voxelize(points.data_ptr() if points.numel() else None, points.shape[1], offs_c, B,
                                          _boundary_arr(self.boundary), self.discretization, layout,
                                          out.data_ptr(), self.scratch.data_ptr(), self.scratch.numel(),
                                          stream if stream is not None else _lib.stream_ptr(self.device)),
              "sfa_argo_bev_voxelize")
        return out


_argo_voxelizers = {}


def argo_voxelizer(device, boundary, discretization) -> ArgoBevVoxelizer:
    """The device's shared voxeliser for this boundary / discretization (the host drop-in's)."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, tuple(float(boundary[k]) for k in ("minX", "maxX", "minY", "maxY", "minZ", "maxZ")),
           float(discretization))
    v = _argo_voxelizers.get(key)
    if v is None:
        v = _argo_voxelizers[key] = ArgoBevVoxelizer(device, boundary, discretization)
    return v


def filter_points(points: torch.Tensor, boundary=DEFAULT_BOUNDARY) -> torch.Tensor:
    """get_filtered_lidar on the device: (N, 4) f32 -> (M, 4) f32 (order kept, z -= minZ)."""
    points = _require_gpu_tensor(points, "get_filtered_lidar")
    n = points.shape[0]
    out = torch.empty((max(n, 1), 4), dtype=torch.float32, device=points.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=points.device)
    scratch = torch.empty(int(lib().sfa_filter_scratch_size(n)), dtype=torch.uint8,
                          device=points.device)
    check(lib().sfa_filter_points(points.data_ptr() if n else None, n, _boundary_arr(boundary),
                                  out.data_ptr(), cnt.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                  _lib.stream_ptr(points.device)), "sfa_filter_points")
    m = int(cnt.item())
    return out[:m]


# ------------------------------------------------------------------ decode
def sigmoid_clamp_(x: torch.Tensor) -> torch.Tensor:
    """_sigmoid (utils/torch_utils.py:44-45) in place on a float32 GPU tensor; a non-contiguous
    one (the reference accepts any strided tensor) goes through a contiguous copy that is
    written back into it."""
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda" or x.dtype != torch.float32:
        raise SfaNativeError("_sigmoid: the HIP path needs a float32 GPU tensor")
    if x.numel() == 0:
        return x
    t = x if x.is_contiguous() else x.contiguous()
    check(lib().sfa_sigmoid_clamp_inplace(t.data_ptr(), t.numel(), _lib.stream_ptr(x.device)),
          "sfa_sigmoid_clamp_inplace")
    if t is not x:
        x.copy_(t)
    return x


def heat_nms(heat: torch.Tensor) -> torch.Tensor:
    """_nms (evaluation_utils.py:21-26, kernel 3): a new tensor heat * (max_pool3x3(heat) == heat)."""
    heat = _require_gpu_tensor(heat, "_nms")
    if heat.dim() < 2:
        raise ValueError("_nms: expected (..., H, W)")
    H, W = int(heat.shape[-2]), int(heat.shape[-1])
    out = torch.empty_like(heat)
    check(lib().sfa_heat_nms(heat.data_ptr() if heat.numel() else None, out.data_ptr() if out.numel() else None,
                             heat.numel() // max(1, H * W), H, W, _lib.stream_ptr(heat.device)), "sfa_heat_nms")
    return out


def topk(scores: torch.Tensor, K: int = 40, per_channel: bool = False):
    """_topk (evaluation_utils.py:47-62): (score (B,K) f32, inds (B,K) int64, clses (B,K) int32,
    ys (B,K) f32, xs (B,K) f32); per_channel = _topk_channel (:65-74): (scores, inds, ys, xs), each
    (B, C, K). Ties: lower flat index first, then lower class (torch leaves them unspecified)."""
    scores = _require_gpu_tensor(scores, "_topk")
    if scores.dim() != 4:
        raise ValueError(f"_topk: expected (B, C, H, W), got {tuple(scores.shape)}")
    B, C, H, W = (int(v) for v in scores.shape)
    K = int(K)
    if K > H * W:  # torch.topk: "selected index k out of range"
        raise RuntimeError(f"_topk: K = {K} exceeds the {H * W} elements of a class map")
    dev = scores.device
    shp = (B, C, K) if per_channel else (B, K)
    sc = torch.empty(shp, dtype=torch.float32, device=dev)
    ind = torch.empty(shp, dtype=torch.int64, device=dev)
    cls = None if per_channel else torch.empty(shp, dtype=torch.int32, device=dev)
    ys = torch.empty(shp, dtype=torch.float32, device=dev)
    xs = torch.empty(shp, dtype=torch.float32, device=dev)
    nws = int(lib().sfa_topk_workspace_size_hw(B, C, H, W, K)) or int(lib().sfa_topk_workspace_size(B, C, K))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    check(lib().sfa_topk(scores.data_ptr(), B, C, H, W, K, 1 if per_channel else 0, sc.data_ptr(), ind.data_ptr(),
                         cls.data_ptr() if cls is not None else None, ys.data_ptr(), xs.data_ptr(), ws.data_ptr(),
                         ws.numel(), _lib.stream_ptr(dev)), "sfa_topk")
    return (sc, ind, ys, xs) if per_channel else (sc, ind, cls, ys, xs)


def gather_feat(feat: torch.Tensor, ind: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """_gather_feat (evaluation_utils.py:29-37, mask None): feat (B, N, D), ind (B, K) int64 ->
    (B, K, D); transpose = _transpose_and_gather_feat (:40-44): feat (B, D, H, W) -> (B, K, D).
    4- or 8-byte elements (f32, int32, int64). Indices outside [0, N) raise, as torch.gather does."""
    if not isinstance(feat, torch.Tensor) or feat.device.type != "cuda":
        raise SfaNativeError("_gather_feat: the HIP path needs GPU tensors; there is no CPU fallback")
    if feat.element_size() not in (4, 8):
        raise TypeError(f"_gather_feat: {feat.dtype} elements are not 4 or 8 bytes")
    ind = _require_gpu_tensor(ind, "_gather_feat indices", torch.int64)
    feat = feat.contiguous()
    if transpose:
        if feat.dim() != 4:
            raise ValueError("_transpose_and_gather_feat: expected feat (B, C, H, W)")
        B, D, H, W = (int(v) for v in feat.shape)
        N, sn, sd = H * W, 1, H * W
    else:
        if feat.dim() != 3:
            raise ValueError("_gather_feat: expected feat (B, N, D)")
        B, N, D = (int(v) for v in feat.shape)
        sn, sd = D, 1
    if ind.dim() != 2 or int(ind.shape[0]) != B:
        raise ValueError(f"_gather_feat: indices {tuple(ind.shape)} do not match batch {B}")
    K = int(ind.shape[1])
    out = torch.empty((B, K, D), dtype=feat.dtype, device=feat.device)
    if ind.numel():
        lo, hi = (int(v) for v in torch.aminmax(ind))
        if lo < 0 or hi >= N:
            raise RuntimeError(f"_gather_feat: index {lo if lo < 0 else hi} is out of bounds for size {N}")
    check(lib().sfa_gather_feat(feat.data_ptr() if feat.numel() else None, B, N, D, sn, sd, feat.element_size(),
                                ind.data_ptr() if ind.numel() else None, K, out.data_ptr() if out.numel() else None,
                                _lib.stream_ptr(feat.device)), "sfa_gather_feat")
    return out


class Decoder:
    """sfa_decode with a workspace cached per (device, stream, shape): decodes on different
    streams never share scratch."""

    def __init__(self):
        self._ws = {}

    @staticmethod
    def workspace_bytes(B, C, K, H: int = None, W: int = None) -> int:
        """Bytes sfa_decode needs for (B, C, H, W) maps; without H, W the size that serves every map
        of H*W <= 36864 (the tiled form above that needs the map's own size)."""
        if H is not None and W is not None:
            n = int(lib().sfa_decode_workspace_size_hw(B, C, int(H), int(W), K))
            if n:  # 0: a shape sfa_decode refuses (it names the reason)
                return n
        return int(lib().sfa_decode_workspace_size(B, C, K))

    def workspace(self, device, B, C, K, stream: int = None, H: int = None, W: int = None):
        sk = int(stream) if stream is not None else _lib.stream_ptr(device)
        n = self.workspace_bytes(B, C, K, H, W)
        key = (str(device), sk, B, C, K, n)
        ws = self._ws.get(key)
        if ws is None:
            ws = torch.empty(n, dtype=torch.uint8, device=device)
            self._ws[key] = ws
        return ws

    def __call__(self, hm, off, dirn, z, dim, K=40, apply_sigmoid=False, out=None,
                 stream: int = None, workspace: torch.Tensor = None):
        hm = _require_gpu_tensor(hm, "decode")
        dirn, z, dim = (_require_gpu_tensor(t, "decode") for t in (dirn, z, dim))
        if off is not None:
            off = _require_gpu_tensor(off, "decode")
        B, C, H, W = (int(v) for v in hm.shape)
        for t, c in ((off, 2), (dirn, 2), (z, 1), (dim, 3)):
            if t is not None and tuple(t.shape) != (B, c, H, W):
                raise ValueError(f"decode: map shape {tuple(t.shape)} != {(B, c, H, W)}")
        if out is None:
            out = torch.empty((B, K, 10), dtype=torch.float32, device=hm.device)
        sp = stream if stream is not None else _lib.stream_ptr(hm.device)
        need = self.workspace_bytes(B, C, K, H, W)
        ws = workspace if workspace is not None else self.workspace(hm.device, B, C, K, sp, H, W)
        if ws.numel() < need:
            raise ValueError("decode: workspace too small")
        check(lib().sfa_decode(hm.data_ptr(), off.data_ptr() if off is not None else None,
                               dirn.data_ptr(), z.data_ptr(), dim.data_ptr(), B, C, H, W, int(K),
                               1 if apply_sigmoid else 0, out.data_ptr(), ws.data_ptr(), ws.numel(),
                               sp),
              "sfa_decode")
        return out


_decoder = Decoder()


def decode(hm, off, dirn, z, dim, K=40, apply_sigmoid=False):
    return _decoder(hm, off, dirn, z, dim, K=K, apply_sigmoid=apply_sigmoid)


# ---------------------------------------------------------------- pipeline
class DetectorPipeline:
    """Fixed-shape hot path on one GPU: [points ->] BEV -> KFPN forward -> decode.

    All buffers are allocated once; ``run()`` only enqueues kernels on the current
    stream, so it can be captured in a HIP graph (``capture()``).
    """

    def __init__(self, engine: KfpnEngine, batch: int, height: int = 608, width: int = 608,
                 K: int = 50, with_bev: bool = False, max_points: int = 0, two_sided: bool = False,
                 boundary=None, boundary_back=None, bev_layout: str = "nchw3", bev: str = "kitti",
                 discretization: float = None):
        """two_sided (with_bev only): every sweep is also voxelised with ``boundary_back``
        and flipped (demo_2_sides.py: demo_dataset.py:70-88 + demo_utils.py:110-111), so one
        run infers 2*batch maps: frames [0, batch) front, [batch, 2*batch) back.
        bev_layout (with_bev only): the voxeliser's output / the model's input — "nchw3" (the
        reference's (B, 3, 608, 608) f32, read by the patch stem directly: 3/4 of NHWC4's bytes)
        or "nhwc4" ((B, 608, 608, 4), channel 3 = 0).
        bev (with_bev only): "kitti" (default: get_filtered_lidar + makeBEVMap, 608 x 608) or
        "argoverse": the sweeps go through makeBVFeature (argoverse_test2.py:198-257,
        ArgoBevVoxelizer) with ``boundary`` (default ARGO_BOUNDARY) and ``discretization`` (default
        0.1) straight into the model's input; height x width must be that map's H x W; points may
        have 3 columns (intensity 0.5) or >= 4; not two_sided."""
        if bev not in ("kitti", "argoverse"):
            raise ValueError(f"bev must be 'kitti' or 'argoverse', not {bev!r}")
        self.bev_kind = bev
        if bev == "argoverse":
            if not with_bev or two_sided:
                raise ValueError("bev='argoverse' needs with_bev and has no back view (two_sided)")
            boundary = ARGO_BOUNDARY if boundary is None else boundary
            discretization = ARGO_DISCRETIZATION if discretization is None else discretization
        elif discretization is not None:
            raise ValueError("discretization belongs to bev='argoverse' (the KITTI grid is fixed)")
        if boundary is None:
            boundary = DEFAULT_BOUNDARY
        self.engine = engine
        self.dev = engine.device
        self.B, self.H, self.W, self.K = batch, height, width, K
        self.with_bev = with_bev
        self.two_sided = bool(two_sided)
        if self.two_sided and not with_bev:
            raise ValueError("two_sided needs with_bev (the back view is voxelised on the GPU)")
        self.boundary = boundary
        self.boundary_back = boundary_back if boundary_back is not None else DEFAULT_BOUNDARY_BACK
        nmap = 2 * batch if self.two_sided else batch
        self.nmap = nmap
        with torch.cuda.device(self.dev):
            # the pipeline's own workspace (it is replayed on streams of the caller's choosing,
            # so it must not be the engine's per-stream cache entry)
            self.ws = torch.empty(engine.workspace_bytes(nmap, height, width), dtype=torch.uint8,
                                  device=self.dev)
            self.outs = engine.alloc_outputs(nmap, height, width)
            self.dets = torch.empty((nmap, K, 10), dtype=torch.float32, device=self.dev)
            hm_h, hm_w = (int(v) for v in self.outs["hm_cen"].shape[2:])
            self.dec_ws = torch.empty(Decoder.workspace_bytes(nmap, dict(engine.heads)["hm_cen"], K, hm_h, hm_w),
                                      dtype=torch.uint8, device=self.dev)
            if with_bev:
                if bev == "argoverse":
                    self.vox = ArgoBevVoxelizer(self.dev, boundary, discretization, batch)
                    if (height, width) != (self.vox.H, self.vox.W):
                        raise ValueError(f"the boundary and discretization give a {self.vox.H}x{self.vox.W} map, "
                                         f"the pipeline was asked for {height}x{width}")
                else:
                    if (height, width) != (608, 608):
                        raise ValueError("the BEV grid is 608x608 (config/kitti_config.py:45-46)")
                    self.vox = BevVoxelizer(self.dev, batch)
                if bev_layout not in ("nchw3", "nhwc4"):
                    raise ValueError(f"bev_layout must be 'nchw3' or 'nhwc4', not {bev_layout!r}")
                self.bev_layout = bev_layout
                self.bev_fmt = _lib.BEV_NCHW3_F32 if bev_layout == "nchw3" else _lib.BEV_NHWC4_F32
                self.in_fmt = _lib.IN_NCHW3 if bev_layout == "nchw3" else _lib.IN_NHWC4
                shape = (nmap, 3, height, width) if bev_layout == "nchw3" else (nmap, height, width, 4)
                self.bev = torch.empty(shape, dtype=torch.float32, device=self.dev)
                self.points = torch.zeros((max(max_points, 1), 4), dtype=torch.float32,
                                          device=self.dev)
                self.offsets = np.zeros(batch + 1, np.int64)
            else:
                self.x = torch.empty((batch, 3, height, width), dtype=torch.float32, device=self.dev)
        self.graph = None
        self.infer_graph = None  # forward + decode only (capture_infer): the BEV stays eager

    def set_points(self, clouds):
        """Copy a list of (N_i, 4) float32 clouds into the resident point buffer."""
        offs = np.zeros(len(clouds) + 1, np.int64)
        for i, c in enumerate(clouds):
            offs[i + 1] = offs[i] + c.shape[0]
        if len(clouds) != self.B or offs[-1] > self.points.shape[0]:
            raise ValueError("clouds do not fit the pipeline's point buffer")
        host = torch.from_numpy(np.concatenate(clouds).astype(np.float32))
        if host.shape[1] != self.points.shape[1]:
            if self.bev_kind != "argoverse" or host.shape[1] < 3:
                raise ValueError(f"clouds must be (N, {self.points.shape[1]}), got (N, {host.shape[1]})")
            self.points = torch.zeros((self.points.shape[0], host.shape[1]), dtype=torch.float32, device=self.dev)
        self.points[: offs[-1]].copy_(host)
        self.offsets = offs

    def load_points(self, points: torch.Tensor, offsets):
        """Use a resident device buffer of points (e.g. a BinStream batch) without a copy;
        a short batch is padded with empty frames."""
        offs = np.asarray(offsets, dtype=np.int64)
        if offs.size - 1 > self.B:
            raise ValueError("more frames than the pipeline batch")
        self.points = _require_gpu_tensor(points, "load_points")
        self.offsets = np.concatenate([offs, np.full(self.B + 1 - offs.size, offs[-1], np.int64)])

    def run(self, bev_done=None, _eager=False):
        """Enqueue the step; ``bev_done`` (torch.cuda.Event) is recorded once the points have
        been consumed (after voxelisation).  With ``capture_infer()`` done, the forward + decode
        part replays that graph (``_eager`` forces the eager launches: capture() uses it)."""
        st = _lib.stream_ptr(self.dev)
        if self.with_bev:
            if self.bev_kind == "argoverse":
                self.vox(self.points, self.offsets, layout=self.bev_fmt, out=self.bev, stream=st)
            else:
                self.vox(self.points, self.offsets, boundary=self.boundary, layout=self.bev_fmt,
                         flags=_lib.BEV_RAW, out=self.bev[: self.B], stream=st)
            if self.two_sided:
                self.vox(self.points, self.offsets, boundary=self.boundary_back,
                         layout=self.bev_fmt, flags=_lib.BEV_RAW | _lib.BEV_FLIP_HW,
                         out=self.bev[self.B:], stream=st)
            if bev_done is not None:
                bev_done.record(torch.cuda.current_stream(self.dev))
        if self.infer_graph is not None and not _eager:
            self.infer_graph.replay()
            return self.dets
        return self._infer(st)

    def _infer(self, st):
        if self.with_bev:
            self.engine.forward_into(self.bev, self.outs, self.in_fmt, self.ws, st)
        else:
            self.engine.forward_into(self.x, self.outs, _lib.IN_NCHW3, self.ws, st)
        o = self.outs
        _decoder(o["hm_cen"], o["cen_offset"], o["direction"], o["z_coor"], o["dim"], K=self.K,
                 apply_sigmoid=True, out=self.dets, stream=st, workspace=self.dec_ws)
        return self.dets

    def capture(self):
        """Capture run() into a HIP graph (launch-overhead amortisation)."""
        with torch.cuda.device(self.dev):
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self.run(_eager=True)  # warm (module load, lazy init) outside capture
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.run(_eager=True)  # the kernels themselves, never a nested graph launch
            self.graph = g
        return g

    def capture_infer(self):
        """Capture the forward + decode (everything after the BEV) into a HIP graph that run()
        replays: the voxeliser's launches depend on the batch's host frame offsets (a new
        ragged batch per step when streaming), the rest of the step does not."""
        with torch.cuda.device(self.dev):
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._infer(_lib.stream_ptr(self.dev))  # warm outside capture
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._infer(_lib.stream_ptr(self.dev))
            self.infer_graph = g
        return g

    def replay(self):
        if self.graph is None:
            return self.run()
        self.graph.replay()
        return self.dets


# ------------------------------------------------------------------ fusion
def iou_matrix(boxes_a, boxes_b, device=None) -> torch.Tensor:
    """calculate_iou for every pair (test6.py:76-101): int [x, y, w, h] boxes -> (na, nb) f64."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    a = torch.as_tensor(np.asarray(boxes_a, np.int32).reshape(-1, 4)).to(dev)
    b = torch.as_tensor(np.asarray(boxes_b, np.int32).reshape(-1, 4)).to(dev)
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float64, device=dev)
    check(lib().sfa_iou_matrix(a.data_ptr() if a.numel() else None, a.shape[0],
                               b.data_ptr() if b.numel() else None, b.shape[0],
                               out.data_ptr() if out.numel() else None, _lib.stream_ptr(dev)),
          "sfa_iou_matrix")
    return out


def gaussian_nms_(boxes: torch.Tensor, conf: torch.Tensor, starts: torch.Tensor, counts: torch.Tensor,
                  sigma: float = 0.5, stream: int = None) -> torch.Tensor:
    """Gaussian soft-NMS in place on device arrays (README.md:250-261 gaussian_nms, batched):
    boxes int32 (N, 4) [x, y, w, h], conf f64 (N,), frame b = the counts[b] entries from
    starts[b] (int32 device tensors). Returns conf."""
    for t, name, dt in ((boxes, "boxes", torch.int32), (conf, "conf", torch.float64),
                        (starts, "starts", torch.int32), (counts, "counts", torch.int32)):
        _require_gpu_tensor(t, "gaussian_nms " + name, dt)
        if not t.is_contiguous():
            raise ValueError(f"gaussian_nms: {name} must be contiguous (updated in place)")
    if starts.numel() != counts.numel():
        raise ValueError("gaussian_nms: starts and counts differ in length")
    st = stream if stream is not None else _lib.stream_ptr(conf.device)
    check(lib().sfa_gaussian_nms(int(starts.numel()), boxes.data_ptr() if boxes.numel() else None,
                                 conf.data_ptr() if conf.numel() else None, starts.data_ptr(),
                                 counts.data_ptr(), float(sigma), st), "sfa_gaussian_nms")
    return conf


def gaussian_nms_frames(frames, sigma: float = 0.5, device=None):
    """[(boxes (n, 4) int, conf (n,) f64), ...] -> the decayed confidences per frame (host f64),
    all frames in one launch."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    counts = np.array([len(c) for _, c in frames], np.int32)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32) if len(frames) else np.zeros(0, np.int32)
    boxes = np.concatenate([np.asarray(b, np.int32).reshape(-1, 4) for b, _ in frames]) if len(frames) \
        else np.zeros((0, 4), np.int32)
    conf = np.concatenate([np.asarray(c, np.float64).reshape(-1) for _, c in frames]) if len(frames) \
        else np.zeros(0, np.float64)
    tb = torch.from_numpy(np.ascontiguousarray(boxes)).to(dev)
    tc = torch.from_numpy(np.ascontiguousarray(conf)).to(dev)
    gaussian_nms_(tb, tc, torch.from_numpy(starts).to(dev), torch.from_numpy(counts).to(dev), sigma)
    out = tc.cpu().numpy()
    return [out[s:s + n] for s, n in zip(starts, counts)]


class FusionResult:
    """Per-frame fused lists (reference order) and NMS survivors (host arrays)."""

    def __init__(self, boxes, conf, cls, src, origin, match, keep):
        self.boxes, self.conf, self.cls, self.src, self.keep = boxes, conf, cls, src, keep
        self.origin, self.match = origin, match


def fuse_frames(frames, conf_threshold=0.3, fusion_iou_threshold=0.7, nms_threshold=0.5,
                mode=_lib.FUSE_BAYES, apply_nms=True, device=None):
    """frames: list of (yolo_boxes (n,4) int, yolo_conf (n,) f64, yolo_cls (n,) int,
    sfa_boxes (m,4) int, sfa_conf (m,) f64).  Runs sfa_fuse_detections on the GPU."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    B = len(frames)
    if B == 0:
        return []
    yb, yc, yk, sb, sc = [], [], [], [], []
    yoff, soff = [0], [0]
    for f in frames:
        a, c, k, s, d = (np.asarray(v) for v in f)
        yb.append(a.astype(np.int32).reshape(-1, 4))
        yc.append(c.astype(np.float64).reshape(-1))
        yk.append(k.astype(np.int32).reshape(-1))
        sb.append(s.astype(np.int32).reshape(-1, 4))
        sc.append(d.astype(np.float64).reshape(-1))
        if yb[-1].shape[0] > 512 or sb[-1].shape[0] > 512:
            raise ValueError("fusion: at most 512 boxes per side per frame")
        yoff.append(yoff[-1] + yb[-1].shape[0])
        soff.append(soff[-1] + sb[-1].shape[0])
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(x) if x else x, dt)).to(dev)
    Y, YC, YK = t(yb, np.int32), t(yc, np.float64), t(yk, np.int32)
    S, SC = t(sb, np.int32), t(sc, np.float64)
    YO = torch.tensor(yoff, dtype=torch.int32, device=dev)
    SO = torch.tensor(soff, dtype=torch.int32, device=dev)
    cap = max(1, yoff[-1] + soff[-1])
    ob = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
    oc = torch.zeros(cap, dtype=torch.float64, device=dev)
    ok = torch.zeros(cap, dtype=torch.int32, device=dev)
    osrc = torch.zeros(cap, dtype=torch.int32, device=dev)
    oorig = torch.zeros(cap, dtype=torch.int32, device=dev)
    omatch = torch.zeros(cap, dtype=torch.int32, device=dev)
    ocount = torch.zeros(B, dtype=torch.int32, device=dev)
    okeep = torch.zeros(cap, dtype=torch.int32, device=dev)
    okc = torch.zeros(B, dtype=torch.int32, device=dev)
    prm = _lib.SfaFusionParams(float(conf_threshold), float(fusion_iou_threshold),
                               float(nms_threshold), int(mode), 1 if apply_nms else 0)
    ptr = lambda x: x.data_ptr() if x.numel() else None
    check(lib().sfa_fuse_detections(B, ptr(Y), ptr(YC), ptr(YK), YO.data_ptr(), ptr(S), ptr(SC),
                                    SO.data_ptr(), ctypes.byref(prm), ob.data_ptr(), oc.data_ptr(),
                                    ok.data_ptr(), osrc.data_ptr(), oorig.data_ptr(),
                                    omatch.data_ptr(), ocount.data_ptr(),
                                    okeep.data_ptr(), okc.data_ptr(), _lib.stream_ptr(dev)),
          "sfa_fuse_detections")
    ob, oc, ok, osrc = ob.cpu().numpy(), oc.cpu().numpy(), ok.cpu().numpy(), osrc.cpu().numpy()
    oorig, omatch = oorig.cpu().numpy(), omatch.cpu().numpy()
    ocount, okeep, okc = ocount.cpu().numpy(), okeep.cpu().numpy(), okc.cpu().numpy()
    out = []
    for b in range(B):
        base, n = yoff[b] + soff[b], int(ocount[b])
        sl = slice(base, base + n)
        keep = okeep[base: base + int(okc[b])].copy() if apply_nms else None
        if n < 0:
            raise ValueError(f"fusion: frame {b} exceeds 512 boxes per side")
        out.append(FusionResult(ob[sl].copy(), oc[sl].copy(), ok[sl].copy(), osrc[sl].copy(),
                                oorig[sl].copy(), omatch[sl].copy(), keep))
    return out


# ------------------------------------------------- post-processing on device
def make_calib(V2C, R0, P2, img_shape) -> "_lib.SfaCalib":
    """One frame's calibration (kitti_data_utils.py:127-139 Calibration fields: V2C 3x4,
    R0 3x3, P2 3x4 — f32 in the reference, widened exactly) + image shape (rows, cols)."""
    c = _lib.SfaCalib()
    c.V2C[:] = [float(v) for v in np.asarray(V2C, np.float64).reshape(-1)[:12]]
    c.R0[:] = [float(v) for v in np.asarray(R0, np.float64)[:3, :3].reshape(-1)]
    c.P2[:] = [float(v) for v in np.asarray(P2, np.float64).reshape(-1)[:12]]
    c.img_h, c.img_w = int(img_shape[0]), int(img_shape[1])
    return c


def calib_tensor(calibs, device) -> torch.Tensor:
    """list of SfaCalib -> device bytes (the C struct array)."""
    arr = (_lib.SfaCalib * len(calibs))(*calibs)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device)


def post_params(num_classes=3, down_ratio=4, peak_thresh=0.2, arith=_lib.REAL_F32,
                boundary=DEFAULT_BOUNDARY, bev_hw=(608, 608)) -> "_lib.SfaPostParams":
    p = _lib.SfaPostParams()
    p.num_classes, p.down_ratio, p.peak_thresh = int(num_classes), int(down_ratio), float(peak_thresh)
    p.bev_h, p.bev_w = int(bev_hw[0]), int(bev_hw[1])
    p.bound_x = float(boundary["maxX"] - boundary["minX"])
    p.bound_y = float(boundary["maxY"] - boundary["minY"])
    p.min_x, p.min_y, p.min_z = (float(boundary[k]) for k in ("minX", "minY", "minZ"))
    p.arith = int(arith)
    return p


def post_process(dets: torch.Tensor, num_classes=3, down_ratio=4, peak_thresh=0.2,
                 arith=_lib.REAL_F32, boundary=DEFAULT_BOUNDARY, bev_hw=(608, 608), out=None):
    """post_processing (evaluation_utils.py:112-163, every frame) + convert_det_to_real_values
    (:177-193) on the GPU.  dets (B, K, 10) f32 -> (preds (B*K, 8) f32, real (B*K, 8) f64,
    offsets (B+1,) int32), all device tensors; frame b owns rows offsets[b]:offsets[b+1]."""
    dets = _require_gpu_tensor(dets, "post_process")
    B, K = int(dets.shape[0]), int(dets.shape[1])
    if dets.dim() != 3 or dets.shape[2] != 10:
        raise ValueError("post_process: dets must be (B, K, 10)")
    dev = dets.device
    if out is None:
        out = (torch.empty((max(1, B * K), 8), dtype=torch.float32, device=dev),
               torch.empty((max(1, B * K), 8), dtype=torch.float64, device=dev),
               torch.empty(B + 1, dtype=torch.int32, device=dev))
    preds, real, off = out
    prm = post_params(num_classes, down_ratio, peak_thresh, arith, boundary, bev_hw)
    check(lib().sfa_post_process(dets.data_ptr(), B, K, ctypes.byref(prm), preds.data_ptr(),
                                 real.data_ptr(), off.data_ptr(), _lib.stream_ptr(dev)),
          "sfa_post_process")
    return preds, real, off


def project_boxes(real: torch.Tensor, offsets: torch.Tensor, calibs, preds=None, conf_min=0.3,
                  conf_source=_lib.CONF_CLASS_ID, extents=False, out=None):
    """convert_sfa3d_to_2d_boxes (test6.py:129-187) on the GPU for every frame.
    calibs: a device tensor from calib_tensor() or a list of SfaCalib (one per frame, or
    one for all).  Returns (boxes (cap, 4) int32, conf f64, row int32, extent f64 or None,
    offsets (B+1,) int32) device tensors (cap = number of real rows)."""
    real = _require_gpu_tensor(real, "project_boxes", torch.float64)
    offsets = _require_gpu_tensor(offsets, "project_boxes offsets", torch.int32)
    dev = real.device
    B = int(offsets.numel()) - 1
    if real.shape[0] == 0:  # no rows: the offsets are all 0, nothing is read
        real = torch.zeros((1, 8), dtype=torch.float64, device=dev)
    if isinstance(calibs, torch.Tensor):
        ct = calibs
        n_cal = ct.numel() // ctypes.sizeof(_lib.SfaCalib)
    else:
        calibs = list(calibs)
        ct, n_cal = calib_tensor(calibs, dev), len(calibs)
    if n_cal not in (1, B) or n_cal == 0:
        raise ValueError("project_boxes: need one calibration or one per frame")
    if conf_source == _lib.CONF_SCORE:
        preds = _require_gpu_tensor(preds, "project_boxes preds")
    cap = max(1, real.shape[0])
    if out is None:
        out = (torch.empty((cap, 4), dtype=torch.int32, device=dev),
               torch.empty(cap, dtype=torch.float64, device=dev),
               torch.empty(cap, dtype=torch.int32, device=dev),
               torch.empty((cap, 4), dtype=torch.float64, device=dev) if extents else None,
               torch.empty(B + 1, dtype=torch.int32, device=dev))
    boxes, conf, row, ext, off = out
    prm = _lib.SfaProjectParams(float(conf_min), int(conf_source), 1 if n_cal == B and B > 1 else 0)
    check(lib().sfa_project_boxes(real.data_ptr(), preds.data_ptr() if preds is not None else None,
                                  offsets.data_ptr(), B, ct.data_ptr(), ctypes.byref(prm),
                                  boxes.data_ptr(), conf.data_ptr(), row.data_ptr(),
                                  ext.data_ptr() if ext is not None else None, off.data_ptr(),
                                  _lib.stream_ptr(dev)),
          "sfa_project_boxes")
    return boxes, conf, row, ext, off


class ArgoBoxProjector:
    """sfa_argo_project_boxes for one log: the device rows of post_process (preds, offsets) -> the
    eight image corners of every detection (argoverse_test2.py:432-436 grid -> metres, :355-402
    create_3d_bbox_corners, :324-353 project_to_image) and the scripts' draw flag (:458), no host hop.
    ``calib``: an object with ``T_l2c`` (4x4) and ``P2`` (3x4), e.g.
    utils.argoverse_box_utils.ArgoverseCalibration; their float32 values are widened exactly."""

    def __init__(self, device, calib, boundary=ARGO_BOUNDARY, discretization: float = ARGO_DISCRETIZATION):
        self.device = torch.device(device)
        self.T = (ctypes.c_double * 16)(*np.asarray(calib.T_l2c, np.float64).reshape(16).tolist())
        self.P = (ctypes.c_double * 12)(*np.asarray(calib.P2, np.float64).reshape(12).tolist())
        self.boundary = _boundary_arr(boundary)
        self.discretization = float(discretization)

    def __call__(self, preds: torch.Tensor, offsets: torch.Tensor = None, corners3d: bool = False, out=None,
                 stream: int = None):
        """preds (n, 8) f32 [score, x, y, z, h, w, l, yaw]; offsets: post_process' (B + 1,) int32 (rows
        past offsets[B] are left as they are) or None (every row).  Returns (pixels (n, 8, 2) f32 with
        NaN for corners at camera Z <= 0.1, all8 (n,) int32, corners (n, 8, 3) f32 or None)."""
        preds = _require_gpu_tensor(preds, "argo_project_boxes")
        if preds.dim() != 2 or preds.shape[1] != 8:
            raise ValueError("argo_project_boxes: preds must be (n, 8)")
        n, dev = int(preds.shape[0]), preds.device
        B = 0
        if offsets is not None:
            offsets = _require_gpu_tensor(offsets, "argo_project_boxes offsets", torch.int32)
            B = int(offsets.numel()) - 1
        if out is None:
            out = (torch.full((n, 8, 2), float("nan"), dtype=torch.float32, device=dev),
                   torch.zeros(n, dtype=torch.int32, device=dev),
                   torch.zeros((n, 8, 3), dtype=torch.float32, device=dev) if corners3d else None)
        px, all8, c3 = out
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        check(lib().sfa_argo_project_boxes(ptr(preds), ptr(offsets), B, n, self.boundary, self.discretization,
                                           self.T, self.P, ptr(px), ptr(all8), ptr(c3),
                                           stream if stream is not None else _lib.stream_ptr(dev)),
              "sfa_argo_project_boxes")
        return px, all8, c3

    def project_points(self, points: torch.Tensor) -> torch.Tensor:
        """project_to_image (:324-353): (n, 3) f32 or f64 GPU points -> (n, 2) f32 pixels (NaN rows
        for points at camera Z <= 0.1)."""
        if not isinstance(points, torch.Tensor) or points.dtype not in (torch.float32, torch.float64):
            raise TypeError("project_to_image: expected a float32 or float64 tensor")
        points = _require_gpu_tensor(points, "project_to_image", points.dtype)
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"project_to_image: points must be (n, 3), got {tuple(points.shape)}")
        n = int(points.shape[0])
        out = torch.empty((n, 2), dtype=torch.float32, device=points.device)
        check(lib().sfa_argo_project_points(points.data_ptr() if n else None, 1 if points.dtype == torch.float64 else 0,
                                            n, self.T, self.P, out.data_ptr() if n else None,
                                            _lib.stream_ptr(points.device)), "sfa_argo_project_points")
        return out


# ------------------------------------------------------- fused LiDAR + camera
class FusionPipeline:
    """BASELINE config #5 on one GPU (test6.py's per-frame flow, batched): sweeps -> BEV ->
    KFPN forward -> decode (DetectorPipeline) -> post_process + convert_det_to_real_values
    (sfa_post_process) -> camera boxes (sfa_project_boxes) -> association, fusion and NMS
    with the camera detector's boxes (sfa_fuse_detections).  Every stage is a HIP kernel on
    device-resident CSR buffers, so run() is one HIP-graph-capturable sequence.

    The camera branch (YOLOv8n, ultralytics) is not part of this framework: its per-frame
    boxes are inputs (``set_camera``), as test6.py:189-209 hands them to the fusion.

    ``nms="gaussian"``: the fused lists get the README's Gaussian soft-NMS (README.md:250-261,
    sfa_gaussian_nms: confidences decayed in place, ``fconf``) instead of the greedy NMS of
    test6.py:104-126 (``fkeep`` then stays unused)."""

    def __init__(self, engine: KfpnEngine, batch: int, calibs, K: int = 50, max_points: int = 0,
                 max_camera_boxes: int = 512, conf_threshold=0.3, fusion_iou_threshold=0.7,
                 nms_threshold=0.5, mode=_lib.FUSE_BAYES, conf_source=_lib.CONF_CLASS_ID,
                 nms: str = "greedy", soft_nms_sigma: float = 0.5):
        self.det = DetectorPipeline(engine, batch, K=K, with_bev=True, max_points=max_points)
        self.B, self.K, self.dev = batch, K, engine.device
        dev = self.dev
        calibs = list(calibs)
        self.calib = calib_tensor(calibs, dev)
        self.conf_source = conf_source
        if nms not in ("greedy", "gaussian"):
            raise ValueError(f"nms must be 'greedy' or 'gaussian', got {nms!r}")
        self.nms, self.soft_nms_sigma = nms, float(soft_nms_sigma)
        self.params = _lib.SfaFusionParams(float(conf_threshold), float(fusion_iou_threshold),
                                           float(nms_threshold), int(mode), 1 if nms == "greedy" else 0)
        self.proj_params = _lib.SfaProjectParams(0.3, int(conf_source),
                                                 1 if len(calibs) == batch and batch > 1 else 0)
        self.post_prm = post_params()
        n = batch * K
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        with torch.cuda.device(dev):
            self.preds = torch.empty((n, 8), dtype=f32, device=dev)
            self.real = torch.empty((n, 8), dtype=f64, device=dev)
            self.real_off = torch.zeros(batch + 1, dtype=i32, device=dev)
            self.sboxes = torch.empty((n, 4), dtype=i32, device=dev)
            self.sconf = torch.empty(n, dtype=f64, device=dev)
            self.srow = torch.empty(n, dtype=i32, device=dev)
            self.soff = torch.zeros(batch + 1, dtype=i32, device=dev)
            cy = batch * max_camera_boxes
            self.ybox = torch.zeros((cy, 4), dtype=i32, device=dev)
            self.yconf = torch.zeros(cy, dtype=f64, device=dev)
            self.ycls = torch.zeros(cy, dtype=i32, device=dev)
            self.yoff = torch.zeros(batch + 1, dtype=i32, device=dev)
            cap = cy + n
            self.fbox = torch.empty((cap, 4), dtype=i32, device=dev)
            self.fconf = torch.empty(cap, dtype=f64, device=dev)
            self.fcls = torch.empty(cap, dtype=i32, device=dev)
            self.fsrc = torch.empty(cap, dtype=i32, device=dev)
            self.fcount = torch.empty(batch, dtype=i32, device=dev)
            self.fkeep = torch.empty(cap, dtype=i32, device=dev)
            self.fkeep_count = torch.empty(batch, dtype=i32, device=dev)
            self.fstart = torch.zeros(batch, dtype=i32, device=dev)  # frame b's fused list start
        self.max_camera_boxes = max_camera_boxes
        self.graph = None

    def set_points(self, clouds):
        self.det.set_points(clouds)

    def set_camera(self, frames):
        """frames: per frame (boxes (n, 4) int [x, y, w, h], conf (n,), class ids (n,))."""
        if len(frames) != self.B:
            raise ValueError("one camera detection list per frame")
        b, c, k, off = [], [], [], [0]
        for boxes, conf, cls in frames:
            boxes = np.asarray(boxes, np.int32).reshape(-1, 4)
            if boxes.shape[0] > min(512, self.max_camera_boxes):
                raise ValueError("at most 512 camera boxes per frame")
            b.append(boxes)
            c.append(np.asarray(conf, np.float64).reshape(-1))
            k.append(np.asarray(cls, np.int32).reshape(-1))
            off.append(off[-1] + boxes.shape[0])
        n = off[-1]
        if n:
            self.ybox[:n].copy_(torch.from_numpy(np.concatenate(b)))
            self.yconf[:n].copy_(torch.from_numpy(np.concatenate(c)))
            self.ycls[:n].copy_(torch.from_numpy(np.concatenate(k)))
        self.yoff.copy_(torch.tensor(off, dtype=torch.int32))

    def run(self):
        st = _lib.stream_ptr(self.dev)
        L = lib()
        dets = self.det.run()
        check(L.sfa_post_process(dets.data_ptr(), self.B, self.K, ctypes.byref(self.post_prm),
                                 self.preds.data_ptr(), self.real.data_ptr(),
                                 self.real_off.data_ptr(), st), "sfa_post_process")
        check(L.sfa_project_boxes(self.real.data_ptr(), self.preds.data_ptr(),
                                  self.real_off.data_ptr(), self.B, self.calib.data_ptr(),
                                  ctypes.byref(self.proj_params), self.sboxes.data_ptr(),
                                  self.sconf.data_ptr(), self.srow.data_ptr(), None,
                                  self.soff.data_ptr(), st), "sfa_project_boxes")
        check(L.sfa_fuse_detections(self.B, self.ybox.data_ptr(), self.yconf.data_ptr(),
                                    self.ycls.data_ptr(), self.yoff.data_ptr(),
                                    self.sboxes.data_ptr(), self.sconf.data_ptr(),
                                    self.soff.data_ptr(), ctypes.byref(self.params),
                                    self.fbox.data_ptr(), self.fconf.data_ptr(),
                                    self.fcls.data_ptr(), self.fsrc.data_ptr(), None, None,
                                    self.fcount.data_ptr(), self.fkeep.data_ptr(),
                                    self.fkeep_count.data_ptr(), st), "sfa_fuse_detections")
        if self.nms == "gaussian":
            torch.add(self.yoff[:-1], self.soff[:-1], out=self.fstart)  # on the current stream (= st)
            check(L.sfa_gaussian_nms(self.B, self.fbox.data_ptr(), self.fconf.data_ptr(), self.fstart.data_ptr(),
                                     self.fcount.data_ptr(), self.soft_nms_sigma, st), "sfa_gaussian_nms")
        return self.fcount

    def capture(self):
        with torch.cuda.device(self.dev):
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self.run()
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.run()
            self.graph = g
        return g

    def replay(self):
        if self.graph is None:
            return self.run()
        self.graph.replay()
        return self.fcount

    def results(self):
        """Host copy per frame: (fused boxes, conf, cls, source, NMS keep indices); with
        nms="gaussian" conf is the decayed confidence and keep is every index (nothing dropped)."""
        yoff = self.yoff.cpu().numpy()
        soff = self.soff.cpu().numpy()
        cnt, kc = self.fcount.cpu().numpy(), self.fkeep_count.cpu().numpy()
        fb, fc, fk, fs, keep = (t.cpu().numpy() for t in (self.fbox, self.fconf, self.fcls,
                                                          self.fsrc, self.fkeep))
        out = []
        for b in range(self.B):
            base = yoff[b] + soff[b]
            n = int(cnt[b])
            kp = np.arange(max(n, 0), dtype=keep.dtype) if self.nms == "gaussian" else keep[base:base + int(kc[b])]
            out.append((fb[base:base + n], fc[base:base + n], fk[base:base + n], fs[base:base + n], kp))
        return out


# ------------------------------------------------------- validation: targets + loss
TARGET_KEYS = ("hm_cen", "cen_offset", "direction", "z_coor", "dim", "indices_center", "obj_mask")
LOSS_KEYS = ("total_loss", "hm_cen_loss", "cen_offset_loss", "dim_loss", "direction_loss", "z_coor_loss")


class TargetBuilder:
    """KittiDataset.build_targets (kitti_dataset.py:157-244) for a batch of label lists on the device
    (sfa_build_targets).  ``labels``: (N, 8) float32 rows [cls, x, y, z, h, w, l, yaw] of all frames, in
    label order; ``offsets``: B + 1 row offsets (a sequence, or an int64 GPU tensor); ``hflipped``: one
    bool per frame.  Returns the reference's dict of GPU tensors, batched as its collate stacks them.
    ``status`` (uint32 per frame, bit 0: a centre outside the map, bit 1: a class id the reference
    raises on) is kept on the builder; with ``verify`` (the default) bit 1 raises IndexError, which
    synchronises.  With ``out`` (a dict from :meth:`alloc`), ``verify=False`` and device offsets the call
    only enqueues one launch and can be captured into a HIP graph."""

    def __init__(self, device, boundary=DEFAULT_BOUNDARY, hm_size=(152, 152), num_classes: int = 3,
                 max_objects: int = 50):
        self.dev = torch.device(device)
        self.boundary = dict(boundary)
        self.hm_size = (int(hm_size[0]), int(hm_size[1]))
        self.num_classes, self.max_objects = int(num_classes), int(max_objects)
        self.status = None

    def alloc(self, B: int) -> dict:
        (H, W), C, M, dev = self.hm_size, self.num_classes, self.max_objects, self.dev
        f32 = torch.float32
        return {"hm_cen": torch.empty((B, C, H, W), dtype=f32, device=dev),
                "cen_offset": torch.empty((B, M, 2), dtype=f32, device=dev),
                "direction": torch.empty((B, M, 2), dtype=f32, device=dev),
                "z_coor": torch.empty((B, M, 1), dtype=f32, device=dev),
                "dim": torch.empty((B, M, 3), dtype=f32, device=dev),
                "indices_center": torch.empty((B, M), dtype=torch.int64, device=dev),
                "obj_mask": torch.empty((B, M), dtype=torch.uint8, device=dev)}

    def params(self, hflipped, B: int) -> "_lib.SfaTargetParams":
        p = _lib.SfaTargetParams()
        p.boundary = _boundary_arr(self.boundary)
        p.hm_h, p.hm_w = self.hm_size
        p.num_classes, p.max_objects = self.num_classes, self.max_objects
        mask = 0
        if hflipped is not None:
            flips = [bool(f) for f in hflipped]
            if len(flips) != B:
                raise ValueError(f"build_targets: {len(flips)} hflipped flags for {B} frames")
            mask = sum(1 << b for b, f in enumerate(flips) if f)
        p.hflip_mask_lo, p.hflip_mask_hi = mask & 0xFFFFFFFF, mask >> 32
        return p

    def __call__(self, labels, offsets, hflipped=None, out: dict = None, verify: bool = True) -> dict:
        if isinstance(labels, np.ndarray):
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float32).reshape(-1, 8)).to(self.dev)
        labels = _require_gpu_tensor(labels, "build_targets")
        if labels.dim() != 2 or labels.shape[1] != 8:
            raise ValueError(f"build_targets: labels {tuple(labels.shape)}, expected (N, 8)")
        if not isinstance(offsets, torch.Tensor):
            offsets = torch.tensor([int(o) for o in offsets], dtype=torch.int64).to(self.dev)
        offsets = _require_gpu_tensor(offsets, "build_targets offsets", torch.int64)
        B = int(offsets.numel()) - 1
        if B < 1 or B > _lib.TARGET_MAX_BATCH:
            raise ValueError(f"build_targets: {B} frames; 1..{_lib.TARGET_MAX_BATCH} per call")
        n = int(labels.shape[0])
        rows = labels if n else torch.zeros((1, 8), dtype=torch.float32, device=self.dev)
        out = self.alloc(B) if out is None else out
        if self.status is None or self.status.numel() != B:
            self.status = torch.empty(B, dtype=torch.int32, device=self.dev)  # the uint32 words
        p = self.params(hflipped, B)
        check_rc = lib().sfa_build_targets(
            rows.data_ptr(), offsets.data_ptr(), n, B, ctypes.byref(p), out["hm_cen"].data_ptr(),
            out["cen_offset"].data_ptr(), out["direction"].data_ptr(), out["z_coor"].data_ptr(),
            out["dim"].data_ptr(), out["indices_center"].data_ptr(), out["obj_mask"].data_ptr(),
            self.status.data_ptr(), _lib.stream_ptr(self.dev))
        check(check_rc, "sfa_build_targets")
        if verify:
            bad = [b for b, s in enumerate(self.status.cpu().tolist()) if s & _lib.STATUS_BAD_CLASS]
            if bad:
                raise IndexError(f"build_targets: frames {bad} hold a class id outside "
                                 f"[-{self.num_classes + 1}, {self.num_classes})")
        return out


class LossEvaluator:
    """Compute_Loss.forward (losses/losses.py:138-163) on the device (sfa_compute_loss): owns the
    workspace and the output words.  ``__call__`` returns the float32 [6] GPU tensor
    [total, hm_cen, cen_offset, dim, direction, z_coor] (LOSS_KEYS order); ``sums`` holds the float64
    pieces, ``status`` the bad-index word.  ``verify`` (default) reads the status word back and raises
    IndexError as the reference's gather does; with ``verify=False`` the call only enqueues its three
    launches and can be captured into a HIP graph.  :meth:`grad` gives the gradient of the total at the
    five head maps."""

    def __init__(self, device):
        self.dev = torch.device(device)
        self.loss = torch.empty(6, dtype=torch.float32, device=self.dev)
        self.sums = torch.empty(8, dtype=torch.float64, device=self.dev)
        self.status = torch.empty(1, dtype=torch.int32, device=self.dev)
        self.grad_status = torch.empty(1, dtype=torch.int32, device=self.dev)
        self._ws = {}

    @staticmethod
    def workspace_bytes(B, C, H, W, M) -> int:
        return int(lib().sfa_compute_loss_workspace_size(B, C, H, W, M))

    def _operands(self, outputs: dict, targets: dict):
        heads = [_require_gpu_tensor(outputs[k], f"Compute_Loss outputs[{k!r}]") for k in DEFAULT_HEADS]
        tg = [_require_gpu_tensor(targets[k], f"Compute_Loss targets[{k!r}]") for k in TARGET_KEYS[:5]]
        ind = _require_gpu_tensor(targets["indices_center"], "Compute_Loss indices_center", torch.int64)
        msk = targets["obj_mask"]
        if isinstance(msk, torch.Tensor) and msk.dtype == torch.bool:
            msk = msk.to(torch.uint8)
        msk = _require_gpu_tensor(msk, "Compute_Loss obj_mask", torch.uint8)
        if heads[0].dim() != 4:
            raise ValueError(f"Compute_Loss: hm_cen {tuple(heads[0].shape)}, expected (B, C, H, W)")
        B, C, H, W = (int(v) for v in heads[0].shape)
        if ind.dim() != 2 or int(ind.shape[0]) != B:
            raise ValueError(f"Compute_Loss: indices_center {tuple(ind.shape)} for a batch of {B}")
        M = int(ind.shape[1])
        for t, c in zip(heads, (C, 2, 2, 1, 3)):
            if tuple(t.shape) != (B, c, H, W):
                raise ValueError(f"Compute_Loss: map shape {tuple(t.shape)} != {(B, c, H, W)}")
        for t, s in zip(tg + [ind, msk], ((B, C, H, W), (B, M, 2), (B, M, 2), (B, M, 1), (B, M, 3), (B, M), (B, M))):
            if tuple(t.shape) != s:
                raise ValueError(f"Compute_Loss: target shape {tuple(t.shape)} != {s}")
        return heads, tg, ind, msk, (B, C, H, W, M)

    def _workspace(self, tag: str, need: int, shape):
        if need == 0:
            B, C, H, W, M = shape
            raise ValueError(f"Compute_Loss: shape B={B}, C={C}, H={H}, W={W}, M={M} outside the kernels' range")
        sp = _lib.stream_ptr(self.dev)
        ws = self._ws.get((tag, sp, need))
        if ws is None:
            ws = self._ws[(tag, sp, need)] = torch.empty(need // 8, dtype=torch.float64, device=self.dev)
        return ws, sp

    def __call__(self, outputs: dict, targets: dict, apply_sigmoid: bool = False, verify: bool = True):
        heads, tg, ind, msk, shape = self._operands(outputs, targets)
        B, C, H, W, M = shape
        need = self.workspace_bytes(B, C, H, W, M)
        ws, sp = self._workspace("loss", need, shape)
        check_rc = lib().sfa_compute_loss(*(t.data_ptr() for t in heads), *(t.data_ptr() for t in tg), ind.data_ptr(),
                                          msk.data_ptr(), B, C, H, W, M, 1 if apply_sigmoid else 0,
                                          self.loss.data_ptr(), self.sums.data_ptr(), self.status.data_ptr(),
                                          ws.data_ptr(), need, sp)
        check(check_rc, "sfa_compute_loss")
        if verify and int(self.status.item()) & _lib.STATUS_INDEX_OUT_OF_MAP:
            raise IndexError(f"Compute_Loss: an indices_center entry under a set obj_mask is outside [0, {H * W})")
        return self.loss

    @staticmethod
    def grad_workspace_bytes(B, C, H, W, M) -> int:
        return int(lib().sfa_compute_loss_grad_workspace_size(B, C, H, W, M))

    def grad(self, outputs: dict, targets: dict, apply_sigmoid: bool = False, verify: bool = True,
             out: dict = None) -> dict:
        """d total_loss / d (the five head maps) (sfa_compute_loss_grad): a dict of float32 GPU tensors of
        the heads' shapes under the heads' keys, every element written by the call.  With
        ``apply_sigmoid`` hm_cen and cen_offset are logits and their gradients are taken with respect to
        the logits, otherwise with respect to the clamped probabilities.  ``out`` (a dict of contiguous
        tensors) receives the maps instead of fresh tensors; with it and ``verify=False`` the call only
        enqueues its three launches and can be captured into a HIP graph.  ``grad_status`` holds the
        bad-index word; ``verify`` reads it back and raises IndexError like ``__call__``."""
        heads, tg, ind, msk, shape = self._operands(outputs, targets)
        B, C, H, W, M = shape
        need = self.grad_workspace_bytes(B, C, H, W, M)
        ws, sp = self._workspace("grad", need, shape)
        if out is None:
            out = {k: torch.empty_like(t) for k, t in zip(DEFAULT_HEADS, heads)}
        grads = [_require_gpu_tensor(out[k], f"Compute_Loss grad out[{k!r}]") for k in DEFAULT_HEADS]
        for k, t, h in zip(DEFAULT_HEADS, grads, heads):
            if t.shape != h.shape or t.data_ptr() != out[k].data_ptr():
                raise ValueError(f"Compute_Loss grad out[{k!r}]: a contiguous tensor of shape {tuple(h.shape)} is needed")
        check_rc = lib().sfa_compute_loss_grad(*(t.data_ptr() for t in heads), *(t.data_ptr() for t in tg),
                                               ind.data_ptr(), msk.data_ptr(), B, C, H, W, M,
                                               1 if apply_sigmoid else 0, *(t.data_ptr() for t in grads),
                                               self.grad_status.data_ptr(), ws.data_ptr(), need, sp)
        check(check_rc, "sfa_compute_loss_grad")
        if verify and int(self.grad_status.item()) & _lib.STATUS_INDEX_OUT_OF_MAP:
            raise IndexError(f"Compute_Loss: an indices_center entry under a set obj_mask is outside [0, {H * W})")
        return dict(zip(DEFAULT_HEADS, grads))


# ------------------------------------------------- apply_kfpn as an operator: forward + gradient
def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _opt_ptr(t):
    return None if t is None else t.data_ptr()


def _dparams(tensors):
    """The ``dparams`` argument of a gradient entry: its pointers, null where not wanted; None when none is."""
    if all(t is None for t in tensors):
        return None
    return (ctypes.c_void_p * len(tensors))(*[_opt_ptr(t) for t in tensors])


def _workspace(what, dims, need, workspace, device):
    """The workspace of an operator call: the caller's, or a fresh one of ``need`` bytes.  ``need`` == 0 is the size
    query's refusal of ``dims``: ValueError with the library's text."""
    if need == 0:
        msg = lib().sfa_last_error_string()
        raise ValueError(f"{what}: {dims} refused: {msg.decode() if msg else ''}")
    return workspace if workspace is not None else torch.empty(need, dtype=torch.uint8, device=device)


def bn_unfold_grad(weight, gamma, mean, var, eps, dWf, dbf, want=(True, True, True)):
    """The gradients of a convolution weight and of the BatchNorm after it from the gradients ``dWf``, ``dbf`` of their
    folded form W' = s W, b' = beta - mean s, s = gamma / sqrt(var + eps) (sfa_bn_unfold_grad; float64 from the
    float32 operands, rounded once).  ``weight`` (Cout, ...) and ``dWf`` of its shape, ``gamma``, ``mean``, ``var``,
    ``dbf`` (Cout): contiguous float32 GPU tensors.  Returns (dW, dgamma, dbeta), None where ``want`` is False.  One
    launch on the current stream."""
    ts = [_require_gpu_tensor(t, f"bn_unfold_grad {n}").detach() for t, n in
          ((weight, "weight"), (gamma, "gamma"), (mean, "mean"), (var, "var"), (dWf, "dWf"), (dbf, "dbf"))]
    weight, gamma, mean, var, dWf, dbf = ts
    cout = int(weight.shape[0])
    K = weight.numel() // max(cout, 1)
    if tuple(dWf.shape) != tuple(weight.shape) or any(tuple(t.shape) != (cout,) for t in (gamma, mean, var, dbf)):
        raise ValueError("bn_unfold_grad: dWf must have weight's shape and gamma, mean, var, dbf its (Cout,)")
    if not all(t.is_contiguous() for t in ts):
        raise ValueError("bn_unfold_grad: the operands must be contiguous")
    if not any(want):
        return None, None, None
    dW = torch.empty_like(weight) if want[0] else None
    dg = torch.empty_like(gamma) if want[1] else None
    dbt = torch.empty_like(gamma) if want[2] else None
    with torch.cuda.device(weight.device):
        check(lib().sfa_bn_unfold_grad(weight.data_ptr(), gamma.data_ptr(), mean.data_ptr(), var.data_ptr(), float(eps),
                                       dWf.data_ptr(), dbf.data_ptr(), cout, K, _opt_ptr(dW), _opt_ptr(dg), _opt_ptr(dbt),
                                       _lib.stream_ptr(weight.device)), "sfa_bn_unfold_grad")
    return dW, dg, dbt


# ------------------------------------------------- one BasicBlock in training mode (batch statistics): no engine
def _block_train_dims(what, layer, block, x, params):
    cin, cout, s, ds = KfpnEngine.block_shape(layer, block)
    x = _require_gpu_tensor(x, f"{what} x")
    if x.dim() != 4 or int(x.shape[3]) != cin:
        raise ValueError(f"{what} x: {tuple(x.shape)} is not the NHWC (B, h, w, {cin}) of layer{layer}.{block}")
    B, h, w, _ = (int(v) for v in x.shape)
    shapes = [(cout, cin, 3, 3), (cout,), (cout,), (cout, cout, 3, 3), (cout,), (cout,)]
    shapes += [(cout, cin, 1, 1), (cout,), (cout,)] if ds else []
    params = list(params)
    if len(params) != len(shapes):
        raise ValueError(f"{what}: layer{layer}.{block} takes {len(shapes)} parameters, got {len(params)}")
    ps = []
    for i, (t, sh) in enumerate(zip(params, shapes)):
        t = _require_gpu_tensor(t, f"{what} params[{i}]").detach()
        if tuple(t.shape) != sh or not t.is_contiguous():
            raise ValueError(f"{what} params[{i}]: a contiguous tensor of shape {sh} is needed, got {tuple(t.shape)}")
        ps.append(t)
    return x, B, h, w, cin, cout, ds, (B, -(-h // s), -(-w // s), cout), ps, shapes


def _params9(ps):
    return (ctypes.c_void_p * 9)(*([t.data_ptr() for t in ps] + [None] * (9 - len(ps))))


def block_train_forward_workspace_bytes(layer, block, B, h, w, max_chunk_pixels: int = 0) -> int:
    return int(lib().sfa_block_train_forward_workspace_size(layer, block, B, h, w, int(max_chunk_pixels)))


def block_train_grad_workspace_bytes(layer, block, B, h, w, max_chunk_pixels: int = 0) -> int:
    return int(lib().sfa_block_train_grad_workspace_size(layer, block, B, h, w, int(max_chunk_pixels)))


def block_train_chunk_pixels(layer, block, which: int, B, h, w, max_chunk_pixels: int = 0) -> int:
    """K_c of dW1 (which = 0), dW2 (1) or dWd (2) in :func:`block_train_grad`, or the pixels of one statistics block
    (3); 0 for what the entries refuse."""
    return int(lib().sfa_block_train_chunk_pixels(layer, block, int(which), B, h, w, int(max_chunk_pixels)))


def block_train_forward(layer: int, block: int, x: torch.Tensor, params, eps: float = 1e-5, out: dict = None,
                        max_chunk_pixels: int = 0, workspace: torch.Tensor = None) -> dict:
    """BasicBlock layer{layer}.{block} in training mode (sfa_block_train_forward) on a caller's ``x``, float32 NHWC
    (B, h, w, Cin) on the GPU: every BatchNorm normalises with the statistics of the batch.  ``params``: conv1.weight,
    bn1.weight, bn1.bias, conv2.weight, bn2.weight, bn2.bias and, on a block with a downsample, downsample.0.weight,
    downsample.1.weight, downsample.1.bias: raw contiguous float32 GPU tensors in torch's shapes (no engine, no host
    repack).  Returns {z1, mid, z2, zd (None without a downsample), y, stats}: the NHWC maps (B, oh, ow, Cout) and
    ``stats`` (nbn, 2, Cout), the batch mean and biased variance of BatchNorm 1, 2 and the downsample's.  ``out`` (the
    same keys) receives them instead; with ``out`` and ``workspace`` given the call only enqueues its launches."""
    what = "block_train_forward"
    x, B, h, w, _, cout, ds, osh, ps, _ = _block_train_dims(what, layer, block, x, params)
    names = ["z1", "mid", "z2"] + (["zd"] if ds else []) + ["y", "stats"]
    shapes = [osh] * (len(names) - 1) + [(3 if ds else 2, 2, cout)]
    bufs = dict(zip(names, _kfpn_buffers(out, names, shapes, x, f"{what} out")))
    bufs.setdefault("zd", None)
    workspace = _workspace(what, f"B={B}, h={h}, w={w}",
                           block_train_forward_workspace_bytes(layer, block, B, h, w, max_chunk_pixels), workspace, x.device)
    with torch.cuda.device(x.device):
        check(lib().sfa_block_train_forward(layer, block, x.data_ptr(), _params9(ps), float(eps), B, h, w,
                                            bufs["z1"].data_ptr(), bufs["mid"].data_ptr(), bufs["z2"].data_ptr(),
                                            _opt_ptr(bufs["zd"]), bufs["y"].data_ptr(), bufs["stats"].data_ptr(),
                                            int(max_chunk_pixels), workspace.data_ptr(), workspace.numel(),
                                            _lib.stream_ptr(x.device)), "sfa_block_train_forward")
    return bufs


def block_train_grad(layer: int, block: int, x, maps: dict, gy, params, eps: float = 1e-5, want_x: bool = True,
                     want_params=(True,) * 9, out=None, max_chunk_pixels: int = 0, workspace: torch.Tensor = None):
    """The gradients of layer{layer}.{block} in training mode (sfa_block_train_grad), every BatchNorm differentiated
    through its batch statistics, from ``gy`` = d total / d y, ``x`` and ``maps`` = what :func:`block_train_forward`
    returned.  Returns (dx, [dW1, dgamma1, dbeta1, dW2, dgamma2, dbeta2, dWd, dgammad, dbetad]) in torch's shapes,
    None where not wanted (the last three are None on a block without a downsample whatever ``want_params`` says);
    every element of a wanted output is written.  ``out`` = (tensor or None, 9 tensors or Nones) receives them
    instead of fresh tensors.  With ``out`` and ``workspace`` given the call only enqueues its launches."""
    what = "block_train_grad"
    x, B, h, w, cin, cout, ds, osh, ps, pshapes = _block_train_dims(what, layer, block, x, params)
    ms = {}
    for n in ["z1", "mid", "z2", "y"] + (["zd"] if ds else []):
        ms[n] = _require_gpu_tensor(maps[n], f"{what} {n}")
    ms["gy"] = _require_gpu_tensor(gy, f"{what} gy")
    for n, t in ms.items():
        if tuple(t.shape) != osh or not t.is_contiguous():
            raise ValueError(f"{what} {n}: a contiguous NHWC {osh} is needed, got {tuple(t.shape)}")
    stats = _require_gpu_tensor(maps["stats"], f"{what} stats")
    if tuple(stats.shape) != (3 if ds else 2, 2, cout) or not stats.is_contiguous():
        raise ValueError(f"{what} stats: a contiguous {(3 if ds else 2, 2, cout)} is needed, got {tuple(stats.shape)}")
    want = [bool(want_x)] + [bool(v) for v in list(want_params)[:9]] + [False] * (9 - len(list(want_params)[:9]))
    if not ds:
        want[7:10] = [False] * 3
    shapes = [(B, h, w, cin)] + pshapes + ([(1,)] * 3 if not ds else [])
    given = out and ([out[0]] + list(out[1]) + [None] * (9 - len(out[1])))
    res = _grad_outputs(what, want, shapes, given, x)
    workspace = _workspace(what, f"B={B}, h={h}, w={w}",
                           block_train_grad_workspace_bytes(layer, block, B, h, w, max_chunk_pixels), workspace, x.device)
    with torch.cuda.device(x.device):
        check(lib().sfa_block_train_grad(layer, block, x.data_ptr(), ms["z1"].data_ptr(), ms["mid"].data_ptr(),
                                         ms["z2"].data_ptr(), _opt_ptr(ms.get("zd")), ms["y"].data_ptr(),
                                         ms["gy"].data_ptr(), stats.data_ptr(), _params9(ps), float(eps), B, h, w,
                                         _opt_ptr(res[0]), _dparams(res[1:]), int(max_chunk_pixels), workspace.data_ptr(),
                                         workspace.numel(), _lib.stream_ptr(x.device)), "sfa_block_train_grad")
    return res[0], res[1:]


# ------------------------------------------------- the stem in training mode (batch statistics): no engine
_STEM_TRAIN_PARAM_SHAPES = ((64, 3, 7, 7), (64,), (64,))


def _stem_train_dims(what, x, params):
    x = _require_gpu_tensor(x, f"{what} x")
    if x.dim() != 4 or int(x.shape[1]) != 3:
        raise ValueError(f"{what} x: {tuple(x.shape)} is not the NCHW (B, 3, H, W)")
    B, _, H, W = (int(v) for v in x.shape)
    params = list(params)
    if len(params) != 3:
        raise ValueError(f"{what}: the stem takes 3 parameters, got {len(params)}")
    ps = []
    for i, (t, sh) in enumerate(zip(params, _STEM_TRAIN_PARAM_SHAPES)):
        t = _require_gpu_tensor(t, f"{what} params[{i}]").detach()
        if tuple(t.shape) != sh or not t.is_contiguous():
            raise ValueError(f"{what} params[{i}]: a contiguous tensor of shape {sh} is needed, got {tuple(t.shape)}")
        ps.append(t)
    return x, B, H, W, ps


def stem_train_forward_workspace_bytes(B, H, W, max_chunk_pixels: int = 0) -> int:
    return int(lib().sfa_stem_train_forward_workspace_size(B, H, W, int(max_chunk_pixels)))


def stem_train_grad_workspace_bytes(B, H, W, max_chunk_pixels: int = 0) -> int:
    return int(lib().sfa_stem_train_grad_workspace_size(B, H, W, int(max_chunk_pixels)))


def stem_train_chunk_pixels(which: int, B, H, W, max_chunk_pixels: int = 0) -> int:
    """K_c of dW (which = 0) in :func:`stem_train_grad`, or the pixels of one statistics block (1); 0 for what the
    entries refuse."""
    return int(lib().sfa_stem_train_chunk_pixels(int(which), B, H, W, int(max_chunk_pixels)))


def stem_train_forward(x: torch.Tensor, params, eps: float = 1e-5, out: dict = None, max_chunk_pixels: int = 0,
                       workspace: torch.Tensor = None) -> dict:
    """The stem in training mode (sfa_stem_train_forward) on a caller's ``x``, float32 NCHW (B, 3, H, W) on the GPU:
    bn1 normalises with the statistics of the batch.  ``params``: conv1.weight, bn1.weight, bn1.bias, raw contiguous
    float32 GPU tensors in torch's shapes (no engine, no host repack).  Returns {z, a, pooled, stats}: the NHWC maps
    (B, oh, ow, 64) of the raw convolution and of the ReLU, its max-pool (B, ph, pw, 64), and ``stats`` (2, 64), the
    batch mean and biased variance.  ``out`` (the same keys) receives them instead; with ``out`` and ``workspace``
    given the call only enqueues its launches."""
    what = "stem_train_forward"
    x, B, H, W, ps = _stem_train_dims(what, x, params)
    ash, psh = KfpnEngine.stem_shapes(B, H, W)
    names = ["z", "a", "pooled", "stats"]
    bufs = dict(zip(names, _kfpn_buffers(out, names, [ash, ash, psh, (2, 64)], x, f"{what} out")))
    workspace = _workspace(what, f"B={B}, H={H}, W={W}", stem_train_forward_workspace_bytes(B, H, W, max_chunk_pixels),
                           workspace, x.device)
    with torch.cuda.device(x.device):
        check(lib().sfa_stem_train_forward(x.data_ptr(), _ptr_array(ps), float(eps), B, H, W, bufs["z"].data_ptr(),
                                           bufs["a"].data_ptr(), bufs["pooled"].data_ptr(), bufs["stats"].data_ptr(),
                                           int(max_chunk_pixels), workspace.data_ptr(), workspace.numel(),
                                           _lib.stream_ptr(x.device)), "sfa_stem_train_forward")
    return bufs


def stem_train_grad(x, maps: dict, gp, params, eps: float = 1e-5, want_x: bool = True, want_params=(True, True, True),
                    out=None, max_chunk_pixels: int = 0, workspace: torch.Tensor = None):
    """The gradients of the stem in training mode (sfa_stem_train_grad), bn1 differentiated through its batch
    statistics, from ``gp`` = d total / d pooled (NHWC), ``x`` and ``maps`` = what :func:`stem_train_forward` returned
    (z, a and stats are read).  Returns (dx, [dW, dgamma, dbeta]) in torch's shapes, None where not wanted; every
    element of a wanted output is written.  ``out`` = (tensor or None, 3 tensors or Nones) receives them instead of
    fresh tensors.  With ``out`` and ``workspace`` given the call only enqueues its launches."""
    what = "stem_train_grad"
    x, B, H, W, ps = _stem_train_dims(what, x, params)
    ash, psh = KfpnEngine.stem_shapes(B, H, W)
    ms = []
    for t, n, s in ((maps["z"], "z", ash), (maps["a"], "a", ash), (gp, "gp", psh), (maps["stats"], "stats", (2, 64))):
        t = _require_gpu_tensor(t, f"{what} {n}")
        if tuple(t.shape) != s:
            raise ValueError(f"{what} {n}: {tuple(t.shape)} is not the {s} the forward wrote")
        ms.append(t)
    want = [bool(want_x)] + [bool(v) for v in list(want_params)[:3]]
    want += [False] * (4 - len(want))
    shapes = [(B, 3, H, W)] + list(_STEM_TRAIN_PARAM_SHAPES)
    res = _grad_outputs(what, want, shapes, out and ([out[0]] + list(out[1])), x)
    workspace = _workspace(what, f"B={B}, H={H}, W={W}", stem_train_grad_workspace_bytes(B, H, W, max_chunk_pixels),
                           workspace, x.device)
    with torch.cuda.device(x.device):
        check(lib().sfa_stem_train_grad(x.data_ptr(), *(t.data_ptr() for t in ms), _ptr_array(ps), float(eps), B, H, W,
                                        _opt_ptr(res[0]), _dparams(res[1:]), int(max_chunk_pixels), workspace.data_ptr(),
                                        workspace.numel(), _lib.stream_ptr(x.device)), "sfa_stem_train_grad")
    return res[0], res[1:]


def _kfpn_operands(levels_by_head: dict, level0_half: bool, what: str):
    """Checks {head: [level 0, level 1, level 2]}: (names, flat contiguous tensors, channels, (B, h, w))."""
    if not isinstance(levels_by_head, dict) or not 1 <= len(levels_by_head) <= _lib.SFA_MAX_HEADS:
        raise ValueError(f"{what}: a dict of 1..{_lib.SFA_MAX_HEADS} heads is needed")
    names, flat, channels, shape, dev = list(levels_by_head), [], [], None, None
    for name in names:
        lv = list(levels_by_head[name])
        if len(lv) != 3:
            raise ValueError(f"{what}: head {name!r} has {len(lv)} levels, expected 3")
        lv = [_require_gpu_tensor(t, f"{what} levels[{name!r}][{i}]") for i, t in enumerate(lv)]
        if lv[1].dim() != 4:
            raise ValueError(f"{what}: head {name!r} level 1 is {tuple(lv[1].shape)}, expected (B, c, h, w)")
        B, c, h, w = (int(v) for v in lv[1].shape)
        if shape is None:
            shape, dev = (B, h, w), lv[1].device
        if level0_half and (h % 2 or w % 2):
            raise ValueError(f"{what}: level0_half needs even h and w, got {h} x {w}")
        want = [(B, c, h // 2, w // 2) if level0_half else (B, c, h, w), (B, c, h, w), (B, c, h, w)]
        for i, t in enumerate(lv):
            if tuple(t.shape) != want[i] or (B, h, w) != shape or t.device != dev:
                raise ValueError(f"{what}: head {name!r} level {i} is {tuple(t.shape)} on {t.device}, expected "
                                 f"{want[i]} (B, h, w = {shape}) on {dev}")
        flat += lv
        channels.append(c)
    return names, flat, channels, shape


def _kfpn_buffers(given, names, shapes, like, what):
    """The output tensors of one entry: fresh ones, or the caller's (contiguous, of the right shape)."""
    if given is None:
        return [torch.empty(s, dtype=torch.float32, device=like.device) for s in shapes]
    out = []
    for name, s in zip(names, shapes):
        t = _require_gpu_tensor(given[name], f"{what}[{name!r}]")
        if tuple(t.shape) != tuple(s) or t.data_ptr() != given[name].data_ptr():
            raise ValueError(f"{what}[{name!r}]: a contiguous tensor of shape {tuple(s)} is needed")
        out.append(t)
    return out


def _grad_outputs(what, want, shapes, given, like):
    """The outputs of a gradient entry, in order: None where ``want`` is False, the caller's tensor where ``given``
    (a list, or None) has one, else a fresh one."""
    res = []
    for k, (wnt, s) in enumerate(zip(want, shapes)):
        if not wnt:
            res.append(None)
        elif not given or given[k] is None:
            res.append(torch.empty(s, dtype=torch.float32, device=like.device))
        else:
            res.append(_kfpn_buffers({0: given[k]}, [0], [s], like, f"{what} out[{k}]")[0])
    return res


def kfpn_combine(levels_by_head: dict, level0_half: bool = False, return_weights: bool = False, out: dict = None,
                 weights: dict = None):
    """apply_kfpn (models/fpn_resnet.py:248-254) for every head of ``levels_by_head`` = {head: [level 0, level 1,
    level 2]} in one launch (sfa_kfpn_combine).  Levels 1 and 2 are float32 GPU tensors (B, c, h, w); level 0 too,
    or (B, c, h / 2, w / 2) with ``level0_half`` (the nearest resize of :229-230 is read in place).  Returns
    {head: (B, c, h, w)}, with ``return_weights`` also {head: (B, c, h, w, 3)}, the softmax over the levels.  Not
    differentiable (see :func:`kfpn_heads`); ``out`` / ``weights`` (dicts of contiguous tensors) receive the
    results instead of fresh tensors, and the call then only enqueues its launch (graph-capturable)."""
    names, flat, channels, (B, h, w) = _kfpn_operands(levels_by_head, level0_half, "kfpn_combine")
    shapes = [(B, c, h, w) for c in channels]
    outs = _kfpn_buffers(out, names, shapes, flat[0], "kfpn_combine out")
    wts = None
    if return_weights or weights is not None:
        wts = _kfpn_buffers(weights, names, [s + (3,) for s in shapes], flat[0], "kfpn_combine weights")
    with torch.cuda.device(flat[0].device):
        check(lib().sfa_kfpn_combine(_ptr_array(flat), (ctypes.c_int * len(channels))(*channels), len(names), B, h, w,
                                     1 if level0_half else 0, _ptr_array(outs), _ptr_array(wts) if wts else None,
                                     _lib.stream_ptr(flat[0].device)), "sfa_kfpn_combine")
    res = dict(zip(names, outs))
    return (res, dict(zip(names, wts))) if wts is not None else res


def kfpn_combine_grad(levels_by_head: dict, grad_out_by_head: dict, level0_half: bool = False, out: dict = None):
    """The gradient of apply_kfpn at the level maps (sfa_kfpn_combine_grad): ``grad_out_by_head`` = {head:
    d total / d out, (B, c, h, w)}; returns {head: [d total / d level 0, 1, 2]} of the levels' shapes, every
    element written by the call (float64 from the float32 operands, rounded once; under ``level0_half`` a level-0
    cell gathers its four children in a fixed order, so runs are bit-identical).  ``out`` ({head: [three
    contiguous tensors]}) receives the maps instead of fresh tensors; the call then only enqueues its launch."""
    names, flat, channels, (B, h, w) = _kfpn_operands(levels_by_head, level0_half, "kfpn_combine_grad")
    gouts = []
    for name, c in zip(names, channels):
        g = _require_gpu_tensor(grad_out_by_head[name], f"kfpn_combine_grad grad_out[{name!r}]")
        if tuple(g.shape) != (B, c, h, w):
            raise ValueError(f"kfpn_combine_grad grad_out[{name!r}]: {tuple(g.shape)} != {(B, c, h, w)}")
        gouts.append(g)
    if out is None:
        glev = [torch.empty_like(t) for t in flat]
    else:
        glev = []
        for name, lv in zip(names, (flat[i:i + 3] for i in range(0, len(flat), 3))):
            glev += _kfpn_buffers(dict(enumerate(out[name])), range(3), [t.shape for t in lv], lv[0],
                                  f"kfpn_combine_grad out[{name!r}]")
    with torch.cuda.device(flat[0].device):
        check(lib().sfa_kfpn_combine_grad(_ptr_array(flat), (ctypes.c_int * len(channels))(*channels), len(names), B, h,
                                          w, 1 if level0_half else 0, _ptr_array(gouts), _ptr_array(glev),
                                          _lib.stream_ptr(flat[0].device)), "sfa_kfpn_combine_grad")
    return {name: glev[3 * j:3 * j + 3] for j, name in enumerate(names)}


class _KfpnCombine(torch.autograd.Function):
    """apply_kfpn of all heads with its gradient, both from the HIP library: forward runs sfa_kfpn_combine and
    saves the level tensors, backward runs sfa_kfpn_combine_grad on them.  The outputs come first, then (when
    wanted) the weights, which are marked non-differentiable (the reference only ever detaches them)."""

    @staticmethod
    def forward(ctx, names, level0_half, want_weights, *levels):
        by_head = {n: levels[3 * j:3 * j + 3] for j, n in enumerate(names)}
        res = kfpn_combine(by_head, level0_half, return_weights=want_weights)
        ctx.names, ctx.half = tuple(names), bool(level0_half)
        ctx.save_for_backward(*levels)
        if not want_weights:
            return tuple(res[n] for n in names)
        wts = tuple(res[1][n] for n in names)
        ctx.mark_non_differentiable(*wts)
        return tuple(res[0][n] for n in names) + wts

    @staticmethod
    def backward(ctx, *grads):
        levels, n = ctx.saved_tensors, len(ctx.names)
        by_head = {name: levels[3 * j:3 * j + 3] for j, name in enumerate(ctx.names)}
        g = kfpn_combine_grad(by_head, dict(zip(ctx.names, grads[:n])), ctx.half)
        flat = [t for name in ctx.names for t in g[name]]
        return (None, None, None) + tuple(t if need else None for t, need in zip(flat, ctx.needs_input_grad[3:]))


def kfpn_heads(levels_by_head: dict, level0_half: bool = True, return_weights: bool = False):
    """The differentiable all-heads form: what the loop of models/fpn_resnet.py:219-244 leaves in ``ret`` from the
    15 per-level head outputs, {head: [level 0, level 1, level 2]}, in one launch; level 0 is taken at half
    resolution as the head convolutions produce it (``level0_half=False``: already (B, c, h, w)).  Returns {head:
    (B, c, h, w)} (with ``return_weights`` also the detached softmax weights per head); ``backward`` through the
    result reaches the level tensors that require grad, again in one launch."""
    names = list(levels_by_head)
    flat = [t for n in names for t in levels_by_head[n]]
    if len(flat) != 3 * len(names):
        raise ValueError("kfpn_heads: every head needs its three levels")
    res = _KfpnCombine.apply(tuple(names), bool(level0_half), bool(return_weights), *flat)
    outs = dict(zip(names, res[:len(names)]))
    return (outs, dict(zip(names, res[len(names):]))) if return_weights else outs
