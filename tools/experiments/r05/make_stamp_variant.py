#!/usr/bin/env python3
"""Writes tools/experiments/r05/conv_h3s_stamp.h: a DIAGNOSTIC copy of the product strip kernel
(csrc/conv_h3s_kernel.h) with per-k-step s_memtime stamps (tools/stampbench.hip, tools/stamp_summary.py).
Rerun after changing the product kernel."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
SRC = os.path.join(ROOT, "lidar-image_object-detection_-fpn_resnet-yolov8_amd", "csrc", "conv_h3s_kernel.h")
DST = os.path.join(ROOT, "tools", "experiments", "r05", "conv_h3s_stamp.h")


def rep(s, old, new, count=1):
    assert s.count(old) >= 1, old[:80]
    return s.replace(old, new, count)


s = open(SRC).read()
# the option bits (h3sopt) are the product header's: included, not copied
s = rep(s, '#include "conv_r3_kernel.h"', '#include "../../../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/conv_h3s_kernel.h"')
s = s[:s.index("namespace h3sopt {")] + s[s.index("}  // namespace h3sopt\n") + len("}  // namespace h3sopt\n"):]
s = s.replace("conv_h3s_kernel(", "conv_h3s_stamp_kernel(").replace("launch_conv_h3s_cfg", "launch_conv_h3s_stamp_cfg")
s = s.replace(" conv_h3s_kernel<", " conv_h3s_stamp_kernel<")
s = rep(s, "__global__ void __launch_bounds__((BM / WM) * 64, OCC) conv_h3s_stamp_kernel(const ConvArgs a) {",
        """__global__ void __launch_bounds__((BM / WM) * 64, OCC) conv_h3s_stamp_kernel(const ConvArgs a) {
  // DIAGNOSTIC BUILD: s_memtime stamps per k-step of every wave into the buffer passed as a.hout
  // (read by nothing else); record (per block, wave): [0] start, [1] after the prologue, per k-step t:
  // [2 + 5 t + 0..4] before the wait, after the wait, after the barrier, after the DMA issue / presplit,
  // after the compute; [2 + 5 NKS] after the epilogue.  The block's XCC id and HW id at [2 + 5 NKS + 1].
  constexpr int NKS_MAX = 96, REC = 2 + 5 * NKS_MAX + 2;
  unsigned long long* const STP = reinterpret_cast<unsigned long long*>(a.hout) +
                                  ((size_t)blockIdx.x * (BM / WM) + (threadIdx.x >> 6)) * REC;
  auto stamp = [&](int i) {
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    if ((threadIdx.x & 63) == 0) STP[i + (threadIdx.x & 63)] = t;  // lane-dependent address: a vector store
  };
  stamp(0);""")
s = rep(s, """  for (int sl = 0; sl < nsl; ++sl) {
    const int s = s0 + sl;""", """  stamp(1);
  for (int sl = 0; sl < nsl; ++sl) {
    const int s = s0 + sl;""")
s = rep(s, """      const int t = 3 * sl + kw;
      if constexpr (PS) {""", """      const int t = 3 * sl + kw;
      if (t < NKS_MAX) stamp(2 + 5 * t);
      if constexpr (PS) {""")
s = rep(s, """        if constexpr (RW) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // W(t) stores
        __builtin_amdgcn_s_barrier();""", """        if constexpr (RW) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // W(t) stores
        if (t < NKS_MAX) stamp(2 + 5 * t + 1);
        __builtin_amdgcn_s_barrier();
        if (t < NKS_MAX) stamp(2 + 5 * t + 2);""")
s = rep(s, """        if (kw == 0) presplit(smem);
        compute(smem, WB + (t & 1) * W_BYTES, kw);""", """        if (kw == 0) presplit(smem);
        if (t < NKS_MAX) stamp(2 + 5 * t + 3);
        compute(smem, WB + (t & 1) * W_BYTES, kw);
        if (t < NKS_MAX) stamp(2 + 5 * t + 4);""")
s = rep(s, """      if constexpr (RW) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // W(t) stores
      __builtin_amdgcn_s_barrier();  // W(t) (and the strip) landed for every wave; W(t-1) no longer read""",
        """      if constexpr (RW) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // W(t) stores
      if (t < NKS_MAX) stamp(2 + 5 * t + 1);
      __builtin_amdgcn_s_barrier();  // W(t) (and the strip) landed for every wave; W(t-1) no longer read
      if (t < NKS_MAX) stamp(2 + 5 * t + 2);""")
s = rep(s, """      if (kw == 0) load_strip(last ? s : s + 1, sdst);
      compute(smem + (sl & 1) * S_BYTES, WB + (t & 1) * W_BYTES, kw);""", """      if (kw == 0) load_strip(last ? s : s + 1, sdst);
      if (t < NKS_MAX) stamp(2 + 5 * t + 3);
      compute(smem + (sl & 1) * S_BYTES, WB + (t & 1) * W_BYTES, kw);
      if (t < NKS_MAX) stamp(2 + 5 * t + 4);""")
s = rep(s, """  __syncthreads();
  r3t_epilogue_std<TM, TN, NT, false, RESPF, true>(a, acc, smem, m0 + wave * WM, m0, n0, lane, ainv, rvp, CSB);
}""", """  __syncthreads();
  r3t_epilogue_std<TM, TN, NT, false, RESPF, true>(a, acc, smem, m0 + wave * WM, m0, n0, lane, ainv, rvp, CSB);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  stamp(2 + 5 * NKS_MAX);
  {
    unsigned xcc, hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    if ((threadIdx.x & 63) == 0) STP[2 + 5 * NKS_MAX + 1 + (threadIdx.x & 63)] = ((unsigned long long)xcc << 32) | hw;
  }
}""")
s = s.replace("#pragma once", "#pragma once\n// tools/experiments/r05: DIAGNOSTIC copy of the product strip kernel (conv_h3s_kernel.h) with per-k-step\n// s_memtime stamps, generated by make_stamp_variant.py; never built into the library.", 1)
open(DST, "w").write(s)
print("wrote", DST)
