// The bias gradient and the split-K fold of the float32-MFMA gradient operators (neck.hip, block.hip, stem_grad.hip;
// gfx950).  No atomics; every sum has a fixed order, so runs are bit-identical.
#include "dispatch.h"
#include "grad_host.h"

using namespace sfa;

namespace sfa {

// grid (ceil(M ntaps cin / 256)), block (256): one dW element per thread
__global__ void __launch_bounds__(256) grad_wgrad_fold_kernel(const float* __restrict__ part, int chunks, int M, int cin,
                                                              int ntaps, float* __restrict__ dW, int ldo, int col0) {
  const int N = ntaps * cin;
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= M * N) return;
  const int o = e / N, rem = e - o * N;
  const int tap = rem / cin, c = rem - tap * cin;
  double s = 0.0;
  for (int k = 0; k < chunks; ++k) s += (double)part[(size_t)k * M * N + e];
  dW[((size_t)o * ldo + col0 + c) * ntaps + tap] = (float)s;
}

// grid (blocks, ceil(cout / 256)), block (256): thread o adds g[p][o] (masked by gm) over the block's run of pixels.
// part: [block][cout].
__global__ void __launch_bounds__(256) grad_bias_kernel(const float* __restrict__ g, const float* __restrict__ gm,
                                                        double* __restrict__ part, int npix, int pixels, int cout) {
  const GradRange run = grad_chunk_at((int)blockIdx.x, npix, pixels);
  const int o = (int)blockIdx.y * 256 + (int)threadIdx.x;
  if (o >= cout) return;
  double s = 0.0;
  for (int p = run.first; p < run.first + run.count; ++p) {
    const size_t at = (size_t)p * cout + o;
    const float v = g[at];
    s += (double)((!gm || gm[at] > 0.f) ? v : 0.f);
  }
  part[(size_t)blockIdx.x * cout + o] = s;
}

// grid (ceil(cout / 256)), block (256)
__global__ void __launch_bounds__(256) grad_bias_fold_kernel(const double* __restrict__ part, int blocks, int cout,
                                                             float* __restrict__ db) {
  const int o = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (o >= cout) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += part[(size_t)b * cout + o];
  db[o] = (float)s;
}

}  // namespace sfa

int sfa::launch_wgrad_fold(const float* part, int chunks, int M, int cin, int ntaps, float* dW, int ldo, int col0,
                           hipStream_t st) {
  return launch({dim3((unsigned)ceil_div(M * ntaps * cin, 256)), dim3(256), st}, grad_wgrad_fold_kernel, part, chunks, M,
                cin, ntaps, dW, ldo, col0);
}

int sfa::launch_bias_grad(const GradBias& b, const float* g, const float* gm, double* part, float* db, hipStream_t st) {
  const unsigned cy = (unsigned)ceil_div(b.cout, 256);
  if (int rc = launch({dim3((unsigned)b.blocks, cy), dim3(256), st}, grad_bias_kernel, g, gm, part, b.npix, b.pixels,
                      b.cout))
    return rc;
  return launch({dim3(cy), dim3(256), st}, grad_bias_fold_kernel, part, b.blocks, b.cout, db);
}
