// Per-sample scale: y[n, ...] = x[n, ...] * scale[n], stochastic depth's forward and -- on dy,
// with the same scale -- its backward. It streams the tensor once and is bandwidth-bound; no
// atomics, no allocation, nothing that synchronises (capturable like every kernel here).
//
// (The stand-alone SiLU, BatchNorm's SiLU kind and the squeeze-excitation gate that EfficientNet
// also needs have no kernels here yet: see ops/activation.py and ops/excite.py.)
#include "common.h"
#include "kernels.h"

namespace tdp {
namespace {

inline unsigned ew4_grid(long n) {
  long g = ((n + 3) / 4 + 255) / 256;
  if (g > 8192) g = 8192;
  return (unsigned)(g < 1 ? 1 : g);
}

// A dense tensor whose samples are `per` consecutive elements (plain-contiguous and
// channels_last alike). A thread owns 4 consecutive elements: one 16-B load and store. The last,
// partial group of 4 -- and every group when a pointer is not 16-B aligned or `per` is no
// multiple of 4 -- goes element by element: a thread's four scalar accesses are then 4 floats
// apart from its neighbour's, only partly coalesced, which is acceptable for a fallback that no
// NHWC activation with C % 4 == 0 takes.
__global__ __launch_bounds__(256) void sample_scale_kernel(const float* __restrict__ x,
                                                           const float* __restrict__ scale,
                                                           long n, long per,
                                                           float* __restrict__ y, int vec) {
  const long groups = (n + 3) / 4;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < groups; t += (long)gridDim.x * 256) {
    const long i0 = 4 * t;
    if (vec && i0 + 4 <= n) {  // vec: per % 4 == 0, so the 4 elements share a sample
      const float sc = scale[i0 / per];
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + i0);
      *reinterpret_cast<f32x4*>(y + i0) = v * sc;
    } else {
      for (int k = 0; k < 4 && i0 + k < n; ++k) y[i0 + k] = x[i0 + k] * scale[(i0 + k) / per];
    }
  }
}

}  // namespace

void sample_scale(const float* x, const float* scale, long samples, long per, float* y,
                  hipStream_t s) {
  const long n = samples * per;
  if (n <= 0) return;
  const int vec = per % 4 == 0 && ((((uintptr_t)x) | ((uintptr_t)y)) & 15) == 0;
  hipLaunchKernelGGL(sample_scale_kernel, dim3(ew4_grid(n)), dim3(256), 0, s, x, scale, n, per,
                     y, vec);
}

}  // namespace tdp
