// Weight standardisation (fp32, gfx950): every output filter of a convolution weight brought to
// zero mean and unit variance over its K = Cg*R*S elements, and the backward of that map.
//   mean_o = mean_K(w[o]),  var_o = mean_K((w[o] - mean_o)^2)  (biased)
//   w_hat[o] = (w[o] - mean_o) * rstd_o,  rstd_o = 1 / sqrt(var_o + eps)
//   dw[o]    = rstd_o * (g[o] - mean_K(g[o]) - w_hat[o] * mean_K(g[o] * w_hat[o]))
// In both memory layouts of a Conv2d weight (channels_last [Cout][R][S][Cg], contiguous
// [Cout][Cg][R][S]) filter o is the run of K floats at o*K: the kernels see a dense [rows][K]
// matrix and never learn which layout it was.
//
// Work split: one 64-lane wave owns one row; a 256-thread workgroup holds four waves, so four
// rows; the grid is ceil(rows / 4). Waves of a workgroup share nothing (no LDS, no barrier).
//
// Three forms, chosen on the host from K and the pointers, never per row:
//   register  -- K % 4 == 0, 16-byte aligned, K <= kWsCap. Lane l holds the 16-byte units
//                l, l + 64, l + 128, ... of its row (NV units, NV a template constant picked
//                from K); the row is loaded once, reduced from registers and written once. The
//                backward holds both of its rows (g and w_hat) the same way.
//   streaming -- K % 4 == 0, aligned, K > kWsCap: the same units in the same order, but every
//                pass re-reads the row from memory (from L2 after the first pass).
//   scalar    -- any K, any 4-byte aligned pointer: the streaming form with one-float units.
//
// A row sum is the lane's own units added in ascending order, then the xor butterfly across
// the wave (wave_sum): a function of K alone. No atomics, no scratch; row o of a tensor is
// bitwise that row standardised alone, and two runs agree bitwise.
//
// Numerics. The deviations are taken twice: d = x - m0 with m0 = sum / K (exact by Sterbenz for
// a row with a large common offset), then d -= mean(d), which removes the rounding of m0; the
// variance is sum(d^2) / K from those deviations, never E[x^2] - mean^2. The backward centres g
// the same way before the second row sum. A row whose elements are all equal is detected by
// comparison with its first element (one ballot) and gives d = 0, so w_hat = 0 exactly.
#include <initializer_list>
#include <stdexcept>

#include "common.h"
#include "kernels.h"

namespace tdp {
namespace {

constexpr int kT = 256;                     // 4 waves = 4 rows per workgroup
constexpr int kWsMaxNV = kWsCap / (4 * kWave);  // 16-byte units per lane at the cap (18)

// a unit of V floats (V = 4: one 16-byte access, V = 1: one 4-byte access)
template <int V>
__device__ __forceinline__ void ld(const float* p, float (&r)[V]) {
  if constexpr (V == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3];
  } else {
    r[0] = *p;
  }
}

template <int V>
__device__ __forceinline__ void st(float* p, const float (&r)[V]) {
  if constexpr (V == 4) {
    f32x4 v;
    v[0] = r[0]; v[1] = r[1]; v[2] = r[2]; v[3] = r[3];
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    *p = r[0];
  }
}

__device__ __forceinline__ int ws_row() { return blockIdx.x * (kT / kWave) + (threadIdx.x >> 6); }

// ---------------------------------------------------------------------------- register form
template <int NV>
__global__ __launch_bounds__(kT) void ws_fwd_reg(const float* __restrict__ w, int rows, int K,
                                                 float eps, float* __restrict__ out,
                                                 float* __restrict__ rstd_out) {
  const int row = ws_row(), lane = threadIdx.x & 63;
  if (row >= rows) return;  // the whole wave: waves share nothing
  const float* src = w + (long)row * K;
  const int nu = K >> 2;
  const float Kf = (float)K;
  float v[NV][4];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.f;
    if (i * kWave + lane < nu) ld<4>(src + 4 * (i * kWave + lane), v[i]);
  }
  const float x0 = __shfl(v[0][0], 0, kWave);
  bool same = true;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const bool on = i * kWave + lane < nu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s += v[i][j];
      same = same && (!on || v[i][j] == x0);
    }
  }
  const bool flat = __all(same);
  const float m0 = wave_sum(s) / Kf;
  s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const bool on = i * kWave + lane < nu && !flat;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[i][j] = on ? v[i][j] - m0 : 0.f;
      s += v[i][j];
    }
  }
  const float c = wave_sum(s) / Kf;
  s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const bool on = i * kWave + lane < nu && !flat;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[i][j] = on ? v[i][j] - c : 0.f;
      s = fmaf(v[i][j], v[i][j], s);
    }
  }
  const float rstd = 1.f / sqrtf(wave_sum(s) / Kf + eps);
  float* dst = out + (long)row * K;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (i * kWave + lane < nu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] *= rstd;
      st<4>(dst + 4 * (i * kWave + lane), v[i]);
    }
  }
  if (lane == 0) rstd_out[row] = rstd;
}

template <int NV>
__global__ __launch_bounds__(kT) void ws_bwd_reg(const float* __restrict__ g,
                                                 const float* __restrict__ what,
                                                 const float* __restrict__ rstd_in, int rows,
                                                 int K, float* __restrict__ dw) {
  const int row = ws_row(), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const long base = (long)row * K;
  const int nu = K >> 2;
  const float Kf = (float)K;
  float gv[NV][4], hv[NV][4];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    gv[i][0] = gv[i][1] = gv[i][2] = gv[i][3] = 0.f;
    hv[i][0] = hv[i][1] = hv[i][2] = hv[i][3] = 0.f;
    if (i * kWave + lane < nu) {
      ld<4>(g + base + 4 * (i * kWave + lane), gv[i]);
      ld<4>(what + base + 4 * (i * kWave + lane), hv[i]);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) s += gv[i][j];
  const float a0 = wave_sum(s) / Kf;
  s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const bool on = i * kWave + lane < nu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gv[i][j] = on ? gv[i][j] - a0 : 0.f;
      s += gv[i][j];
    }
  }
  const float a1 = wave_sum(s) / Kf;
  s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const bool on = i * kWave + lane < nu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gv[i][j] = on ? gv[i][j] - a1 : 0.f;
      s = fmaf(gv[i][j], hv[i][j], s);
    }
  }
  const float b = wave_sum(s) / Kf;
  const float rstd = rstd_in[row];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (i * kWave + lane < nu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) gv[i][j] = rstd * fmaf(-hv[i][j], b, gv[i][j]);
      st<4>(dw + base + 4 * (i * kWave + lane), gv[i]);
    }
  }
}

// ------------------------------------------------------------------ streaming / scalar form
// V = 4: 16-byte units (K % 4 == 0, aligned); V = 1: one float per unit (anything).
template <int V>
__global__ __launch_bounds__(kT) void ws_fwd_stream(const float* __restrict__ w, int rows, int K,
                                                    float eps, float* __restrict__ out,
                                                    float* __restrict__ rstd_out) {
  const int row = ws_row(), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* src = w + (long)row * K;
  const int nu = K / V;
  const float Kf = (float)K;
  const float x0 = src[0];
  float r[V];
  bool same = true;
  float s = 0.f;
  for (int u = lane; u < nu; u += kWave) {
    ld<V>(src + V * u, r);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      s += r[j];
      same = same && r[j] == x0;
    }
  }
  const bool flat = __all(same);
  const float m0 = wave_sum(s) / Kf;
  s = 0.f;
  for (int u = lane; u < nu; u += kWave) {
    ld<V>(src + V * u, r);
#pragma unroll
    for (int j = 0; j < V; ++j) s += flat ? 0.f : r[j] - m0;
  }
  const float c = wave_sum(s) / Kf;
  s = 0.f;
  for (int u = lane; u < nu; u += kWave) {
    ld<V>(src + V * u, r);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float d = flat ? 0.f : (r[j] - m0) - c;
      s = fmaf(d, d, s);
    }
  }
  const float rstd = 1.f / sqrtf(wave_sum(s) / Kf + eps);
  float* dst = out + (long)row * K;
  for (int u = lane; u < nu; u += kWave) {
    ld<V>(src + V * u, r);
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = (flat ? 0.f : (r[j] - m0) - c) * rstd;
    st<V>(dst + V * u, r);
  }
  if (lane == 0) rstd_out[row] = rstd;
}

template <int V>
__global__ __launch_bounds__(kT) void ws_bwd_stream(const float* __restrict__ g,
                                                    const float* __restrict__ what,
                                                    const float* __restrict__ rstd_in, int rows,
                                                    int K, float* __restrict__ dw) {
  const int row = ws_row(), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const long base = (long)row * K;
  const int nu = K / V;
  const float Kf = (float)K;
  float r[V], h[V];
  float s = 0.f;
  for (int u = lane; u < nu; u += kWave) {
    ld<V>(g + base + V * u, r);
#pragma unroll
    for (int j = 0; j < V; ++j) s += r[j];
  }
  const float a0 = wave_sum(s) / Kf;
  s = 0.f;
  for (int u = lane; u < nu; u += kWave) {
    ld<V>(g + base + V * u, r);
#pragma unroll
    for (int j = 0; j < V; ++j) s += r[j] - a0;
  }
  const float a1 = wave_sum(s) / Kf;
  s = 0.f;
  for (int u = lane; u < nu; u += kWave) {
    ld<V>(g + base + V * u, r);
    ld<V>(what + base + V * u, h);
#pragma unroll
    for (int j = 0; j < V; ++j) s = fmaf((r[j] - a0) - a1, h[j], s);
  }
  const float b = wave_sum(s) / Kf;
  const float rstd = rstd_in[row];
  for (int u = lane; u < nu; u += kWave) {
    ld<V>(g + base + V * u, r);
    ld<V>(what + base + V * u, h);
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = rstd * fmaf(-h[j], b, (r[j] - a0) - a1);
    st<V>(dw + base + V * u, r);
  }
}

inline bool ws_vec(int K, std::initializer_list<const void*> ptrs) {
  bool ok = K % 4 == 0;
  for (const void* p : ptrs) ok = ok && ((uintptr_t)p & 15) == 0;
  return ok;
}

inline void ws_check(int rows, int K) {
  if (rows < 1 || K < 1) throw std::invalid_argument("weight_std: empty weight");
}

// 0 register, 1 streaming, 2 scalar
inline int ws_form(int K, bool aligned) {
  if (!aligned || K % 4) return 2;
  return K <= kWsCap ? 0 : 1;
}

}  // namespace

// NV of the register form: the smallest of {1, 2, 4, 9, 18} with 256 * NV >= K (ResNet-50's
// filters: 64 -> 1, 256 / 512 -> 1 / 2, 576 / 1024 -> 4, 1152 / 2048 / 2304 -> 9, 4608 -> 18)
#define WS_DISPATCH_NV(K, CALL)          \
  do {                                   \
    if ((K) <= 256) { CALL(1); }         \
    else if ((K) <= 512) { CALL(2); }    \
    else if ((K) <= 1024) { CALL(4); }   \
    else if ((K) <= 2304) { CALL(9); }   \
    else { CALL(kWsMaxNV); }             \
  } while (0)

void ws_fwd(const float* w, int rows, int K, float eps, float* out, float* rstd, hipStream_t s) {
  ws_check(rows, K);
  const dim3 grid((unsigned)ceil_div(rows, kT / kWave)), block(kT);
  const int form = ws_form(K, ws_vec(K, {w, out}));
  if (form == 0) {
#define WS_CALL(NV) \
  hipLaunchKernelGGL(ws_fwd_reg<NV>, grid, block, 0, s, w, rows, K, eps, out, rstd)
    WS_DISPATCH_NV(K, WS_CALL);
#undef WS_CALL
  } else if (form == 1) {
    hipLaunchKernelGGL(ws_fwd_stream<4>, grid, block, 0, s, w, rows, K, eps, out, rstd);
  } else {
    hipLaunchKernelGGL(ws_fwd_stream<1>, grid, block, 0, s, w, rows, K, eps, out, rstd);
  }
}

void ws_bwd(const float* g, const float* what, const float* rstd, int rows, int K, float* dw,
            hipStream_t s) {
  ws_check(rows, K);
  const dim3 grid((unsigned)ceil_div(rows, kT / kWave)), block(kT);
  const int form = ws_form(K, ws_vec(K, {g, what, dw}));
  if (form == 0) {
#define WS_CALL(NV) \
  hipLaunchKernelGGL(ws_bwd_reg<NV>, grid, block, 0, s, g, what, rstd, rows, K, dw)
    WS_DISPATCH_NV(K, WS_CALL);
#undef WS_CALL
  } else if (form == 1) {
    hipLaunchKernelGGL(ws_bwd_stream<4>, grid, block, 0, s, g, what, rstd, rows, K, dw);
  } else {
    hipLaunchKernelGGL(ws_bwd_stream<1>, grid, block, 0, s, g, what, rstd, rows, K, dw);
  }
}

}  // namespace tdp
