// Group-norm kernels (fp32, gfx950): nn.GroupNorm's forward and backward, with an optional fused
// residual add and ReLU. x is [N][C][HW], G groups of Cg = C / G channels; statistics are taken
// over the Cg*HW elements of one (sample, group):
//   mean[n,g], rstd[n,g] = rsqrt(var + eps) (biased variance)
//   y  = act((x - mean) * rstd * w[c] + b[c] [+ residual])
//   dx = rstd * (w g - mean_g(w g) - xhat * mean_g(w g xhat)),  g = dy gated by the ReLU
//   dw[c] = sum_n sum_hw g xhat,  db[c] = sum_n sum_hw g
//
// Two layout forms:
//   NHWC    -- channels_last [N][HW][C], C % 4 == 0, 16-byte aligned. A thread owns 4 adjacent
//              channels (one 16-byte load per pixel; with Cg < 4 the load spans several groups)
//              and a strip of pixels, as moments_rows4 / elemt_rows4 of norm.hip, and keeps
//              PER-CHANNEL partials; the channels of a (sample, group) are merged afterwards.
//   generic -- any contiguous [N][C][HW]; a (sample, group) is one contiguous run of Cg*HW floats
//              read with scalar (4-byte) loads, so a run may start at any float.
//
// Determinism: no atomics. Every reduction is partitioned by (C, HW, G) alone -- a workgroup never
// spans two samples, and the split of a sample's pixels (or of a run) into workgroup parts is a
// function of C and HW -- and partials are merged in index order. So sample n of a batch is
// bitwise the same sample run alone, and two runs agree bitwise. dw / db sum the per-sample
// values over n in ascending order.
//
// Statistics are Welford per thread and Chan merges (welford.h), never E[x^2] - E[x]^2.
#include <initializer_list>
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "welford.h"

namespace tdp {
namespace {

constexpr int kT = 256;          // threads per workgroup (every kernel here)
constexpr int kRowIters = 16;    // NHWC: pixels per thread per part
constexpr int kRunPart = 4096;   // generic: floats of a run per workgroup part (16 per thread)

// NHWC partition: a workgroup owns CB = min(C, 256) channels (LPR = CB / 4 lanes per pixel row),
// its RPW = 256 / LPR row groups walk a part of P = 16 * RPW pixels of ONE sample.
struct GnRows {
  int CB, LPR, RPW, nblk, P, parts;
};

inline GnRows gn_rows(int C, int HW) {
  GnRows L;
  L.CB = C < 256 ? C : 256;
  L.LPR = L.CB / 4;
  L.RPW = kT / L.LPR;
  L.nblk = (C + L.CB - 1) / L.CB;
  L.P = kRowIters * L.RPW;
  L.parts = (HW + L.P - 1) / L.P;
  return L;
}

__device__ __forceinline__ int pow2_ceil_gn(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

// ---------------------------------------------------------------------------------- statistics
// NHWC: per-channel (count, mean, M2) of one (sample, part) -> ws[n][part][3][C]
__global__ __launch_bounds__(kT) void gn_stats_nhwc(const float* __restrict__ x, int C, int HW,
                                                    GnRows L, float* __restrict__ ws) {
  __shared__ float sh[3][1024];  // RPW * CB <= 1024
  const int bid = blockIdx.x;
  const int cb = bid % L.nblk, part = (bid / L.nblk) % L.parts, n = bid / (L.nblk * L.parts);
  const int t = threadIdx.x, cq = t % L.LPR, rg = t / L.LPR;
  const int c = cb * L.CB + 4 * cq;
  const bool on = rg < L.RPW && c < C;
  const int b = part * L.P, e = b + L.P < HW ? b + L.P : HW;
  float cnt = 0.f, mu[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
  if (on) {
    const float* xs = x + (long)n * HW * C + c;
#pragma unroll 4
    for (int r = b + rg; r < e; r += L.RPW) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xs + (long)r * C);
      cnt += 1.f;
      const float inv = 1.f / cnt;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = v[j] - mu[j];
        mu[j] = fmaf(d, inv, mu[j]);
        m2[j] = fmaf(d, v[j] - mu[j], m2[j]);
      }
    }
  }
  if (rg < L.RPW) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = rg * L.CB + 4 * cq + j;
      sh[0][q] = cnt;
      sh[1][q] = mu[j];
      sh[2][q] = m2[j];
    }
  }
  // tree merge of the RPW row groups (Chan), in a fixed order
  for (int st = pow2_ceil_gn(L.RPW) >> 1; st > 0; st >>= 1) {
    __syncthreads();
    for (int i = t; i < st * L.CB; i += kT) {
      if (i / L.CB + st < L.RPW) {
        const int k = i + st * L.CB;
        const Wf w = wf_merge(Wf{sh[0][i], sh[1][i], sh[2][i]}, Wf{sh[0][k], sh[1][k], sh[2][k]});
        sh[0][i] = w.n; sh[1][i] = w.mean; sh[2][i] = w.m2;
      }
    }
  }
  __syncthreads();
  float* o = ws + ((long)n * L.parts + part) * 3 * C;
  for (int k = t; k < L.CB; k += kT) {
    const int ch = cb * L.CB + k;
    if (ch >= C) continue;
    o[ch] = sh[0][k]; o[C + ch] = sh[1][k]; o[2 * C + ch] = sh[2][k];
  }
}

// generic: (count, mean, M2) of one part of the run of (sample n, group g) -> ws[n][part][3][G]
__global__ __launch_bounds__(kT) void gn_stats_gen(const float* __restrict__ x, long run, int G,
                                                   int parts, float* __restrict__ ws) {
  __shared__ Wf sh[kT / 64];
  const int part = blockIdx.x % parts, ng = blockIdx.x / parts;
  const int n = ng / G, g = ng - n * G;
  const float* xs = x + (long)ng * run;
  const long b = (long)part * kRunPart, e = b + kRunPart < run ? b + kRunPart : run;
  Wf w{0.f, 0.f, 0.f};
  for (long i = b + threadIdx.x; i < e; i += kT) wf_push(w, xs[i]);
  w = wf_wave(w);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    w = wf_merge(wf_merge(sh[0], sh[1]), wf_merge(sh[2], sh[3]));
    float* o = ws + ((long)n * parts + part) * 3 * G;
    o[g] = w.n; o[G + g] = w.mean; o[2 * G + g] = w.m2;
  }
}

// One wave per (sample, group): merges the group's Cg * parts partials of ws[n][part][3][Cw]
// (item i = channel i / parts of the group, part i % parts; lane l takes items l, l + 64, ... and
// the 64 lanes merge by butterfly) -> stats [mean(N*G) | rstd(N*G)]. The generic form passes
// Cw = G, Cg = 1.
__global__ __launch_bounds__(64) void gn_stats_finish(const float* __restrict__ ws, int Cw,
                                                      int Cg, int parts, int G, long NG,
                                                      float eps, float* __restrict__ stats) {
  const int ng = blockIdx.x, n = ng / G, g = ng - n * G;
  const int items = Cg * parts;
  Wf w{0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < items; i += 64) {
    const int ci = i / parts, p = i - ci * parts;
    const int c = g * Cg + ci;
    const float* o = ws + ((long)n * parts + p) * 3 * Cw;
    w = wf_merge(w, Wf{o[c], o[Cw + c], o[2 * Cw + c]});
  }
  w = wf_wave(w);
  if (threadIdx.x == 0) {
    stats[ng] = w.mean;
    stats[NG + ng] = rsqrtf((w.n > 0.f ? w.m2 / w.n : 0.f) + eps);
  }
}

// ----------------------------------------------------------------------------------- normalise
// x is centred before the multiply (as elemt_rows4): a constant group gives exactly its bias
__global__ __launch_bounds__(kT) void gn_elemt_nhwc(const float* __restrict__ x,
                                                    const float* __restrict__ stats,
                                                    const float* __restrict__ w,
                                                    const float* __restrict__ bb,
                                                    const float* __restrict__ res, int C, int HW,
                                                    int G, int Cg, long NG, GnRows L, int relu,
                                                    float* __restrict__ y,
                                                    uint8_t* __restrict__ mk) {
  const int bid = blockIdx.x;
  const int cb = bid % L.nblk, part = (bid / L.nblk) % L.parts, n = bid / (L.nblk * L.parts);
  const int t = threadIdx.x, cq = t % L.LPR, rg = t / L.LPR;
  const int c = cb * L.CB + 4 * cq;
  if (rg >= L.RPW || c >= C) return;
  const int b = part * L.P, e = b + L.P < HW ? b + L.P : HW;
  float sc[4], mn[4], sf[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long gi = (long)n * G + (c + j) / Cg;
    mn[j] = stats[gi];
    sc[j] = stats[NG + gi] * (w ? w[c + j] : 1.f);
    sf[j] = bb ? bb[c + j] : 0.f;
  }
  const long base = (long)n * HW * C + c;
#pragma unroll 4
  for (int r = b + rg; r < e; r += L.RPW) {
    const long off = base + (long)r * C;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + off);
    f32x4 q;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = fmaf(v[j] - mn[j], sc[j], sf[j]);
    if (res) q += *reinterpret_cast<const f32x4*>(res + off);
    f32x4 o = q;
    if (relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = fmaxf(q[j], 0.f);
    }
    *reinterpret_cast<f32x4*>(y + off) = o;
    // the ReLU gate for the backward, BatchNorm's format: one byte per 4 channels
    if (mk)
      mk[off >> 2] = (uint8_t)((q[0] > 0.f ? 1 : 0) | (q[1] > 0.f ? 2 : 0) |
                               (q[2] > 0.f ? 4 : 0) | (q[3] > 0.f ? 8 : 0));
  }
}

__global__ __launch_bounds__(kT) void gn_elemt_gen(const float* __restrict__ x,
                                                   const float* __restrict__ stats,
                                                   const float* __restrict__ w,
                                                   const float* __restrict__ bb,
                                                   const float* __restrict__ res, long total,
                                                   int C, int HW, int G, int Cg, long NG,
                                                   int relu, float* __restrict__ y) {
  for (long i = blockIdx.x * (long)kT + threadIdx.x; i < total; i += (long)gridDim.x * kT) {
    const long nc = i / HW;
    const long n = nc / C;
    const int c = (int)(nc - n * C);
    const long gi = n * G + c / Cg;
    float q = fmaf(x[i] - stats[gi], stats[NG + gi] * (w ? w[c] : 1.f), bb ? bb[c] : 0.f);
    if (res) q += res[i];
    y[i] = relu ? fmaxf(q, 0.f) : q;
  }
}

// ----------------------------------------------------------------------------- backward reduce
// NHWC: per-channel [sum g | sum g xhat] of one (sample, part) -> ws[n][part][2][C]
__global__ __launch_bounds__(kT) void gn_bwd_reduce_nhwc(const float* __restrict__ dy,
                                                         const float* __restrict__ x,
                                                         const float* __restrict__ stats,
                                                         const uint8_t* __restrict__ mk, int C,
                                                         int HW, int G, int Cg, long NG,
                                                         GnRows L, float* __restrict__ ws) {
  __shared__ float sh[2][1024];
  const int bid = blockIdx.x;
  const int cb = bid % L.nblk, part = (bid / L.nblk) % L.parts, n = bid / (L.nblk * L.parts);
  const int t = threadIdx.x, cq = t % L.LPR, rg = t / L.LPR;
  const int c = cb * L.CB + 4 * cq;
  const bool on = rg < L.RPW && c < C;
  const int b = part * L.P, e = b + L.P < HW ? b + L.P : HW;
  float a[4] = {0.f, 0.f, 0.f, 0.f}, m[4] = {0.f, 0.f, 0.f, 0.f};
  if (on) {
    float mn[4], rs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long gi = (long)n * G + (c + j) / Cg;
      mn[j] = stats[gi];
      rs[j] = stats[NG + gi];
    }
    const long base = (long)n * HW * C + c;
#pragma unroll 4
    for (int r = b + rg; r < e; r += L.RPW) {
      const long off = base + (long)r * C;
      f32x4 d = *reinterpret_cast<const f32x4*>(dy + off);
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + off);
      if (mk) {
        const uint32_t bits = mk[off >> 2];
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = ((bits >> j) & 1u) ? d[j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j] += d[j];
        m[j] = fmaf(d[j], (xv[j] - mn[j]) * rs[j], m[j]);
      }
    }
  }
  if (rg < L.RPW) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sh[0][rg * L.CB + 4 * cq + j] = a[j];
      sh[1][rg * L.CB + 4 * cq + j] = m[j];
    }
  }
  for (int st = pow2_ceil_gn(L.RPW) >> 1; st > 0; st >>= 1) {
    __syncthreads();
    for (int i = t; i < st * L.CB; i += kT) {
      if (i / L.CB + st < L.RPW) {
        sh[0][i] += sh[0][i + st * L.CB];
        sh[1][i] += sh[1][i + st * L.CB];
      }
    }
  }
  __syncthreads();
  float* o = ws + ((long)n * L.parts + part) * 2 * C;
  for (int k = t; k < L.CB; k += kT) {
    const int ch = cb * L.CB + k;
    if (ch >= C) continue;
    o[ch] = sh[0][k];
    o[C + ch] = sh[1][k];
  }
}

// generic: one wave per (sample, channel) -- its HW contiguous floats, lane-strided, then a
// butterfly sum -> ws[n][0][2][C] (one part). `yr`: the saved ReLU output (null = no ReLU).
__global__ __launch_bounds__(kT) void gn_bwd_reduce_gen(const float* __restrict__ dy,
                                                        const float* __restrict__ x,
                                                        const float* __restrict__ stats,
                                                        const float* __restrict__ yr, long NC,
                                                        int C, int HW, int G, int Cg, long NG,
                                                        float* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const long nc = blockIdx.x * (long)(kT / 64) + (threadIdx.x >> 6);
  if (nc >= NC) return;  // (whole waves leave: no barrier below)
  const long n = nc / C;
  const int c = (int)(nc - n * C);
  const long gi = n * G + c / Cg;
  const float mn = stats[gi], rs = stats[NG + gi];
  const long base = nc * HW;
  float a = 0.f, m = 0.f;
  for (int i = lane; i < HW; i += 64) {
    float d = dy[base + i];
    if (yr && !(yr[base + i] > 0.f)) d = 0.f;
    a += d;
    m = fmaf(d, (x[base + i] - mn) * rs, m);
  }
  a = wave_sum(a);
  m = wave_sum(m);
  if (lane == 0) {
    ws[n * 2 * C + c] = a;
    ws[n * 2 * C + C + c] = m;
  }
}

// One wave per (sample, group): A[n,c] = sum_parts, B[n,c] likewise (parts in index order) ->
// ab[n][2][C]; and the group's means of w g and w g xhat -> gs[ng][2]
__global__ __launch_bounds__(64) void gn_bwd_finish(const float* __restrict__ ws,
                                                    const float* __restrict__ w, int C, int Cg,
                                                    int parts, int G, float inv_cnt,
                                                    float* __restrict__ ab,
                                                    float* __restrict__ gs) {
  const int ng = blockIdx.x, n = ng / G, g = ng - n * G;
  float wa = 0.f, wb = 0.f;
  for (int ci = threadIdx.x; ci < Cg; ci += 64) {
    const int c = g * Cg + ci;
    float A = 0.f, B = 0.f;
    for (int p = 0; p < parts; ++p) {
      const float* o = ws + ((long)n * parts + p) * 2 * C;
      A += o[c];
      B += o[C + c];
    }
    ab[(long)n * 2 * C + c] = A;
    ab[(long)n * 2 * C + C + c] = B;
    const float wc = w ? w[c] : 1.f;
    wa = fmaf(wc, A, wa);
    wb = fmaf(wc, B, wb);
  }
  wa = wave_sum(wa);
  wb = wave_sum(wb);
  if (threadIdx.x == 0) {
    gs[2L * ng] = wa * inv_cnt;
    gs[2L * ng + 1] = wb * inv_cnt;
  }
}

// dw[c] = sum_n B[n,c], db[c] = sum_n A[n,c], n ascending
__global__ __launch_bounds__(kT) void gn_dwdb(const float* __restrict__ ab, int N, int C,
                                              float* __restrict__ dw, float* __restrict__ db) {
  const int c = blockIdx.x * kT + threadIdx.x;
  if (c >= C) return;
  float A = 0.f, B = 0.f;
  for (int n = 0; n < N; ++n) {
    A += ab[(long)n * 2 * C + c];
    B += ab[(long)n * 2 * C + C + c];
  }
  if (dw) dw[c] = B;
  if (db) db[c] = A;
}

// ------------------------------------------------------------------------ backward elementwise
__global__ __launch_bounds__(kT) void gn_bwd_elemt_nhwc(const float* __restrict__ dy,
                                                        const float* __restrict__ x,
                                                        const float* __restrict__ stats,
                                                        const float* __restrict__ w,
                                                        const float* __restrict__ gs,
                                                        const uint8_t* __restrict__ mk, int C,
                                                        int HW, int G, int Cg, long NG, GnRows L,
                                                        float* __restrict__ dx,
                                                        float* __restrict__ dres) {
  const int bid = blockIdx.x;
  const int cb = bid % L.nblk, part = (bid / L.nblk) % L.parts, n = bid / (L.nblk * L.parts);
  const int t = threadIdx.x, cq = t % L.LPR, rg = t / L.LPR;
  const int c = cb * L.CB + 4 * cq;
  if (rg >= L.RPW || c >= C) return;
  const int b = part * L.P, e = b + L.P < HW ? b + L.P : HW;
  float k1[4], k2[4], k3[4], mn[4], rs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long gi = (long)n * G + (c + j) / Cg;
    mn[j] = stats[gi];
    rs[j] = stats[NG + gi];
    k1[j] = rs[j] * (w ? w[c + j] : 1.f);
    k2[j] = -rs[j] * gs[2 * gi + 1];
    k3[j] = -rs[j] * gs[2 * gi];
  }
  const long base = (long)n * HW * C + c;
#pragma unroll 4
  for (int r = b + rg; r < e; r += L.RPW) {
    const long off = base + (long)r * C;
    f32x4 d = *reinterpret_cast<const f32x4*>(dy + off);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + off);
    if (mk) {
      const uint32_t bits = mk[off >> 2];
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = ((bits >> j) & 1u) ? d[j] : 0.f;
    }
    if (dx) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = fmaf(d[j], k1[j], fmaf((xv[j] - mn[j]) * rs[j], k2[j], k3[j]));
      *reinterpret_cast<f32x4*>(dx + off) = o;
    }
    // gradient of the fused residual input: the ReLU-masked dy itself
    if (dres) *reinterpret_cast<f32x4*>(dres + off) = d;
  }
}

__global__ __launch_bounds__(kT) void gn_bwd_elemt_gen(const float* __restrict__ dy,
                                                       const float* __restrict__ x,
                                                       const float* __restrict__ stats,
                                                       const float* __restrict__ w,
                                                       const float* __restrict__ gs,
                                                       const float* __restrict__ yr, long total,
                                                       int C, int HW, int G, int Cg, long NG,
                                                       float* __restrict__ dx,
                                                       float* __restrict__ dres) {
  for (long i = blockIdx.x * (long)kT + threadIdx.x; i < total; i += (long)gridDim.x * kT) {
    const long nc = i / HW;
    const long n = nc / C;
    const int c = (int)(nc - n * C);
    const long gi = n * G + c / Cg;
    const float mn = stats[gi], rs = stats[NG + gi];
    float d = dy[i];
    if (yr && !(yr[i] > 0.f)) d = 0.f;
    if (dx)
      dx[i] = fmaf(d, rs * (w ? w[c] : 1.f),
                   fmaf((x[i] - mn) * rs, -rs * gs[2 * gi + 1], -rs * gs[2 * gi]));
    if (dres) dres[i] = d;
  }
}

inline bool al16(std::initializer_list<const void*> ptrs) {
  for (const void* q : ptrs)
    if (q && ((uintptr_t)q & 15)) return false;
  return true;
}

inline int ew_grid_gn(long total) {
  long g = (total + kT - 1) / kT;
  if (g > 8192) g = 8192;
  return g < 1 ? 1 : (int)g;
}

inline void check_grid(long blocks) {
  if (blocks < 1 || blocks > 0x7fffffffL) throw std::runtime_error("group norm: grid too large");
}

}  // namespace

int gn_parts(int C, int HW, int G, bool nhwc) {
  if (nhwc) return gn_rows(C, HW).parts;
  const long run = (long)(C / G) * HW;
  return (int)((run + kRunPart - 1) / kRunPart);
}

long gn_ws_floats(int N, int C, int HW, int G, bool nhwc) {
  // forward partials [N][parts][3][C or G]; backward [N][parts or 1][2][C]
  const long parts = gn_parts(C, HW, G, nhwc);
  const long f = (long)N * parts * 3 * (nhwc ? C : G);
  const long b = (long)N * (nhwc ? parts : 1) * 2 * C;
  return f > b ? f : b;
}

void gn_fwd(const float* x, const float* w, const float* b, const float* residual, int N, int C,
            int HW, int G, bool nhwc, float eps, int relu, float* ws, float* stats, float* y,
            uint8_t* mask_out, hipStream_t s) {
  if (N < 1 || C < 1 || HW < 1 || G < 1 || C % G) throw std::runtime_error("gn_fwd: bad shape");
  const int Cg = C / G;
  const long NG = (long)N * G;
  check_grid(NG);
  if (nhwc) {
    if (C % 4 || !al16({x, y, residual}))
      throw std::runtime_error("gn_fwd: the NHWC form needs C % 4 == 0 and 16-byte alignment");
    const GnRows L = gn_rows(C, HW);
    const long blocks = (long)N * L.parts * L.nblk;
    check_grid(blocks);
    hipLaunchKernelGGL(gn_stats_nhwc, dim3((unsigned)blocks), dim3(kT), 0, s, x, C, HW, L, ws);
    hipLaunchKernelGGL(gn_stats_finish, dim3((unsigned)NG), dim3(64), 0, s, ws, C, Cg, L.parts,
                       G, NG, eps, stats);
    hipLaunchKernelGGL(gn_elemt_nhwc, dim3((unsigned)blocks), dim3(kT), 0, s, x, stats, w, b,
                       residual, C, HW, G, Cg, NG, L, relu, y, relu ? mask_out : nullptr);
    return;
  }
  if (mask_out) throw std::runtime_error("gn_fwd: a ReLU mask needs the NHWC form");
  const long run = (long)Cg * HW;
  const int parts = gn_parts(C, HW, G, false);
  check_grid(NG * parts);
  hipLaunchKernelGGL(gn_stats_gen, dim3((unsigned)(NG * parts)), dim3(kT), 0, s, x, run, G, parts,
                     ws);
  hipLaunchKernelGGL(gn_stats_finish, dim3((unsigned)NG), dim3(64), 0, s, ws, G, 1, parts, G, NG,
                     eps, stats);
  const long total = (long)N * C * HW;
  hipLaunchKernelGGL(gn_elemt_gen, dim3(ew_grid_gn(total)), dim3(kT), 0, s, x, stats, w, b,
                     residual, total, C, HW, G, Cg, NG, relu, y);
}

void gn_bwd(const float* dy, const float* x, const float* stats, const float* w,
            const float* y_relu, const uint8_t* mask, int N, int C, int HW, int G, bool nhwc,
            float* ws, float* ab, float* gs, float* dx, float* dres, float* dw, float* db,
            hipStream_t s) {
  if (N < 1 || C < 1 || HW < 1 || G < 1 || C % G) throw std::runtime_error("gn_bwd: bad shape");
  const int Cg = C / G;
  const long NG = (long)N * G;
  check_grid(NG);
  const float inv_cnt = (float)(1.0 / ((double)Cg * HW));
  if (nhwc) {
    if (C % 4 || !al16({dy, x, dx, dres}))
      throw std::runtime_error("gn_bwd: the NHWC form needs C % 4 == 0 and 16-byte alignment");
    if (y_relu) throw std::runtime_error("gn_bwd: the NHWC form reads the ReLU mask");
    const GnRows L = gn_rows(C, HW);
    const long blocks = (long)N * L.parts * L.nblk;
    check_grid(blocks);
    hipLaunchKernelGGL(gn_bwd_reduce_nhwc, dim3((unsigned)blocks), dim3(kT), 0, s, dy, x, stats,
                       mask, C, HW, G, Cg, NG, L, ws);
    hipLaunchKernelGGL(gn_bwd_finish, dim3((unsigned)NG), dim3(64), 0, s, ws, w, C, Cg, L.parts,
                       G, inv_cnt, ab, gs);
    if (dw || db)
      hipLaunchKernelGGL(gn_dwdb, dim3((C + kT - 1) / kT), dim3(kT), 0, s, ab, N, C, dw, db);
    if (dx || dres)
      hipLaunchKernelGGL(gn_bwd_elemt_nhwc, dim3((unsigned)blocks), dim3(kT), 0, s, dy, x, stats,
                         w, gs, mask, C, HW, G, Cg, NG, L, dx, dres);
    return;
  }
  if (mask) throw std::runtime_error("gn_bwd: a ReLU mask needs the NHWC form");
  const long NC = (long)N * C;
  const long rblocks = (NC + kT / 64 - 1) / (kT / 64);
  check_grid(rblocks);
  hipLaunchKernelGGL(gn_bwd_reduce_gen, dim3((unsigned)rblocks), dim3(kT), 0, s, dy, x, stats,
                     y_relu, NC, C, HW, G, Cg, NG, ws);
  hipLaunchKernelGGL(gn_bwd_finish, dim3((unsigned)NG), dim3(64), 0, s, ws, w, C, Cg, 1, G,
                     inv_cnt, ab, gs);
  if (dw || db)
    hipLaunchKernelGGL(gn_dwdb, dim3((C + kT - 1) / kT), dim3(kT), 0, s, ab, N, C, dw, db);
  if (dx || dres) {
    const long total = NC * HW;
    hipLaunchKernelGGL(gn_bwd_elemt_gen, dim3(ew_grid_gn(total)), dim3(kT), 0, s, dy, x, stats, w,
                       gs, y_relu, total, C, HW, G, Cg, NG, dx, dres);
  }
}

}  // namespace tdp
