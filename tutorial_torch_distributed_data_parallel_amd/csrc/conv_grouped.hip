// Grouped and depthwise 2-D convolution, NHWC, fp32 tensors in and out: forward, input gradient
// and weight gradient (declared in kernels.h, "Grouped / depthwise convolution").
//
// Arithmetic: plain fp32 FMA on the VALU, one rounding per accumulation step. At ResNeXt's
// Cg = Kg = 4 a 32-wide MFMA tile would span 8 groups and discard 7/8 of its products, and a
// depthwise stencil has no matrix shape at all, so neither family uses the matrix core. The
// weight operand is the parameter's own channels_last memory [Cout][R][S][Cg] in every pass.
//
// Grouped family (Cg % 4 == 0, Kg % 4 == 0):
//   gconv_kernel<false>   forward:        in = x,  out = y,  reduction over (r, s, c < Cg)
//   gconv_kernel<true>    input gradient: in = dy, out = dx, reduction over (r, s, k < Kg); the
//                         taps are gathered (transposed) from the same weight memory, and a tap
//                         that no output pixel reaches through the stride contributes nothing
//                         (a direct gather: a stride phase without taps is all zeros).
//   A 256-thread block computes 64 output pixels x 64 output channels; a thread owns 4 pixels x 4
//   channels. The block's weight slice is staged through LDS 16 reduction steps at a time, laid
//   out so that a wave's 16-B reads are contiguous (no bank conflict); the input is read with
//   16-B loads of 4 channels of one pixel.
//   gconv_wgrad_kernel    weight gradient: a thread owns a 4 (Cout) x 4 (Cg) block of one tap and
//                         walks a contiguous range of the N*P*Q pixels; ranges (splits) write
//                         partials that splitk_reduce combines in a fixed order.
// Depthwise family (Cg == 1, Cout = m * Cin, Cin % 4 == 0): a bandwidth-bound stencil.
//   dwconv_kernel<DGRAD, R, S>  16-B loads along C, the R x S taps of the thread's 4 channels
//                         held in registers (3x3 and 5x5 with m == 1); any other filter size or a
//                         channel multiplier m > 1 takes the <.., 0, 0> form, which reads taps
//                         and the m-strided channels from memory.
//                         dwconv_kernel<false, R, S, true> (register-tap forward) also emits the
//                         output's BatchNorm statistics: one (count, mean, M2) partial per
//                         (block, channel), reduced in LDS in a fixed order.
//   dwconv_wgrad_kernel   a thread owns one tap of 4 output channels over a pixel range.
// No pass uses atomics: every result is bitwise reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>

#include "kernels.h"

namespace tdp {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kOQB = 16;  // output-channel quads per block (64 channels)
constexpr int kKC = 16;   // reduction steps (one tap x 4 input channels each) per LDS stage
constexpr int kTQ = 4;    // output pixels per thread
constexpr int kPT = 256 / kOQB;  // pixel threads per block

// One pass of the grouped family as "out = conv(in)": for the forward in = x, out = y; for the
// input gradient in = dy, out = dx. icg / ocg: channels per group of in / out.
struct GcArgs {
  int N, IH, IW, IC, OH, OW, OC, R, S, sh, sw, ph, pw, icg, ocg;
};

// input row / column of output coordinate o for tap t; false when the tap does not reach it
template <bool DGRAD>
__device__ __forceinline__ bool tap_coord(int o, int t, int stride, int pad, int extent, int& i) {
  if (!DGRAD) {
    i = o * stride - pad + t;
    return i >= 0 && i < extent;
  }
  const int d = o + pad - t;
  if (d < 0) return false;
  i = d / stride;
  return i * stride == d && i < extent;
}

template <bool DGRAD>
__global__ __launch_bounds__(256) void gconv_kernel(GcArgs a, const float* __restrict__ in,
                                                    const float* __restrict__ w,
                                                    const float* __restrict__ bias,
                                                    float* __restrict__ out, int relu,
                                                    int accumulate) {
  __shared__ f32x4 wl[kKC][4][kOQB];
  const int tid = threadIdx.x, oql = tid % kOQB, pt = tid / kOQB;
  const int oq = blockIdx.y * kOQB + oql;
  const bool oq_ok = oq < a.OC / 4;
  const int I4 = a.icg / 4, RS = a.R * a.S;
  const int KT = RS * I4;
  const int grp = oq_ok ? (4 * oq) / a.ocg : 0;
  const int in_c0 = grp * a.icg;
  const long Mout = (long)a.N * a.OH * a.OW;
  const long m0 = ((long)blockIdx.x * kPT + pt) * kTQ;
  int pn[kTQ], poh[kTQ], pow_[kTQ];
  bool pv[kTQ];
#pragma unroll
  for (int t = 0; t < kTQ; ++t) {
    const long m = m0 + t;
    pv[t] = oq_ok && m < Mout;
    const long mm = pv[t] ? m : 0;
    pow_[t] = (int)(mm % a.OW);
    poh[t] = (int)((mm / a.OW) % a.OH);
    pn[t] = (int)(mm / ((long)a.OW * a.OH));
  }
  f32x4 acc[kTQ];
#pragma unroll
  for (int t = 0; t < kTQ; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < KT; k0 += kKC) {
    __syncthreads();  // the previous stage has been read
    {
      const int kl = pt, kk = k0 + kl;
      f32x4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (oq_ok && kk < KT) {
        const int tap = kk / I4, i4 = kk - tap * I4;
        if (!DGRAD) {
          // w[co = 4 oq + j][tap][4 i4 ..]: Cg = icg
#pragma unroll
          for (int j = 0; j < 4; ++j)
            v[j] = *reinterpret_cast<const f32x4*>(
                w + ((long)(4 * oq + j) * RS + tap) * a.icg + 4 * i4);
        } else {
          // w[co = grp Kg + 4 i4 + ii][tap][c = 4 oq + j - grp Cg], transposed: Cg = ocg, Kg = icg
          const int cl = 4 * oq - grp * a.ocg;
          f32x4 rw[4];
#pragma unroll
          for (int ii = 0; ii < 4; ++ii)
            rw[ii] = *reinterpret_cast<const f32x4*>(
                w + ((long)(in_c0 + 4 * i4 + ii) * RS + tap) * a.ocg + cl);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = f32x4{rw[0][j], rw[1][j], rw[2][j], rw[3][j]};
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) wl[kl][j][oql] = v[j];
    }
    __syncthreads();
    const int kend = min(kKC, KT - k0);
    int tap = k0 / I4, i4 = k0 - tap * I4;
    int r = tap / a.S, s = tap - r * a.S;
    for (int kl = 0; kl < kend; ++kl) {
      f32x4 xv[kTQ];
#pragma unroll
      for (int t = 0; t < kTQ; ++t) {
        int ih = 0, iw = 0;
        const bool ok = pv[t] & tap_coord<DGRAD>(poh[t], r, a.sh, a.ph, a.IH, ih) &
                        tap_coord<DGRAD>(pow_[t], s, a.sw, a.pw, a.IW, iw);
        xv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ok)
          xv[t] = *reinterpret_cast<const f32x4*>(
              in + (((long)pn[t] * a.IH + ih) * a.IW + iw) * a.IC + in_c0 + 4 * i4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 wv = wl[kl][j][oql];
#pragma unroll
        for (int t = 0; t < kTQ; ++t) {
          float c = acc[t][j];
          c = __builtin_fmaf(xv[t][0], wv[0], c);
          c = __builtin_fmaf(xv[t][1], wv[1], c);
          c = __builtin_fmaf(xv[t][2], wv[2], c);
          c = __builtin_fmaf(xv[t][3], wv[3], c);
          acc[t][j] = c;
        }
      }
      if (++i4 == I4) {
        i4 = 0;
        if (++s == a.S) { s = 0; ++r; }
      }
    }
  }

  f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
  if (bias != nullptr && oq_ok) bv = *reinterpret_cast<const f32x4*>(bias + 4 * oq);
#pragma unroll
  for (int t = 0; t < kTQ; ++t) {
    if (!pv[t]) continue;
    f32x4* dst = reinterpret_cast<f32x4*>(out + (m0 + t) * a.OC + 4 * oq);
    f32x4 o = acc[t] + bv;
    if (accumulate) o += *dst;
    if (relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = o[j] > 0.f ? o[j] : 0.f;
    }
    *dst = o;
  }
}

// Weight-gradient geometry shared by both families.
struct WgArgs {
  int N, H, W, C, P, Q, Cout, R, S, sh, sw, ph, pw, Cg, Kg;
  long M;             // N * P * Q
  int k_per_split;    // pixels per split
  long total;         // Cout * R * S * Cg (one partial)
};

// Thread = (tap, co quad, c quad) over the split's pixel range; dst = dw (one split) or the
// split's partial. acc[j][i] = sum_m dy[m][4 cq + j] * x[m @ tap][grp Cg + 4 c4 + i].
__global__ __launch_bounds__(64) void gconv_wgrad_kernel(WgArgs a, const float* __restrict__ dy,
                                                         const float* __restrict__ x,
                                                         float* __restrict__ dst) {
  const int I4 = a.Cg / 4, OQ = a.Cout / 4, RS = a.R * a.S;
  const long U = (long)RS * OQ * I4;
  const long u = (long)blockIdx.x * 64 + threadIdx.x;
  if (u >= U) return;
  const int c4 = (int)(u % I4);
  const int cq = (int)((u / I4) % OQ);
  const int tap = (int)(u / ((long)I4 * OQ));
  const int r = tap / a.S, s = tap - r * a.S;
  const int grp = (4 * cq) / a.Kg;
  const long mb = (long)blockIdx.y * a.k_per_split;
  const long me = min(a.M, mb + a.k_per_split);
  int q = (int)(mb % a.Q), p = (int)((mb / a.Q) % a.P), n = (int)(mb / ((long)a.Q * a.P));
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* dyp = dy + 4 * cq;
  const float* xp = x + grp * a.Cg + 4 * c4;
  for (long m = mb; m < me; ++m) {
    const int ih = p * a.sh - a.ph + r, iw = q * a.sw - a.pw + s;
    if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(dyp + m * a.Cout);
      const f32x4 xv =
          *reinterpret_cast<const f32x4*>(xp + (((long)n * a.H + ih) * a.W + iw) * a.C);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = __builtin_fmaf(g[j], xv[i], acc[j][i]);
      }
    }
    if (++q == a.Q) {
      q = 0;
      if (++p == a.P) { p = 0; ++n; }
    }
  }
  float* o = dst + (long)blockIdx.y * a.total;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    *reinterpret_cast<f32x4*>(o + ((long)(4 * cq + j) * RS + tap) * a.Cg + 4 * c4) = acc[j];
}

// ------------------------------------------------------------------------------------- depthwise
// "out = stencil(in)" with 4 output channels per thread. Forward: in = x (IC = Cin), out = y
// (OC = Cout), output channel o reads input channel o / mult. Input gradient: in = dy
// (IC = Cout), out = dx (OC = Cin), output channel c sums input channels c mult + jj, jj < mult.
struct DwArgs {
  int N, IH, IW, IC, OH, OW, OC, R, S, sh, sw, ph, pw, mult;
};
constexpr int kDwPix = 8;  // consecutive output pixels per thread (the taps are loaded once)

// STATS (forward, register taps, no bias / ReLU): the block also writes the BatchNorm statistics
// of the outputs it produced, part[blockIdx.x][3][OC] = (count, mean, M2) per channel -- the
// [T][3][C] partials bn_moments_partials merges (norm.hip moments_partials_l1). A thread sums its
// <= 8 pixels shifted by its first pixel's value (s1 = sum (v - K), s2 = sum (v - K)^2: mean =
// K + s1 / n, M2 = s2 - s1^2 / n, the shifted-sum form of the GEMM epilogue's statistics); the
// block's threads of one channel quad are then Chan-merged through LDS in ascending thread
// order. No atomics, and the partition depends on the geometry alone: bitwise reproducible. A
// channel no thread of the block covers gets count 0.
template <bool DGRAD, int R_, int S_, bool STATS = false>
__global__ __launch_bounds__(256) void dwconv_kernel(DwArgs a, const float* __restrict__ in,
                                                     const float* __restrict__ w,
                                                     const float* __restrict__ bias,
                                                     float* __restrict__ out, int relu,
                                                     int accumulate,
                                                     float* __restrict__ part = nullptr) {
  static_assert(!STATS || (!DGRAD && R_ > 0), "statistics: register-tap forward only");
  const int OQ = a.OC / 4;
  const long Mout = (long)a.N * a.OH * a.OW;
  const long item = (long)blockIdx.x * 256 + threadIdx.x;
  const int oq = (int)(item % OQ);
  const long mb = (item / OQ) * kDwPix;
  if (!STATS && mb >= Mout) return;  // (with STATS every thread reaches the block reduction)
  const int RS = a.R * a.S;
  f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
  if (bias != nullptr) bv = *reinterpret_cast<const f32x4*>(bias + 4 * oq);

  constexpr bool kRegs = R_ > 0;  // mult == 1, R x S = R_ x S_: taps in registers
  constexpr int kTaps = kRegs ? R_ * S_ : 1;
  f32x4 wr[kTaps];
  if (kRegs) {
#pragma unroll
    for (int t = 0; t < kTaps; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) wr[t][j] = w[(long)(4 * oq + j) * kTaps + t];
  }

  const long me = min(Mout, mb + kDwPix);
  f32x4 sk = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = sk, s2 = sk;  // STATS: shift, shifted sums
  for (long m = mb; m < me; ++m) {
    const int ow = (int)(m % a.OW), oh = (int)((m / a.OW) % a.OH);
    const int n = (int)(m / ((long)a.OW * a.OH));
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if (kRegs) {
#pragma unroll
      for (int r = 0; r < (kRegs ? R_ : 1); ++r) {
        int ih = 0;
        const bool rok = tap_coord<DGRAD>(oh, r, a.sh, a.ph, a.IH, ih);
#pragma unroll
        for (int s = 0; s < (kRegs ? S_ : 1); ++s) {
          int iw = 0;
          if (rok & tap_coord<DGRAD>(ow, s, a.sw, a.pw, a.IW, iw)) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(
                in + (((long)n * a.IH + ih) * a.IW + iw) * a.IC + 4 * oq);
            const f32x4 wv = wr[r * (kRegs ? S_ : 1) + s];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(xv[j], wv[j], acc[j]);
          }
        }
      }
    } else {
      const int nin = DGRAD ? a.mult : 1;
      for (int r = 0; r < a.R; ++r) {
        int ih = 0;
        if (!tap_coord<DGRAD>(oh, r, a.sh, a.ph, a.IH, ih)) continue;
        for (int s = 0; s < a.S; ++s) {
          int iw = 0;
          if (!tap_coord<DGRAD>(ow, s, a.sw, a.pw, a.IW, iw)) continue;
          const float* ip = in + (((long)n * a.IH + ih) * a.IW + iw) * a.IC;
          const int tap = r * a.S + s;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int o = 4 * oq + j;
            const int ibase = DGRAD ? o * a.mult : o / a.mult;
            for (int jj = 0; jj < nin; ++jj) {
              const int ich = ibase + jj;
              const int wch = DGRAD ? ich : o;
              acc[j] = __builtin_fmaf(ip[ich], w[(long)wch * RS + tap], acc[j]);
            }
          }
        }
      }
    }
    f32x4* dst = reinterpret_cast<f32x4*>(out + m * a.OC + 4 * oq);
    f32x4 o = acc + bv;
    if (accumulate) o += *dst;
    if (relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = o[j] > 0.f ? o[j] : 0.f;
    }
    *dst = o;
    if constexpr (STATS) {
      if (m == mb) sk = o;
      const f32x4 d = o - sk;
      s1 += d;
      s2 += d * d;
    }
  }
  if constexpr (STATS) {
    __shared__ float sn[256];
    __shared__ float sm[2][4][256];  // mean | M2, per channel of the quad, per thread
    const float n = me > mb ? (float)(me - mb) : 0.f;
    sn[threadIdx.x] = n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float mu = n > 0.f ? s1[j] / n : 0.f;
      const float m2 = n > 0.f ? s2[j] - s1[j] * mu : 0.f;
      sm[0][j][threadIdx.x] = sk[j] + mu;
      sm[1][j][threadIdx.x] = m2 > 0.f ? m2 : 0.f;
    }
    __syncthreads();
    // thread t of this block holds quad (base + t) % OQ
    const int base = (int)(((long)blockIdx.x * 256) % OQ);
    float* po = part + (long)blockIdx.x * 3 * a.OC;
    for (int q = threadIdx.x; q < OQ; q += 256) {
      const int t0 = ((q - base) % OQ + OQ) % OQ;
      float cn = 0.f, cm[4] = {0.f, 0.f, 0.f, 0.f}, c2[4] = {0.f, 0.f, 0.f, 0.f};
      for (int t = t0; t < 256; t += OQ) {
        const float bn = sn[t];
        if (bn == 0.f) continue;
        const float tot = cn + bn, fb = bn / tot;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float dd = sm[0][j][t] - cm[j];
          c2[j] = c2[j] + sm[1][j][t] + dd * dd * cn * fb;
          cm[j] = __builtin_fmaf(dd, fb, cm[j]);
        }
        cn = tot;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        po[4 * q + j] = cn;
        po[a.OC + 4 * q + j] = cm[j];
        po[2 * a.OC + 4 * q + j] = c2[j];
      }
    }
  }
}

// Thread = (tap, co quad) over the split's pixel range: acc[j] = sum_m dy[m][4 cq + j] *
// x[m @ tap][(4 cq + j) / mult]; dst[(4 cq + j) * R * S + tap].
__global__ __launch_bounds__(64) void dwconv_wgrad_kernel(WgArgs a, int mult,
                                                          const float* __restrict__ dy,
                                                          const float* __restrict__ x,
                                                          float* __restrict__ dst) {
  const int OQ = a.Cout / 4, RS = a.R * a.S;
  const long U = (long)RS * OQ;
  const long u = (long)blockIdx.x * 64 + threadIdx.x;
  if (u >= U) return;
  const int cq = (int)(u % OQ);
  const int tap = (int)(u / OQ);
  const int r = tap / a.S, s = tap - r * a.S;
  const long mb = (long)blockIdx.y * a.k_per_split;
  const long me = min(a.M, mb + a.k_per_split);
  int q = (int)(mb % a.Q), p = (int)((mb / a.Q) % a.P), n = (int)(mb / ((long)a.Q * a.P));
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* dyp = dy + 4 * cq;
  for (long m = mb; m < me; ++m) {
    const int ih = p * a.sh - a.ph + r, iw = q * a.sw - a.pw + s;
    if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(dyp + m * a.Cout);
      const float* xp = x + (((long)n * a.H + ih) * a.W + iw) * a.C;
      f32x4 xv;
      if (mult == 1) {
        xv = *reinterpret_cast<const f32x4*>(xp + 4 * cq);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = xp[(4 * cq + j) / mult];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(g[j], xv[j], acc[j]);
    }
    if (++q == a.Q) {
      q = 0;
      if (++p == a.P) { p = 0; ++n; }
    }
  }
  float* o = dst + (long)blockIdx.y * a.total;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[(long)(4 * cq + j) * RS + tap] = acc[j];
}

int out_extent(int in, int k, int stride, int pad) { return (in + 2 * pad - k) / stride + 1; }

long dw_blocks(const DwArgs& a) {
  const long items = (long)(a.OC / 4) * (((long)a.N * a.OH * a.OW + kDwPix - 1) / kDwPix);
  return (items + 255) / 256;
}

bool dw_stats_form(const DwArgs& a) {
  return a.mult == 1 && ((a.R == 3 && a.S == 3) || (a.R == 5 && a.S == 5));
}

template <bool DGRAD>
void dw_launch(const DwArgs& a, const float* in, const float* w, const float* bias, float* out,
               bool relu, bool accumulate, hipStream_t s, float* part = nullptr) {
  const dim3 grid((unsigned)dw_blocks(a));
  const int rl = relu ? 1 : 0, ac = accumulate ? 1 : 0;
  if constexpr (!DGRAD) {
    if (part != nullptr) {  // statistics epilogue: its own instantiation, same output
      if (a.R == 3)
        hipLaunchKernelGGL((dwconv_kernel<false, 3, 3, true>), grid, dim3(256), 0, s, a, in, w,
                           bias, out, rl, ac, part);
      else
        hipLaunchKernelGGL((dwconv_kernel<false, 5, 5, true>), grid, dim3(256), 0, s, a, in, w,
                           bias, out, rl, ac, part);
      return;
    }
  }
  if (a.mult == 1 && a.R == 3 && a.S == 3)
    hipLaunchKernelGGL((dwconv_kernel<DGRAD, 3, 3>), grid, dim3(256), 0, s, a, in, w, bias, out,
                       rl, ac);
  else if (a.mult == 1 && a.R == 5 && a.S == 5)
    hipLaunchKernelGGL((dwconv_kernel<DGRAD, 5, 5>), grid, dim3(256), 0, s, a, in, w, bias, out,
                       rl, ac);
  else
    hipLaunchKernelGGL((dwconv_kernel<DGRAD, 0, 0>), grid, dim3(256), 0, s, a, in, w, bias, out,
                       rl, ac);
}

template <bool DGRAD>
void gc_launch(const GcArgs& a, const float* in, const float* w, const float* bias, float* out,
               bool relu, bool accumulate, hipStream_t s) {
  const long Mout = (long)a.N * a.OH * a.OW;
  const dim3 grid((unsigned)((Mout + kPT * kTQ - 1) / (kPT * kTQ)),
                  (unsigned)((a.OC / 4 + kOQB - 1) / kOQB));
  hipLaunchKernelGGL(gconv_kernel<DGRAD>, grid, dim3(256), 0, s, a, in, w, bias, out,
                     relu ? 1 : 0, accumulate ? 1 : 0);
}

}  // namespace

int conv_group_family(const GroupConvGeom& g) {
  if (g.groups <= 1 || g.C % g.groups != 0 || g.Cout % g.groups != 0) return kGroupNone;
  const int Cg = g.C / g.groups, Kg = g.Cout / g.groups;
  if (Cg == 1) return g.C % 4 == 0 ? kGroupDepthwise : kGroupNone;
  return (Cg % 4 == 0 && Kg % 4 == 0) ? kGroupGrouped : kGroupNone;
}

int conv_dw_stats_tiles(const GroupConvGeom& g) {
  if (conv_group_family(g) != kGroupDepthwise) return 0;
  const int P = out_extent(g.H, g.R, g.sh, g.ph), Q = out_extent(g.W, g.S, g.sw, g.pw);
  const DwArgs a{g.N, g.H, g.W, g.C, P, Q, g.Cout, g.R, g.S, g.sh, g.sw, g.ph, g.pw,
                 g.Cout / g.C};
  return dw_stats_form(a) ? (int)dw_blocks(a) : 0;
}

void conv_grouped_fwd(const GroupConvGeom& g, const float* x, const float* w, const float* bias,
                      bool relu, float* y, hipStream_t s, float* stats_part) {
  const int P = out_extent(g.H, g.R, g.sh, g.ph), Q = out_extent(g.W, g.S, g.sw, g.pw);
  if (stats_part != nullptr && (conv_dw_stats_tiles(g) == 0 || bias != nullptr || relu))
    throw std::runtime_error("conv_grouped_fwd: statistics need the register-tap depthwise "
                             "forward (3x3 / 5x5, multiplier 1) without bias or ReLU");
  if (conv_group_family(g) == kGroupDepthwise) {
    const DwArgs a{g.N, g.H, g.W, g.C, P, Q, g.Cout, g.R, g.S, g.sh, g.sw, g.ph, g.pw,
                   g.Cout / g.C};
    dw_launch<false>(a, x, w, bias, y, relu, false, s, stats_part);
  } else {
    const GcArgs a{g.N, g.H, g.W, g.C, P, Q, g.Cout, g.R, g.S, g.sh, g.sw, g.ph, g.pw,
                   g.C / g.groups, g.Cout / g.groups};
    gc_launch<false>(a, x, w, bias, y, relu, false, s);
  }
}

void conv_grouped_dgrad(const GroupConvGeom& g, const float* dy, const float* w, float* dx,
                        bool accumulate, hipStream_t s) {
  const int P = out_extent(g.H, g.R, g.sh, g.ph), Q = out_extent(g.W, g.S, g.sw, g.pw);
  if (conv_group_family(g) == kGroupDepthwise) {
    const DwArgs a{g.N, P, Q, g.Cout, g.H, g.W, g.C, g.R, g.S, g.sh, g.sw, g.ph, g.pw,
                   g.Cout / g.C};
    dw_launch<true>(a, dy, w, nullptr, dx, false, accumulate, s);
  } else {
    const GcArgs a{g.N, P, Q, g.Cout, g.H, g.W, g.C, g.R, g.S, g.sh, g.sw, g.ph, g.pw,
                   g.Cout / g.groups, g.C / g.groups};
    gc_launch<true>(a, dy, w, nullptr, dx, false, accumulate, s);
  }
}

GroupConvPlan conv_grouped_wgrad_plan(const GroupConvGeom& g, int num_cus) {
  const int P = out_extent(g.H, g.R, g.sh, g.ph), Q = out_extent(g.W, g.S, g.sw, g.pw);
  const long M = (long)g.N * P * Q;
  const int Cg = g.C / g.groups;
  const long total = (long)g.Cout * g.R * g.S * Cg;
  const long units = total / (Cg == 1 ? 4 : 16);
  const long blocks = (units + 63) / 64;
  // 16 waves per CU over the whole launch, at least 64 pixels per split, and a workspace of at
  // most 64 Mi floats
  long splits = (16L * num_cus + blocks - 1) / blocks;
  splits = std::min(splits, (M + 63) / 64);
  splits = std::min(splits, std::max(1L, (64L << 20) / total));
  splits = std::max(splits, 1L);
  GroupConvPlan pl;
  pl.k_per_split = (int)((M + splits - 1) / splits);
  pl.splits = (int)((M + pl.k_per_split - 1) / pl.k_per_split);
  pl.ws_floats = pl.splits > 1 ? (long)pl.splits * total : 0;
  return pl;
}

void conv_grouped_wgrad(const GroupConvGeom& g, const GroupConvPlan& pl, const float* dy,
                        const float* x, float* dw, float* ws, hipStream_t s) {
  const int P = out_extent(g.H, g.R, g.sh, g.ph), Q = out_extent(g.W, g.S, g.sw, g.pw);
  const int Cg = g.C / g.groups, Kg = g.Cout / g.groups;
  WgArgs a{g.N, g.H, g.W, g.C, P, Q, g.Cout, g.R, g.S, g.sh, g.sw, g.ph, g.pw, Cg, Kg,
           (long)g.N * P * Q, pl.k_per_split, (long)g.Cout * g.R * g.S * Cg};
  float* dst = pl.splits > 1 ? ws : dw;
  const bool dwise = conv_group_family(g) == kGroupDepthwise;
  const long units = a.total / (dwise ? 4 : 16);
  const dim3 grid((unsigned)((units + 63) / 64), (unsigned)pl.splits);
  if (dwise)
    hipLaunchKernelGGL(dwconv_wgrad_kernel, grid, dim3(64), 0, s, a, g.Cout / g.C, dy, x, dst);
  else
    hipLaunchKernelGGL(gconv_wgrad_kernel, grid, dim3(64), 0, s, a, dy, x, dst);
  // partials combined in a fixed order (the tree of splitk_reduce): no atomics
  if (pl.splits > 1)
    splitk_reduce(ws, pl.splits, 1, (int)a.total, dw, false, a.total, nullptr, 0.f, false, s);
}

}  // namespace tdp
