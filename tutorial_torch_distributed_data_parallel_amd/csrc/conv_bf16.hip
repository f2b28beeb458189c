// Mixed-precision NHWC implicit-GEMM convolution (gfx950): the autocast path of ops/conv.py.
//
// gemm_bf16's tile (bf16_tile.h: 128 x 128 x 64, 2 x 2 waves, fp32 operands global -> registers ->
// packed RNE convert -> swizzled bf16 LDS -> one v_mfma_f32_32x32x16_bf16 per K16 step, fp32
// accumulation, bias / beta / ReLU epilogue, fixed-order split-K combine) with implicit operand
// sources in the register stage. Tensors stay fp32 in memory; every operand element is rounded
// once to bf16 per pass. Only the loaders below are new: they fill the same register images as
// the dense loader, with the address computed per 16-byte load (4 consecutive channels of one
// pixel or filter tap; C % 4 == 0 and Cout % 4 == 0).
//   FWD  : C = y [N*P*Q][Cout]; A = RowsSrc over x (rows = output pixels, k = (r, s, c));
//          B = the weight's [Cout][R*S*C] storage (dense, K tail zero-filled)
//   DGRAD: stride-1 geometry (a strided gradient arrives as stride-1 phases). C = dx [N*H*W][C];
//          A = RowsSrc over dy (rows = dx pixels, k = (tap, co)); B = WTapSrc, gathered from the
//          weight parameter's [Cout][Rf][Sf][C] memory
//   WGRAD: C = dWt [Cout][R*S*C]; A = g [N*P*Q][Cout] (dense, MN-contiguous); B = ColsSrc over x
//          (k = dy pixel, columns = (r, s, c)); split-K over N*P*Q
// Padding taps, k past the split's end and the K tail read a valid address (the tensor's start)
// and select zero: no pointer is formed from an out-of-range (h, w). Rows / columns past the
// matrix are clamped and their outputs discarded. Decompositions that do not change over the K
// loop (A's pixel -> (n, y, x), the weight gradient's column -> tap) are computed once per
// workgroup; when the gathered tensor's channel count is a multiple of 64 a K tile is one tap
// and its decomposition is wave-uniform.
#include <stdexcept>

#include "bf16_tile.h"
#include "common.h"
#include "conv.h"

namespace tdp {
using namespace bf16t;
namespace {

// geometry of an implicit operand: the NHWC tensor being gathered ("source") and the pixel grid
// that GEMM rows (RowsSrc) or GEMM k (ColsSrc) walk over
struct CvGeom {
  int Hs, Ws, Cs;       // source tensor dims
  int S, sh, sw, ph, pw;
  int grid_p, grid_q;   // grid rows / pixels per row
  int uniform;          // Cs % 64 == 0: one filter tap per K tile
  FastDiv dC, dS, dPQ, dQ;
};

// input-gradient B in the weight's own [Cout][Rf][Sf][C] storage: row k = (tap, co), co fastest;
// tap walks the phase's Rp x Sp sub-grid of filter taps (r, s) = (r0 + rp*sh, s0 + sp*sw)
struct WTapGeom {
  int Cout, Sp, r0, s0, sh, sw, Sf, C;
  int rs;       // weight row stride Rf*Sf*C
  int uniform;  // Cout % 64 == 0: one tap per K tile
  FastDiv dCout, dSp;
};

struct CParams {
  BParams g;
  CvGeom cv;
  WTapGeom wt;
};

__device__ __forceinline__ f32x4 sel4(bool ok, f32x4 a) {
  return ok ? a : f32x4{0.f, 0.f, 0.f, 0.f};
}

// Implicit K-contiguous A: rows are pixels of the grid, k = (r, s, c) with c fastest.
//   FWD   : source x,  row (n, p, q) reads x[n][p*sh - ph + r][q*sw - pw + s][c]
//   DGRAD : source dy, row (n, h, w) of dx reads dy[n][h + ph - r][w + pw - s][c] (stride 1)
// A thread's four units share one chunk (8 k = two 4-channel halves, decomposed per half: with
// Cs % 8 == 4 the halves are different taps) and differ in the row, decomposed once.
template <bool DGRAD>
struct RowsSrc {
  static constexpr bool kKC = true;
  const float* src;
  const CvGeom* cv;
  int base[4], hb[4], wb[4];

  __device__ __forceinline__ void init(const float* P, const CvGeom& c, int r0, int rlim) {
    src = P;
    cv = &c;
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int gr = r0 + i * 32 + (t >> 3);
      gr = gr < rlim ? gr : rlim - 1;  // clamped: the row's outputs are discarded
      const uint32_t n = fdiv(gr, c.dPQ);
      const uint32_t pq = gr - n * (c.grid_p * c.grid_q);
      const uint32_t y = fdiv(pq, c.dQ);
      const uint32_t x = pq - y * c.grid_q;
      base[i] = (int)n * c.Hs * c.Ws * c.Cs;
      hb[i] = DGRAD ? (int)y + c.ph : (int)y * c.sh - c.ph;
      wb[i] = DGRAD ? (int)x + c.pw : (int)x * c.sw - c.pw;
    }
  }

  __device__ __forceinline__ void load(int k0, int ke, float (&v)[32]) const {
    const CvGeom& c = *cv;
    const int c8 = (threadIdx.x & 7) * 8;
    int ur = 0, us = 0, uc = 0;
    if (c.uniform) {  // k0 is wave-uniform and the whole tile is one tap
      const uint32_t rs = fdiv(k0, c.dC);
      uc = k0 - rs * c.Cs;
      ur = fdiv(rs, c.dS);
      us = rs - ur * c.S;
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int k = k0 + c8 + hf * 4;
      int r, s, cc;
      if (c.uniform) {
        r = ur; s = us; cc = uc + c8 + hf * 4;
      } else {
        const uint32_t rs = fdiv(k, c.dC);
        cc = k - rs * c.Cs;
        r = fdiv(rs, c.dS);
        s = rs - r * c.S;
      }
      const bool kok = k < ke;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int h = DGRAD ? hb[i] - r : hb[i] + r;
        const int w = DGRAD ? wb[i] - s : wb[i] + s;
        const bool ok = kok && (unsigned)h < (unsigned)c.Hs && (unsigned)w < (unsigned)c.Ws;
        const int off = ok ? base[i] + (h * c.Ws + w) * c.Cs + cc : 0;
        const f32x4 a = sel4(ok, ld4(src + off));
#pragma unroll
        for (int e = 0; e < 4; ++e) v[8 * i + 4 * hf + e] = a[e];
      }
    }
  }
};

// Implicit MN-contiguous B of the weight gradient: k = dy pixel (n, p, q), columns (r, s, c)
// with c fastest; element = x[n][p*sh - ph + r][q*sw - pw + s][c]. A thread's 4 columns are one
// tap (Cs % 4 == 0), fixed for the whole kernel; its 8 k are consecutive pixels: the first is
// decomposed, the others step through the grid.
struct ColsSrc {
  static constexpr bool kKC = false;
  const float* src;
  const CvGeom* cv;
  int th, tw, coff;

  __device__ __forceinline__ void init(const float* P, const CvGeom& c, int r0, int rlim) {
    src = P;
    cv = &c;
    int gc = r0 + (threadIdx.x >> 3) * 4;
    gc = gc < rlim ? gc : rlim - 4;  // clamped: the columns' outputs are discarded
    const uint32_t rs = fdiv(gc, c.dC);
    coff = gc - rs * c.Cs;
    const int r = fdiv(rs, c.dS);
    const int s = rs - r * c.S;
    th = r - c.ph;
    tw = s - c.pw;
  }

  __device__ __forceinline__ void load(int k0, int ke, float (&v)[32]) const {
    const CvGeom& c = *cv;
    const int kf = k0 + (threadIdx.x & 7) * 8;
    int n = fdiv(kf, c.dPQ);
    const int pq = kf - n * (c.grid_p * c.grid_q);
    int y = fdiv(pq, c.dQ);
    int x = pq - y * c.grid_q;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int h = y * c.sh + th, w = x * c.sw + tw;
      const bool ok = kf + kk < ke && (unsigned)h < (unsigned)c.Hs && (unsigned)w < (unsigned)c.Ws;
      const int off = ok ? ((n * c.Hs + h) * c.Ws + w) * c.Cs + coff : 0;
      const f32x4 a = sel4(ok, ld4(src + off));
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * kk + j] = a[j];
      if (++x == c.grid_q) {
        x = 0;
        if (++y == c.grid_p) {
          y = 0;
          ++n;
        }
      }
    }
  }
};

// MN-contiguous B of the input gradient gathered from the weight storage (see WTapGeom). A
// thread's 8 k are two groups of 4 output channels, each group within one tap (Cout % 4 == 0).
struct WTapSrc {
  static constexpr bool kKC = false;
  const float* colp;
  const WTapGeom* wt;

  __device__ __forceinline__ void init(const float* P, const WTapGeom& w, int r0, int rlim) {
    wt = &w;
    int gc = r0 + (threadIdx.x >> 3) * 4;
    gc = gc < rlim ? gc : rlim - 4;
    colp = P + gc;
  }

  __device__ __forceinline__ int tap_of(const WTapGeom& w, uint32_t q) const {
    const uint32_t rp = fdiv(q, w.dSp);
    const int sp = (int)q - (int)rp * w.Sp;
    return (w.r0 + (int)rp * w.sh) * w.Sf + w.s0 + sp * w.sw;
  }

  __device__ __forceinline__ void load(int k0, int ke, float (&v)[32]) const {
    const WTapGeom& w = *wt;
    const int k8 = (threadIdx.x & 7) * 8;
    int uoff = 0;
    if (w.uniform) {  // the tile's tap and first output channel are scalar
      const uint32_t q = fdiv(k0, w.dCout);
      uoff = (k0 - (int)q * w.Cout) * w.rs + tap_of(w, q) * w.C;
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int k = k0 + k8 + hf * 4;
      const bool ok = k < ke;
      int off;
      if (w.uniform) {
        off = uoff + (k8 + hf * 4) * w.rs;
      } else {
        const uint32_t q = fdiv(k, w.dCout);
        off = (k - (int)q * w.Cout) * w.rs + tap_of(w, q) * w.C;
      }
      off = ok ? off : 0;  // past the end: output channels 0..3 of the first tap, dropped
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x4 a = sel4(ok, ld4(colp + off + e * w.rs));
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * (4 * hf + e) + j] = a[j];
      }
    }
  }
};

template <int MODE>
__global__ __launch_bounds__(kT) void conv_bf16_kernel(CParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const BParams& g = p.g;
  const int z = blockIdx.x / g.tiles_mn, t = blockIdx.x % g.tiles_mn;
  const int m0 = (t / g.tiles_n) * kBM, n0 = (t % g.tiles_n) * kBN;
  if (MODE == kConvFwd) {
    RowsSrc<false> sa;
    sa.init(g.A, p.cv, m0, g.M);
    const DenseSrc<true, kLoadTail> sb{g.B, g.ldb, g.N, n0};
    tile_body(g, sa, sb, smem, m0, n0, z);
  } else if (MODE == kConvDgrad) {
    RowsSrc<true> sa;
    sa.init(g.A, p.cv, m0, g.M);
    WTapSrc sb;
    sb.init(g.B, p.wt, n0, g.N);
    tile_body(g, sa, sb, smem, m0, n0, z);
  } else {
    const DenseSrc<false, kLoadTail> sa{g.A, g.lda, g.M, m0};
    ColsSrc sb;
    sb.init(g.B, p.cv, n0, g.N);
    tile_body(g, sa, sb, smem, m0, n0, z);
  }
}

template <int MODE>
void launch(const CParams& p, int nblocks, hipStream_t s) {
  static bool configured = false;
  if (!configured) {
    (void)hipFuncSetAttribute((const void*)conv_bf16_kernel<MODE>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsB);
    configured = true;
  }
  hipLaunchKernelGGL((conv_bf16_kernel<MODE>), dim3(nblocks), dim3(kT), kLdsB, s, p);
}

inline bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

ConvPlan conv_bf16_plan(int mode, const ConvGeom& g, int num_cus) {
  ConvPlan pl;
  pl.mode = mode;
  if (mode == kConvFwd) { pl.M = g.N * g.P * g.Q; pl.N = g.Cout; pl.K = g.R * g.S * g.C; }
  else if (mode == kConvDgrad) { pl.M = g.N * g.H * g.W; pl.N = g.C; pl.K = g.R * g.S * g.Cout; }
  else { pl.M = g.Cout; pl.N = g.R * g.S * g.C; pl.K = g.N * g.P * g.Q; }
  pl.fm = 2; pl.fn = 2; pl.bm = kBM;
  // gemm_bf16's split rule; the measured fp32 plan table is for another kernel
  pl.k_per_split = split_k(pl.M, pl.N, pl.K, num_cus);
  pl.splits = ceil_div(pl.K, pl.k_per_split);
  pl.ws_floats = pl.splits > 1 ? (long)pl.splits * pl.M * pl.N : 0;
  return pl;
}

void conv_bf16_run(const ConvPlan& pl, const ConvGeom& g, const float* A, const float* B,
                   float* C, const float* bias, bool relu, float beta, float* ws, hipStream_t s,
                   const WeightTaps* wtap) {
  if (g.C % 4 || g.Cout % 4 || g.C < 4 || g.Cout < 4)
    throw std::runtime_error("conv_bf16: channel counts must be multiples of 4");
  if (pl.M < 1 || pl.N < 1 || pl.K < 1) throw std::runtime_error("conv_bf16: empty operand");
  if (beta != 0.f && beta != 1.f) throw std::runtime_error("conv_bf16: beta must be 0 or 1");
  if (!al16(A) || !al16(B)) throw std::runtime_error("conv_bf16: operands must be 16-B aligned");
  if (pl.splits > 1 && ws == nullptr) throw std::runtime_error("conv_bf16: split-K workspace missing");
  if ((long)g.N * g.C * g.H * g.W >= (1L << 31) || (long)g.N * g.Cout * g.P * g.Q >= (1L << 31))
    throw std::runtime_error("conv_bf16: tensors must have < 2^31 elements");
  CParams p{};
  if (pl.mode == kConvDgrad) {
    if (wtap == nullptr || g.sh != 1 || g.sw != 1)
      throw std::runtime_error("conv_bf16: the input gradient takes stride-1 geometry with "
                               "weight taps (strided gradients go by phases)");
    if ((long)g.Cout * wtap->R * wtap->S * g.C >= (1L << 31))
      throw std::runtime_error("conv_bf16: weight must have < 2^31 elements");
    WTapGeom& w = p.wt;
    w.Cout = g.Cout; w.Sp = g.S;
    w.r0 = wtap->r0; w.s0 = wtap->s0; w.sh = wtap->sh; w.sw = wtap->sw;
    w.Sf = wtap->S; w.C = g.C;
    w.rs = wtap->R * wtap->S * g.C;
    w.uniform = g.Cout % kBK == 0 ? 1 : 0;
    w.dCout = make_fastdiv(g.Cout);
    w.dSp = make_fastdiv(g.S);
  } else if (wtap != nullptr) {
    throw std::runtime_error("conv_bf16: weight taps are for the input gradient");
  }
  CvGeom& cv = p.cv;
  cv.S = g.S; cv.sh = g.sh; cv.sw = g.sw; cv.ph = g.ph; cv.pw = g.pw;
  if (pl.mode == kConvDgrad) {
    cv.Hs = g.P; cv.Ws = g.Q; cv.Cs = g.Cout;
    cv.grid_p = g.H; cv.grid_q = g.W;
  } else {
    cv.Hs = g.H; cv.Ws = g.W; cv.Cs = g.C;
    cv.grid_p = g.P; cv.grid_q = g.Q;
  }
  cv.uniform = cv.Cs % kBK == 0 ? 1 : 0;
  cv.dC = make_fastdiv(cv.Cs);
  cv.dS = make_fastdiv(g.S);
  cv.dPQ = make_fastdiv(cv.grid_p * cv.grid_q);
  cv.dQ = make_fastdiv(cv.grid_q);
  BParams& b = p.g;
  b.A = A; b.B = B; b.C = C; b.ws = ws; b.bias = bias; b.gate = nullptr;
  b.lda = pl.mode == kConvWgrad ? pl.M : 0;
  b.ldb = pl.mode == kConvFwd ? pl.K : 0;
  b.ldc = pl.N; b.ldg = 0;
  b.M = pl.M; b.N = pl.N; b.K = pl.K;
  b.kps = pl.k_per_split;
  b.splits = pl.splits;
  b.tiles_n = ceil_div(pl.N, kBN);
  b.tiles_mn = ceil_div(pl.M, kBM) * b.tiles_n;
  b.relu = relu ? 1 : 0;
  b.beta = beta != 0.f ? 1 : 0;
  const int nblocks = b.tiles_mn * pl.splits;
  if (pl.mode == kConvFwd) launch<kConvFwd>(p, nblocks, s);
  else if (pl.mode == kConvDgrad) launch<kConvDgrad>(p, nblocks, s);
  else launch<kConvWgrad>(p, nblocks, s);
  if (pl.splits > 1) bf16_reduce(b, s);
}

}  // namespace tdp
