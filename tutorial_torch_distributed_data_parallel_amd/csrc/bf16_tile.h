// The bf16 mixed-precision tile shared by gemm_bf16.hip (dense operands) and conv_bf16.hip
// (implicit convolution operands): fp32 operands global -> registers -> packed RNE convert ->
// swizzled bf16 LDS -> one v_mfma_f32_32x32x16_bf16 per K16 step, fp32 accumulation, and the
// bias / beta / ReLU / gate epilogue. See gemm_bf16.hip for the layout; an operand source only
// has to fill the `float v[32]` register image of its share of a [128 rows][64 k] tile:
//   K-contiguous image : unit u = i * 256 + t (i = 0..3) is the 8 k of chunk u & 7 of row u >> 3,
//                        v[8 i .. 8 i + 7]
//   MN-contiguous image: thread t holds k-group t & 7 (8 k) of rows 4 (t >> 3) .. + 3,
//                        v[4 kk + j] = element (k = 8 (t & 7) + kk, row 4 (t >> 3) + j)
// A source type S provides `static constexpr bool kKC` (which image) and
// `void load(int k0, int ke, float (&v)[32]) const` (k0 the tile's first k, ke the end of this
// split's K range: elements at k >= ke are zero).
#pragma once
#include "common.h"
#include "split_bf16.h"  // the vector typedefs

namespace tdp {
namespace bf16t {

constexpr int kT = 256;
constexpr int kBM = 128, kBN = 128, kBK = 64;
constexpr int kRowB = kBK * 2;          // LDS row: 64 bf16
constexpr int kOpB = kBM * kRowB;       // 16 KiB per operand tile
constexpr int kStageB = 2 * kOpB;       // A + B
constexpr int kLdsB = 2 * kStageB;      // two stages

struct BParams {
  const float* A;
  const float* B;
  float* C;
  float* ws;
  const float* bias;
  const float* gate;
  long lda, ldb, ldc, ldg;
  int M, N, K, kps, splits, tiles_n, tiles_mn;
  int relu, beta;
};

// operand load modes: vector loads of whole tiles (K % 64 == 0), scalar bounds-checked loads, or
// vector loads with the K tail zero-filled (per 4 k of a K-contiguous row -- K % 4 == 0 -- or per
// k of an MN-contiguous operand)
constexpr int kLoadFast = 0, kLoadGuard = 1, kLoadTail = 2;

// two fp32 -> packed bf16, round-to-nearest-even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack2(float x0, float x1) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, bf2));
}

__device__ __forceinline__ int swz(int row) { return (row >> 1) & 7; }

__device__ __forceinline__ f32x4 ld4(const float* q) {
  return *reinterpret_cast<const f32x4*>(q);
}

// One dense operand tile ([128 rows][64 k]) global -> registers. P: the operand, R rows (M or
// N), r0 the tile's first row, k0 the tile's first k, ke the end of this split's K range.
template <bool KC, int MODE>
__device__ __forceinline__ void load_tile(const float* __restrict__ P, long ld, int R, int r0,
                                          int k0, int ke, float (&v)[32]) {
  const int t = threadIdx.x;
  if (KC) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = i * kT + t, row = u >> 3, c = u & 7;
      if (MODE == kLoadGuard) {
        const int gr = r0 + row;
        const float* src = P + (long)gr * ld;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int k = k0 + c * 8 + e;
          v[8 * i + e] = (gr < R && k < ke) ? src[k] : 0.f;
        }
      } else {
        // rows past the end are clamped: their outputs are discarded
        const float* row_p = P + (long)min(r0 + row, R - 1) * ld;
        const int k = k0 + c * 8;
        f32x4 a, b;
        if (MODE == kLoadTail) {
          // a 4-k group past the end is read at the row's start and dropped
          const bool oka = k < ke, okb = k + 4 < ke;
          a = ld4(row_p + (oka ? k : 0));
          b = ld4(row_p + (okb ? k + 4 : 0));
          a = oka ? a : f32x4{0.f, 0.f, 0.f, 0.f};
          b = okb ? b : f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
          a = ld4(row_p + k);
          b = ld4(row_p + k + 4);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[8 * i + e] = a[e];
          v[8 * i + 4 + e] = b[e];
        }
      }
    }
  } else {
    const int kg = t & 7, col = (t >> 3) * 4;
    if (MODE == kLoadGuard) {
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const int k = k0 + kg * 8 + kk;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int gr = r0 + col + j;
          v[4 * kk + j] = (k < ke && gr < R) ? P[(long)k * ld + gr] : 0.f;
        }
      }
    } else {
      // R % 4 == 0: a quad of rows is wholly inside or wholly outside (clamped, discarded)
      const float* col_p = P + min(r0 + col, R - 4);
      const int kf = k0 + kg * 8;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        f32x4 a;
        if (MODE == kLoadTail) {
          const bool ok = kf + kk < ke;
          a = ld4(col_p + (long)(ok ? kf + kk : ke - 1) * ld);
          a = ok ? a : f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
          a = ld4(col_p + (long)(kf + kk) * ld);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * kk + j] = a[j];
      }
    }
  }
}

// a dense [R][K] (KC) or [K][R] operand as a tile source
template <bool KC, int MODE>
struct DenseSrc {
  static constexpr bool kKC = KC;
  const float* P;
  long ld;
  int R, r0;
  __device__ __forceinline__ void load(int k0, int ke, float (&v)[32]) const {
    load_tile<KC, MODE>(P, ld, R, r0, k0, ke, v);
  }
};

// registers -> bf16 LDS image of the tile (16-B chunks of 8 k, swizzled)
template <bool KC>
__device__ __forceinline__ void store_tile(char* base, const float (&v)[32]) {
  const int t = threadIdx.x;
  if (KC) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = i * kT + t, row = u >> 3, c = u & 7;
      const u32x4 w{pack2(v[8 * i], v[8 * i + 1]), pack2(v[8 * i + 2], v[8 * i + 3]),
                    pack2(v[8 * i + 4], v[8 * i + 5]), pack2(v[8 * i + 6], v[8 * i + 7])};
      *reinterpret_cast<u32x4*>(base + row * kRowB + ((c ^ swz(row)) * 16)) = w;
    }
  } else {
    const int kg = t & 7, col = (t >> 3) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = col + j;
      const u32x4 w{pack2(v[j], v[4 + j]), pack2(v[8 + j], v[12 + j]),
                    pack2(v[16 + j], v[20 + j]), pack2(v[24 + j], v[28 + j])};
      *reinterpret_cast<u32x4*>(base + row * kRowB + ((kg ^ swz(row)) * 16)) = w;
    }
  }
}

// One 128 x 128 output tile (first row m0, first column n0) of split z: the K loop over
// [z * kps, min(K, (z + 1) * kps)) with the operands read through `sa` / `sb`, then the epilogue
// (or the partial sums of a split-K plan, combined by bf16_reduce).
template <class SA, class SB>
__device__ __forceinline__ void tile_body(const BParams& p, const SA& sa_src, const SB& sb_src,
                                          char* smem, int m0, int n0, int z) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int h = lane >> 5, l31 = lane & 31;
  const int kb = z * p.kps;
  const int ke = min(p.K, kb + p.kps);
  const int nk = (ke - kb + kBK - 1) / kBK;

  f32x16 acc[2][2];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[f][g][r] = 0.f;

  float va[32], vb[32];
  sa_src.load(kb, ke, va);
  sb_src.load(kb, ke, vb);
  store_tile<SA::kKC>(smem, va);
  store_tile<SB::kKC>(smem + kOpB, vb);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    if (more) {  // the next tile's global loads fly behind this tile's MFMAs
      sa_src.load(kb + (kt + 1) * kBK, ke, va);
      sb_src.load(kb + (kt + 1) * kBK, ke, vb);
    }
    const char* sa = smem + (kt & 1) * kStageB;
    const char* sb = sa + kOpB;
#pragma unroll
    for (int s = 0; s < kBK / 16; ++s) {
      bf8 a[2], b[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const int ra = wm * 64 + f * 32 + l31, rb = wn * 64 + f * 32 + l31;
        a[f] = *reinterpret_cast<const bf8*>(sa + ra * kRowB + (((2 * s + h) ^ swz(ra)) * 16));
        b[f] = *reinterpret_cast<const bf8*>(sb + rb * kRowB + (((2 * s + h) ^ swz(rb)) * 16));
      }
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int g = 0; g < 2; ++g)
          acc[f][g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[f], b[g], acc[f][g], 0, 0, 0);
    }
    if (more) {
      // the other stage: every wave left it at the barrier that ended the previous iteration
      char* st = smem + ((kt + 1) & 1) * kStageB;
      store_tile<SA::kKC>(st, va);
      store_tile<SB::kKC>(st + kOpB, vb);
    }
    __syncthreads();
  }

  // MFMA 32x32 layout: acc[r] is row (r & 3) + 8 (r >> 2) + 4 h, column l31 of the tile
  float* ws = p.ws + (long)z * p.M * p.N;
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int col = n0 + wn * 64 + g * 32 + l31;
      if (col >= p.N) continue;
      const float bias = (p.splits == 1 && p.bias) ? p.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 64 + f * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row >= p.M) continue;
        float v = acc[f][g][r];
        if (p.splits > 1) {
          ws[(long)row * p.N + col] = v;
          continue;
        }
        float* c = p.C + (long)row * p.ldc + col;
        v += bias;
        if (p.beta) v += *c;
        if (p.relu) v = fmaxf(v, 0.f);
        if (p.gate) v = p.gate[(long)row * p.ldg + col] > 0.f ? v : 0.f;
        *c = v;
      }
    }
}

// The K split gemm_bf16_plan uses: split only when the tile grid alone leaves CUs idle (two
// workgroups per CU), at least two K tiles per split, at most 32 splits (bounds the partial-sum
// traffic of the combine). Returns the k per split (a multiple of 64); splits = ceil(K / it).
inline int split_k(int M, int N, int K, int num_cus) {
  const long tiles = (long)ceil_div(M, kBM) * ceil_div(N, kBN);
  int splits = 1;
  if (tiles < num_cus) {
    const int want = (int)((2L * num_cus + tiles - 1) / tiles);
    const int kmax = K / (2 * kBK);
    splits = want < kmax ? want : kmax;
    if (splits > 32) splits = 32;
    if (splits < 1) splits = 1;
  }
  return ceil_div(ceil_div(K, splits), kBK) * kBK;
}

// C = epilogue(ws[0] + ws[1] + ... + ws[splits - 1]), the partial sums added in index order
// (gemm_bf16.hip)
void bf16_reduce(const BParams& p, hipStream_t s);

}  // namespace bf16t
}  // namespace tdp
