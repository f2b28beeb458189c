// Mixed-precision GEMM over fp32 tensors (gfx950): C = bf16(A) . op(bf16(B)), fp32 accumulation.
//
// The autocast path of ops/linear.py. Operands and output live in memory as fp32; every operand
// element is rounded ONCE to bf16 (round-to-nearest-even, v_cvt_pk_bf16_f32 -- the conversion
// split3_bits uses for its head term) and the products run as ONE v_mfma_f32_32x32x16_bf16 per
// 16-deep K step: one of the six products of the split-bf16 fp32 GEMM (gemm_f32_fast.hip) and none
// of its VALU split. The products of two bf16 values are exact in fp32, so the only error beyond
// the operand rounding is the fp32 accumulation.
//
// Layout of the kernel:
//   * block tile 128 x 128, 64-deep K tile, 256 threads = 2 x 2 waves of 64 x 64 (2 x 2 MFMA
//     tiles, 16 MFMAs per wave per K tile);
//   * global_load_lds copies raw bytes and cannot convert, so operands are staged through
//     registers: global_load_dwordx4 of fp32 -> packed RNE convert -> ds_write_b128 of bf16. The
//     conversion happens once per element per workgroup (not once per wave that reads it), and
//     LDS holds bf16: [128 rows][64 k] = 128-B rows, 16 KiB per operand, two stages = 64 KiB, two
//     workgroups per CU. The next tile's global loads are in flight behind the current tile's
//     MFMAs; one barrier per K tile;
//   * a 16-B chunk holds the 8 consecutive k of one row: one ds_read_b128 yields a whole MFMA
//     operand; lane half h takes k-slots 8h..8h+7 of the K16 step, for A and B alike. Chunk c of
//     row r sits in slot c ^ ((r >> 1) & 7): the 16 rows of a ds_read_b128 phase cover all 64
//     banks (even rows start at bank 0, odd rows at bank 32, and each parity sees 8 distinct
//     slots);
//   * an MN-contiguous operand (stored [K][MN]) is transposed in the register stage: a thread
//     loads an 8 k x 4 mn block as eight dwordx4 and writes four 16-B chunks;
//   * too few tiles for the chip (skinny M): split-K into a workspace, combined in a FIXED order
//     by bf16_reduce_kernel -- no float atomics, results are bitwise reproducible;
//   * rows that are not 16-B aligned, an MN extent that is no multiple of 4, or K % 64 != 0 take
//     the guarded instantiation (scalar bounds-checked loads, zero fill) of the same kernel.
// Epilogue: bias[N], beta in {0, 1}, ReLU, C-shaped gate (gate > 0), in gemm_f32's order. The row
// sums (bias gradient) are reduced from the UNROUNDED fp32 A by bf16_rowsum_* in a fixed order.
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "split_bf16.h"  // the vector typedefs

namespace tdp {
namespace {

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

// two fp32 -> packed bf16, round-to-nearest-even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack2(float x0, float x1) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, bf2));
}

__device__ __forceinline__ int swz(int row) { return (row >> 1) & 7; }

// One operand tile ([128 rows][64 k]) global -> registers. P: the operand, R rows (M or N), r0
// the tile's first row, k0 the tile's first k, ke the end of this split's K range.
//   KC (K-contiguous, [R][K]): unit u = i * 256 + t is chunk u & 7 of row u >> 3 (four units)
//   else (MN-contiguous, [K][R]): thread t holds k-group t & 7 (8 k) of rows 4 (t >> 3) .. + 3
template <bool KC, bool GUARD>
__device__ __forceinline__ void load_tile(const float* __restrict__ P, long ld, int R, int r0,
                                          int k0, int ke, float (&v)[32]) {
  const int t = threadIdx.x;
  if (KC) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = i * kT + t, row = u >> 3, c = u & 7;
      if (GUARD) {
        const int gr = r0 + row;
        const float* src = P + (long)gr * ld;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int k = k0 + c * 8 + e;
          v[8 * i + e] = (gr < R && k < ke) ? src[k] : 0.f;
        }
      } else {
        // rows past the end are clamped: their outputs are discarded
        const float* src = P + (long)min(r0 + row, R - 1) * ld + k0 + c * 8;
        const f32x4 a = *reinterpret_cast<const f32x4*>(src);
        const f32x4 b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[8 * i + e] = a[e];
          v[8 * i + 4 + e] = b[e];
        }
      }
    }
  } else {
    const int kg = t & 7, col = (t >> 3) * 4;
    if (GUARD) {
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
      const float* src = P + (long)(k0 + kg * 8) * ld + min(r0 + col, R - 4);
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(src + (long)kk * ld);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * kk + j] = a[j];
      }
    }
  }
}

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

template <bool AKC, bool BKC, bool GUARD>
__global__ __launch_bounds__(kT) void gemm_bf16_kernel(BParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int h = lane >> 5, l31 = lane & 31;
  const int z = blockIdx.x / p.tiles_mn, t = blockIdx.x % p.tiles_mn;
  const int m0 = (t / p.tiles_n) * kBM, n0 = (t % p.tiles_n) * kBN;
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
  load_tile<AKC, GUARD>(p.A, p.lda, p.M, m0, kb, ke, va);
  load_tile<BKC, GUARD>(p.B, p.ldb, p.N, n0, kb, ke, vb);
  store_tile<AKC>(smem, va);
  store_tile<BKC>(smem + kOpB, vb);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    if (more) {  // the next tile's global loads fly behind this tile's MFMAs
      load_tile<AKC, GUARD>(p.A, p.lda, p.M, m0, kb + (kt + 1) * kBK, ke, va);
      load_tile<BKC, GUARD>(p.B, p.ldb, p.N, n0, kb + (kt + 1) * kBK, ke, vb);
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
      store_tile<AKC>(st, va);
      store_tile<BKC>(st + kOpB, vb);
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

// C = epilogue(ws[0] + ws[1] + ... + ws[splits - 1]): the partial sums are added in index order
__global__ __launch_bounds__(kT) void bf16_reduce_kernel(BParams p) {
  const long n = (long)p.M * p.N;
  const long idx = (long)blockIdx.x * kT + threadIdx.x;
  if (idx >= n) return;
  float v = p.ws[idx];
  for (int z = 1; z < p.splits; ++z) v += p.ws[(long)z * n + idx];
  const int row = (int)(idx / p.N), col = (int)(idx - (long)row * p.N);
  float* c = p.C + (long)row * p.ldc + col;
  if (p.bias) v += p.bias[col];
  if (p.beta) v += *c;
  if (p.relu) v = fmaxf(v, 0.f);
  if (p.gate) v = p.gate[(long)row * p.ldg + col] > 0.f ? v : 0.f;
  *c = v;
}

// Row sums of op(A) [M][K] from the unrounded fp32 values, fixed order.
// A stored [K][M] (the weight gradient's g [batch][out]): 64 columns x 4 k-slices per workgroup,
// each slice summed serially over its k, the four slices added in slice order.
__global__ __launch_bounds__(kT) void bf16_rowsum_mn_kernel(const float* __restrict__ A, long lda,
                                                            int M, int K, float* __restrict__ out) {
  __shared__ float part[4][64];
  const int c = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int m = blockIdx.x * 64 + c;
  const int per = (K + 3) / 4;
  const int k1 = min(K, (sl + 1) * per);
  float s = 0.f;
  if (m < M)
    for (int k = sl * per; k < k1; ++k) s += A[(long)k * lda + m];
  part[sl][c] = s;
  __syncthreads();
  if (sl == 0 && m < M) out[m] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

// A stored [M][K]: one wave per row (lane-strided partial sums, then the wave butterfly)
__global__ __launch_bounds__(kT) void bf16_rowsum_k_kernel(const float* __restrict__ A, long lda,
                                                           int M, int K, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
  if (m >= M) return;
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s += A[(long)m * lda + k];
  s = wave_sum(s);
  if (lane == 0) out[m] = s;
}

inline bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// an operand takes the vector (unguarded) loads
bool operand_fast(const float* P, long ld, int R, bool kcontig) {
  return al16(P) && ld % 4 == 0 && (kcontig || R % 4 == 0);
}

template <bool AKC, bool BKC, bool GUARD>
void launch(const BParams& p, int nblocks, hipStream_t s) {
  static bool configured = false;
  if (!configured) {
    (void)hipFuncSetAttribute((const void*)gemm_bf16_kernel<AKC, BKC, GUARD>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsB);
    configured = true;
  }
  hipLaunchKernelGGL((gemm_bf16_kernel<AKC, BKC, GUARD>), dim3(nblocks), dim3(kT), kLdsB, s, p);
}

template <bool GUARD>
void launch_layout(const BParams& p, bool akc, bool bkc, int nblocks, hipStream_t s) {
  if (akc && bkc) launch<true, true, GUARD>(p, nblocks, s);
  else if (akc) launch<true, false, GUARD>(p, nblocks, s);
  else if (bkc) launch<false, true, GUARD>(p, nblocks, s);
  else launch<false, false, GUARD>(p, nblocks, s);
}

}  // namespace

GemmBf16Plan gemm_bf16_plan(const GemmBf16Args& a, int num_cus) {
  GemmBf16Plan plan;
  plan.guarded = !(a.K % kBK == 0 && operand_fast(a.A, a.lda, a.M, a.a_kcontig) &&
                   operand_fast(a.B, a.ldb, a.N, a.b_kcontig));
  const long tiles = (long)ceil_div(a.M, kBM) * ceil_div(a.N, kBN);
  // two workgroups per CU (64 KiB of LDS each); split-K when the tile grid alone leaves CUs idle,
  // with at least two K tiles per split
  int splits = 1;
  if (tiles < num_cus) {
    const int want = (int)((2L * num_cus + tiles - 1) / tiles);
    const int kmax = a.K / (2 * kBK);
    splits = want < kmax ? want : kmax;
    if (splits > 32) splits = 32;  // bounds the partial-sum traffic of the combine
    if (splits < 1) splits = 1;
  }
  const int kps = ceil_div(ceil_div(a.K, splits), kBK) * kBK;
  plan.k_per_split = kps;
  plan.splits = ceil_div(a.K, kps);
  plan.ws_floats = plan.splits > 1 ? (long)plan.splits * a.M * a.N : 0;
  return plan;
}

void gemm_bf16(const GemmBf16Args& a, hipStream_t s) {
  if (a.M < 1 || a.N < 1 || a.K < 1) throw std::runtime_error("gemm_bf16: empty operand");
  if (a.beta != 0.f && a.beta != 1.f) throw std::runtime_error("gemm_bf16: beta must be 0 or 1");
  const GemmBf16Plan plan = gemm_bf16_plan(a, a.num_cus);
  if (plan.splits > 1 && (a.ws == nullptr || a.ws_floats < plan.ws_floats))
    throw std::runtime_error("gemm_bf16: split-K workspace missing");
  BParams p{};
  p.A = a.A; p.B = a.B; p.C = a.C;
  p.ws = a.ws;
  p.bias = a.bias; p.gate = a.gate;
  p.lda = a.lda; p.ldb = a.ldb; p.ldc = a.ldc; p.ldg = a.ldgate;
  p.M = a.M; p.N = a.N; p.K = a.K;
  p.kps = plan.k_per_split;
  p.splits = plan.splits;
  p.tiles_n = ceil_div(a.N, kBN);
  p.tiles_mn = ceil_div(a.M, kBM) * p.tiles_n;
  p.relu = a.relu ? 1 : 0;
  p.beta = a.beta != 0.f ? 1 : 0;
  const int nblocks = p.tiles_mn * plan.splits;
  if (plan.guarded) launch_layout<true>(p, a.a_kcontig, a.b_kcontig, nblocks, s);
  else launch_layout<false>(p, a.a_kcontig, a.b_kcontig, nblocks, s);
  if (plan.splits > 1) {
    const long n = (long)a.M * a.N;
    hipLaunchKernelGGL(bf16_reduce_kernel, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, s, p);
  }
  if (a.rowsum) {
    if (a.a_kcontig)
      hipLaunchKernelGGL(bf16_rowsum_k_kernel, dim3(ceil_div(a.M, kT / 64)), dim3(kT), 0, s, a.A,
                         a.lda, a.M, a.K, a.rowsum);
    else
      hipLaunchKernelGGL(bf16_rowsum_mn_kernel, dim3(ceil_div(a.M, 64)), dim3(kT), 0, s, a.A,
                         a.lda, a.M, a.K, a.rowsum);
  }
}

}  // namespace tdp
