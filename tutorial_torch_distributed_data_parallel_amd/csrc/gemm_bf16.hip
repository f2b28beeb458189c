// Mixed-precision GEMM over fp32 tensors (gfx950): C = bf16(A) . op(bf16(B)), fp32 accumulation.
//
// The autocast path of ops/linear.py. Operands and output live in memory as fp32; every operand
// element is rounded ONCE to bf16 (round-to-nearest-even, v_cvt_pk_bf16_f32 -- the conversion
// split3_bits uses for its head term) and the products run as ONE v_mfma_f32_32x32x16_bf16 per
// 16-deep K step: one of the six products of the split-bf16 fp32 GEMM (gemm_f32_fast.hip) and none
// of its VALU split. The products of two bf16 values are exact in fp32, so the only error beyond
// the operand rounding is the fp32 accumulation.
//
// Layout of the kernel (the tile itself -- loaders, LDS image, MFMA loop, epilogue -- is
// bf16_tile.h, shared with the convolutions of conv_bf16.hip):
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
#include "bf16_tile.h"  // the tile: loaders, LDS image, MFMA loop, epilogue

namespace tdp {
using namespace bf16t;
namespace {

template <bool AKC, bool BKC, bool GUARD>
__global__ __launch_bounds__(kT) void gemm_bf16_kernel(BParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int z = blockIdx.x / p.tiles_mn, t = blockIdx.x % p.tiles_mn;
  const int m0 = (t / p.tiles_n) * kBM, n0 = (t % p.tiles_n) * kBN;
  constexpr int MODE = GUARD ? kLoadGuard : kLoadFast;
  const DenseSrc<AKC, MODE> sa{p.A, p.lda, p.M, m0};
  const DenseSrc<BKC, MODE> sb{p.B, p.ldb, p.N, n0};
  tile_body(p, sa, sb, smem, m0, n0, z);
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

void bf16t::bf16_reduce(const BParams& p, hipStream_t s) {
  const long n = (long)p.M * p.N;
  hipLaunchKernelGGL(bf16_reduce_kernel, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, s, p);
}

GemmBf16Plan gemm_bf16_plan(const GemmBf16Args& a, int num_cus) {
  GemmBf16Plan plan;
  plan.guarded = !(a.K % kBK == 0 && operand_fast(a.A, a.lda, a.M, a.a_kcontig) &&
                   operand_fast(a.B, a.ldb, a.N, a.b_kcontig));
  const int kps = split_k(a.M, a.N, a.K, num_cus);
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
  if (plan.splits > 1) bf16_reduce(p, s);
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
