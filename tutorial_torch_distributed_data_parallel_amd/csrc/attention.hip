// Fused scaled-dot-product attention for gfx950: softmax(scale * q k^T) v and its gradients, with
// every GEMM an fp32 GEMM on the bf16 matrix core (split_bf16.h: exact three-way split, six kept
// products, fp32 accumulation) and the score matrix never written to memory.
//
// Tensors are [B][H][S][D] through strides (AttnT: batch / head / row strides, unit inner stride,
// 16-byte aligned rows), D = 32 or 64. The output and the gradients are written through strides
// too, so a packed [B, S, 3, H, D] projection is read and its gradient written in place.
//
// One register layout serves all three kernels. v_mfma_f32_32x32x16_bf16 gives lane (i = lane % 32,
// half = lane / 32) column i of the 32x32 product and its rows 8g + 4 half + s (g, s < 4) in
// accumulator 4g + s. Every score product is computed with the wave's OWN 32 rows (queries in the
// forward and dq kernels, keys in the dk/dv kernel) as the B operand held in registers, and the
// walked tile (in LDS, fp32) as the A operand. So
//   * a lane holds one own row and 16 of the 32 walked rows: softmax statistics of an own row are
//     an in-lane reduction plus one exchange with lane ^ 32, rescaling is a per-lane scalar;
//   * accumulators 8t .. 8t+7 are the walked rows 16t + 8q + 4 half + s: exactly the k-slot
//     permutation split_bf16.h documents for an operand (k = 8q + 4h + s), so p (or dS) goes
//     straight from the accumulators through split3_x8 into the second GEMM as its B operand; the
//     A operand (the walked tile, transposed) is read from LDS with the same permutation.
// Operand staging: the walked tiles are staged global -> registers -> LDS as fp32 (tail rows
// select zero, nothing is read past a tensor) and split per fragment by the wave that consumes
// them; the own rows are loaded and split once per wave. The per-fragment split is VALU work that
// hides under the previous fragment's six MFMAs (192 matrix-core cycles against ~40 VALU issues),
// and fp32 tiles keep LDS at 2 * 64 * (D + 4) * 4 B = 34 KB (D = 64) for up to four workgroups
// a CU.
//
// Work split (fixed summation order, no atomics, partition a function of (Sq, Sk, D) only, one
// (b, h) per blockIdx.y, so results repeat bitwise and do not depend on the batch):
//   forward  workgroup = 128 queries (4 waves x 32), walks 64-key tiles, online softmax;
//   dq       workgroup = 128 queries, walks 64-key tiles, recomputes p from lse;
//   dk, dv   workgroup = 128 keys (4 waves x 32), walks 64-query tiles, recomputes p from lse;
//   delta    rowsum(dO * O) as the diagonal of the MFMA product, in both operand orders, so
//            that it cancels dP exactly where the softmax is one-hot; one small launch.
#include <math.h>

#include <algorithm>

#include "kernels.h"
#include "split_bf16.h"

namespace tdp {
namespace {

constexpr int kAttnThreads = 256;  // 4 waves
constexpr int kOwn = 128;          // rows a workgroup owns (32 a wave)
constexpr int kWalk = 64;          // rows of a walked tile (two 32-row blocks)

// the B-operand fragments of a lane's own row: k-slots d = 16t + 8q + 4 half + s
template <int D>
struct RowFrags {
  bf8 h[D / 16], m[D / 16], l[D / 16];
};

template <int D>
__device__ __forceinline__ void load_row_frags(const float* row, int half, RowFrags<D>& f) {
#pragma unroll
  for (int t = 0; t < D / 16; ++t) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (row) {
      a = *reinterpret_cast<const f32x4*>(row + 16 * t + 4 * half);
      b = *reinterpret_cast<const f32x4*>(row + 16 * t + 8 + 4 * half);
    }
    split3_x8(a, b, f.h[t], f.m[t], f.l[t]);
  }
}

// rows r0 .. r0 + 63 of a [rows][D] tensor -> tile[64][D + 4] (rows at or past `rows` are zero)
template <int D>
__device__ __forceinline__ void stage_tile(float* tile, const float* base, long ss, int r0,
                                           int rows) {
  constexpr int C4 = D / 4, LD = D + 4;
  for (int idx = threadIdx.x; idx < kWalk * C4; idx += kAttnThreads) {
    const int r = idx / C4, c = idx % C4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r0 + r < rows) v = *reinterpret_cast<const f32x4*>(base + (long)(r0 + r) * ss + 4 * c);
    *reinterpret_cast<f32x4*>(tile + r * LD + 4 * c) = v;
  }
}

// A operand, k-step t of tile row `row`: the same k-slots as RowFrags
template <int D>
__device__ __forceinline__ void tile_row_frag(const float* tile, int row, int t, int half, bf8& h,
                                              bf8& m, bf8& l) {
  const float* p = tile + row * (D + 4) + 16 * t + 4 * half;
  split3_x8(*reinterpret_cast<const f32x4*>(p), *reinterpret_cast<const f32x4*>(p + 8), h, m, l);
}

// A operand of the transposed tile: the lane's row is tile column c, its k-slots are the tile
// rows r0 + 8q + 4 half + s (the accumulator order of the score product)
template <int D>
__device__ __forceinline__ void tile_col_frag(const float* tile, int r0, int c, int half, bf8& h,
                                              bf8& m, bf8& l) {
  const float* p = tile + (r0 + 4 * half) * (D + 4) + c;
  float x[8];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int s = 0; s < 4; ++s) x[4 * q + s] = p[(8 * q + s) * (D + 4)];
  split3_x8(x, h, m, l);
}

// tile rows [rb, rb + 32) x own rows: sum over d, A from the tile, B from the own-row fragments
template <int D>
__device__ __forceinline__ f32x16 score_block(const float* tile, int rb, int i, int half,
                                              const RowFrags<D>& own) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int t = 0; t < D / 16; ++t) {
    bf8 ah, am, al;
    tile_row_frag<D>(tile, rb + i, t, half, ah, am, al);
    acc = mfma_emu6(ah, am, al, own.h[t], own.m[t], own.l[t], acc);
  }
  return acc;
}

// acc[db] += tile^T (columns 32 db + i, rows rb + 16 tt + ...) . x (accumulators 8 tt .. 8 tt + 7)
template <int D>
__device__ __forceinline__ void accum_block(const float* tile, int rb, int i, int half,
                                            const f32x16& x, f32x16 (&acc)[D / 32]) {
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    bf8 xh, xm, xl;
    split3_x8(x[8 * tt], x[8 * tt + 1], x[8 * tt + 2], x[8 * tt + 3], x[8 * tt + 4],
              x[8 * tt + 5], x[8 * tt + 6], x[8 * tt + 7], xh, xm, xl);
#pragma unroll
    for (int db = 0; db < D / 32; ++db) {
      bf8 ah, am, al;
      tile_col_frag<D>(tile, rb + 16 * tt, 32 * db + i, half, ah, am, al);
      acc[db] = mfma_emu6(ah, am, al, xh, xm, xl, acc[db]);
    }
  }
}

// the lane's accumulators (own row `row`, columns 32 db + 8g + 4 half + s) times f -> dst
template <int D>
__device__ __forceinline__ void store_own(float* rowp, int half, const f32x16 (&acc)[D / 32],
                                          float f) {
#pragma unroll
  for (int db = 0; db < D / 32; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 v = {acc[db][4 * g] * f, acc[db][4 * g + 1] * f, acc[db][4 * g + 2] * f,
                 acc[db][4 * g + 3] * f};
      *reinterpret_cast<f32x4*>(rowp + 32 * db + 8 * g + 4 * half) = v;
    }
}

__device__ __forceinline__ const float* head_of(const AttnT& t, int b, int h) {
  return t.p + (long)b * t.sb + (long)h * t.sh;
}

// ---------------------------------------------------------------------------------- forward
template <int D>
__global__ __launch_bounds__(kAttnThreads) void attn_fwd_kernel(AttnT q, AttnT k, AttnT v,
                                                                AttnT o, float* __restrict__ lse,
                                                                int H, int Sq, int Sk,
                                                                float scale) {
  constexpr int LD = D + 4, NB = D / 32;
  __shared__ __attribute__((aligned(16))) float ks[kWalk * LD];
  __shared__ __attribute__((aligned(16))) float vs[kWalk * LD];
  const int bh = blockIdx.y, b = bh / H, hd = bh % H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, half = lane >> 5;
  const int row0 = blockIdx.x * kOwn + wave * 32, qrow = row0 + i;
  const bool active = row0 < Sq;  // wave-uniform: a wave with no query rows only stages tiles
  const float* kp = head_of(k, b, hd);
  const float* vp = head_of(v, b, hd);
  RowFrags<D> qf;
  load_row_frags<D>(qrow < Sq ? head_of(q, b, hd) + (long)qrow * q.ss : nullptr, half, qf);
  f32x16 oacc[NB];
#pragma unroll
  for (int db = 0; db < NB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
  float m = -INFINITY, l = 0.f;  // running max of the row; this lane's half of the running sum
  for (int k0 = 0; k0 < Sk; k0 += kWalk) {
    __syncthreads();
    stage_tile<D>(ks, kp, k.ss, k0, Sk);
    stage_tile<D>(vs, vp, v.ss, k0, Sk);
    __syncthreads();
    if (!active) continue;
    f32x16 p[2];
    float mx = m;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      p[kb] = score_block<D>(ks, 32 * kb, i, half, qf);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + 32 * kb + 8 * (r >> 2) + 4 * half + (r & 3);
        p[kb][r] = key < Sk ? p[kb][r] * scale : -INFINITY;  // a tail key has probability 0
        mx = fmaxf(mx, p[kb][r]);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
    const float alpha = expf(m - mx);  // 0 on the first tile (m = -inf; mx is finite: key k0 < Sk)
    m = mx;
    float rs = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[kb][r] = expf(p[kb][r] - mx);
        rs += p[kb][r];
      }
    l = l * alpha + rs;
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) accum_block<D>(vs, 32 * kb, i, half, p[kb], oacc);
  }
  if (!active) return;
  l += __shfl_xor(l, 32, kWave);
  if (qrow < Sq) {
    float* op = const_cast<float*>(head_of(o, b, hd)) + (long)qrow * o.ss;
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {oacc[db][4 * g] / l, oacc[db][4 * g + 1] / l, oacc[db][4 * g + 2] / l,
                     oacc[db][4 * g + 3] / l};
        *reinterpret_cast<f32x4*>(op + 32 * db + 8 * g + 4 * half) = val;
      }
    if (half == 0) lse[(long)bh * Sq + qrow] = m + logf(l);
  }
}

// ------------------------------------------------------------------------------------ delta
// delta[q] = sum_d dO[q][d] * o[q][d], as the diagonal of the same six-product MFMA GEMM that
// forms dP in the backward kernels, once per operand order: delta_q with (o, dO) in the places of
// (v, dO) in the dq kernel, delta_k with (dO, o) in the places of (dO, v) in the dk/dv kernel.
// Where the softmax is exactly one-hot, o is bitwise a row of v, so dP - delta is exactly 0 in
// both kernels (a single key: dq = dk = 0, as in exact arithmetic), which a plain fp32 dot
// product beside an MFMA dP does not give. A wave owns 32 rows; element (i, i) of the 32x32
// product is accumulator 4 (i / 8) + i % 4 of lane i + 32 ((i / 4) % 2).
template <int D>
__global__ __launch_bounds__(kAttnThreads) void attn_delta_kernel(AttnT dout, AttnT o,
                                                                  float* __restrict__ delta_q,
                                                                  float* __restrict__ delta_k,
                                                                  int H, int Sq) {
  const int bh = blockIdx.y, b = bh / H, hd = bh % H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, half = lane >> 5;
  const int row = blockIdx.x * kOwn + wave * 32 + i;
  const bool mine = row < Sq;
  RowFrags<D> gf, of;
  load_row_frags<D>(mine ? head_of(dout, b, hd) + (long)row * dout.ss : nullptr, half, gf);
  load_row_frags<D>(mine ? head_of(o, b, hd) + (long)row * o.ss : nullptr, half, of);
  f32x16 aq, ak;
#pragma unroll
  for (int r = 0; r < 16; ++r) aq[r] = ak[r] = 0.f;
#pragma unroll
  for (int t = 0; t < D / 16; ++t) {
    aq = mfma_emu6(of.h[t], of.m[t], of.l[t], gf.h[t], gf.m[t], gf.l[t], aq);
    ak = mfma_emu6(gf.h[t], gf.m[t], gf.l[t], of.h[t], of.m[t], of.l[t], ak);
  }
  const int diag = 4 * (i >> 3) + (i & 3);
  float vq = 0.f, vk = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (r == diag) {
      vq = aq[r];
      vk = ak[r];
    }
  if (mine && half == ((i >> 2) & 1)) {
    delta_q[(long)bh * Sq + row] = vq;
    delta_k[(long)bh * Sq + row] = vk;
  }
}

// --------------------------------------------------------------------------------------- dq
template <int D>
__global__ __launch_bounds__(kAttnThreads) void attn_bwd_dq_kernel(
    AttnT dout, AttnT q, AttnT k, AttnT v, const float* __restrict__ lse,
    const float* __restrict__ delta, AttnT dq, int H, int Sq, int Sk, float scale) {
  constexpr int LD = D + 4, NB = D / 32;
  __shared__ __attribute__((aligned(16))) float ks[kWalk * LD];
  __shared__ __attribute__((aligned(16))) float vs[kWalk * LD];
  const int bh = blockIdx.y, b = bh / H, hd = bh % H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, half = lane >> 5;
  const int row0 = blockIdx.x * kOwn + wave * 32, qrow = row0 + i;
  const bool active = row0 < Sq, mine = qrow < Sq;
  const float* kp = head_of(k, b, hd);
  const float* vp = head_of(v, b, hd);
  RowFrags<D> qf, gf;
  load_row_frags<D>(mine ? head_of(q, b, hd) + (long)qrow * q.ss : nullptr, half, qf);
  load_row_frags<D>(mine ? head_of(dout, b, hd) + (long)qrow * dout.ss : nullptr, half, gf);
  // a row past Sq: lse = +inf makes its p exactly 0
  const float lse_i = mine ? lse[(long)bh * Sq + qrow] : INFINITY;
  const float delta_i = mine ? delta[(long)bh * Sq + qrow] : 0.f;
  f32x16 acc[NB];
#pragma unroll
  for (int db = 0; db < NB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[db][r] = 0.f;
  for (int k0 = 0; k0 < Sk; k0 += kWalk) {
    __syncthreads();
    stage_tile<D>(ks, kp, k.ss, k0, Sk);
    stage_tile<D>(vs, vp, v.ss, k0, Sk);
    __syncthreads();
    if (!active) continue;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const f32x16 s = score_block<D>(ks, 32 * kb, i, half, qf);   // (k q^T)[key][query]
      const f32x16 dp = score_block<D>(vs, 32 * kb, i, half, gf);  // (v dO^T)[key][query]
      f32x16 ds;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + 32 * kb + 8 * (r >> 2) + 4 * half + (r & 3);
        const float pr = key < Sk ? expf(s[r] * scale - lse_i) : 0.f;
        ds[r] = pr * (dp[r] - delta_i);
      }
      accum_block<D>(ks, 32 * kb, i, half, ds, acc);
    }
  }
  if (mine)
    store_own<D>(const_cast<float*>(head_of(dq, b, hd)) + (long)qrow * dq.ss, half, acc, scale);
}

// ----------------------------------------------------------------------------------- dk, dv
template <int D>
__global__ __launch_bounds__(kAttnThreads) void attn_bwd_dkv_kernel(
    AttnT dout, AttnT q, AttnT k, AttnT v, const float* __restrict__ lse,
    const float* __restrict__ delta, AttnT dk, AttnT dv, int H, int Sq, int Sk, float scale) {
  constexpr int LD = D + 4, NB = D / 32;
  __shared__ __attribute__((aligned(16))) float qs[kWalk * LD];
  __shared__ __attribute__((aligned(16))) float gs[kWalk * LD];
  __shared__ float lses[kWalk], deltas[kWalk];
  const int bh = blockIdx.y, b = bh / H, hd = bh % H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, half = lane >> 5;
  const int row0 = blockIdx.x * kOwn + wave * 32, krow = row0 + i;
  const bool active = row0 < Sk, mine = krow < Sk;
  const float* qp = head_of(q, b, hd);
  const float* gp = head_of(dout, b, hd);
  RowFrags<D> kf, vf;
  load_row_frags<D>(mine ? head_of(k, b, hd) + (long)krow * k.ss : nullptr, half, kf);
  load_row_frags<D>(mine ? head_of(v, b, hd) + (long)krow * v.ss : nullptr, half, vf);
  f32x16 dka[NB], dva[NB];
#pragma unroll
  for (int db = 0; db < NB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) dka[db][r] = dva[db][r] = 0.f;
  for (int q0 = 0; q0 < Sq; q0 += kWalk) {
    __syncthreads();
    stage_tile<D>(qs, qp, q.ss, q0, Sq);
    stage_tile<D>(gs, gp, dout.ss, q0, Sq);
    if (threadIdx.x < kWalk) {
      const bool in = q0 + (int)threadIdx.x < Sq;  // a row past Sq: lse = +inf, p exactly 0
      lses[threadIdx.x] = in ? lse[(long)bh * Sq + q0 + threadIdx.x] : INFINITY;
      deltas[threadIdx.x] = in ? delta[(long)bh * Sq + q0 + threadIdx.x] : 0.f;
    }
    __syncthreads();
    if (!active) continue;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const f32x16 s = score_block<D>(qs, 32 * qb, i, half, kf);   // (q k^T)[query][key]
      const f32x16 dp = score_block<D>(gs, 32 * qb, i, half, vf);  // (dO v^T)[query][key]
      f32x16 p, ds;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qi = 32 * qb + 8 * (r >> 2) + 4 * half + (r & 3);
        p[r] = mine ? expf(s[r] * scale - lses[qi]) : 0.f;
        ds[r] = p[r] * (dp[r] - deltas[qi]);
      }
      accum_block<D>(gs, 32 * qb, i, half, p, dva);   // dv^T += dO^T p
      accum_block<D>(qs, 32 * qb, i, half, ds, dka);  // dk^T += q^T dS
    }
  }
  if (mine) {
    store_own<D>(const_cast<float*>(head_of(dk, b, hd)) + (long)krow * dk.ss, half, dka, scale);
    store_own<D>(const_cast<float*>(head_of(dv, b, hd)) + (long)krow * dv.ss, half, dva, 1.f);
  }
}

// ----------------------------------------------------------------------------------- copy4d
// any-stride [B][H][S][D] -> dense [B][S][H][D]
__global__ __launch_bounds__(kAttnThreads) void attn_copy4d_kernel(
    const float* __restrict__ src, long sb, long sh, long ss, long sd, float* __restrict__ dst,
    int H, int S, int D, long total) {
  for (long idx = (long)blockIdx.x * kAttnThreads + threadIdx.x; idx < total;
       idx += (long)gridDim.x * kAttnThreads) {
    const int d = (int)(idx % D);
    long r = idx / D;
    const int h = (int)(r % H);
    r /= H;
    const int s = (int)(r % S);
    const long b = r / S;
    dst[idx] = src[b * sb + h * sh + s * ss + d * sd];
  }
}

}  // namespace

void attn_fwd(const AttnT& q, const AttnT& k, const AttnT& v, const AttnT& o, float* lse, int B,
              int H, int Sq, int Sk, int D, float scale, hipStream_t s) {
  const dim3 grid(ceil_div(Sq, kOwn), B * H);
  if (D == 64)
    attn_fwd_kernel<64><<<grid, kAttnThreads, 0, s>>>(q, k, v, o, lse, H, Sq, Sk, scale);
  else
    attn_fwd_kernel<32><<<grid, kAttnThreads, 0, s>>>(q, k, v, o, lse, H, Sq, Sk, scale);
}

void attn_bwd(const AttnT& dout, const AttnT& q, const AttnT& k, const AttnT& v, const AttnT& o,
              const float* lse, float* delta, const AttnT& dq, const AttnT& dk, const AttnT& dv,
              int B, int H, int Sq, int Sk, int D, float scale, hipStream_t s) {
  float* delta_k = delta + (long)B * H * Sq;
  const dim3 qgrid(ceil_div(Sq, kOwn), B * H), kgrid(ceil_div(Sk, kOwn), B * H);
  if (D == 64) {
    attn_delta_kernel<64><<<qgrid, kAttnThreads, 0, s>>>(dout, o, delta, delta_k, H, Sq);
    attn_bwd_dq_kernel<64><<<qgrid, kAttnThreads, 0, s>>>(dout, q, k, v, lse, delta, dq, H, Sq,
                                                          Sk, scale);
    attn_bwd_dkv_kernel<64><<<kgrid, kAttnThreads, 0, s>>>(dout, q, k, v, lse, delta_k, dk, dv,
                                                           H, Sq, Sk, scale);
  } else {
    attn_delta_kernel<32><<<qgrid, kAttnThreads, 0, s>>>(dout, o, delta, delta_k, H, Sq);
    attn_bwd_dq_kernel<32><<<qgrid, kAttnThreads, 0, s>>>(dout, q, k, v, lse, delta, dq, H, Sq,
                                                          Sk, scale);
    attn_bwd_dkv_kernel<32><<<kgrid, kAttnThreads, 0, s>>>(dout, q, k, v, lse, delta_k, dk, dv,
                                                           H, Sq, Sk, scale);
  }
}

void attn_copy4d(const float* src, long sb, long sh, long ss, long sd, float* dst, int B, int H,
                 int S, int D, hipStream_t s) {
  const long total = (long)B * H * S * D;
  const int grid = (int)std::min<long>(ceil_div(total, kAttnThreads), 4096);
  attn_copy4d_kernel<<<grid, kAttnThreads, 0, s>>>(src, sb, sh, ss, sd, dst, H, S, D, total);
}

}  // namespace tdp
