// The split-bf16 primitives every fp32-on-the-bf16-matrix-core kernel shares: the exact three-way
// split, the six-product MFMA, the plane store, and the LDS-DMA helpers of the K-tile pipelines.
// One definition each, so the GEMMs (gemm_f32_fast, gemm_emu8, gemm_planes) and the producers that
// emit bf16 planes of their output (gemm_planes, gemm_skinny, norm) are bit-identical by
// construction: tests/test_gemm_planes_gpu.py compares the planes path with the in-kernel split
// bitwise.
//
// The residual subtractions of the split must stay scalar v_sub_f32: packed f32 VALU
// (v_pk_add_f32) costs ~4x the issue slot beside MFMAs. A header is compiled per translation
// unit, so that holds through each including file's own flags: _build.py gives the GEMMs whose
// K loop splits (gemm_f32_fast, gemm_planes, gemm_emu8) -fno-slp-vectorize.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace tdp {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef char lds_char;  // generic pointer into the dynamic LDS array (reads infer ds_read)

// ---- fp32 GEMM on the bf16 matrix core -------------------------------------------------------
// gfx950 runs v_mfma_f32_32x32x2_f32 at 1/16 of the bf16 rate (64 vs 1024 FLOP/clk/SIMD). An
// fp32 operand splits EXACTLY into three bf16 terms x = x0 + x1 + x2 (x0 = RNE_bf16(x),
// x1 = RNE_bf16(x - x0), x2 = x - x0 - x1: 24 significand bits = 3 x 8, every subtraction exact),
// so a*b = sum_ij a_i b_j with the six terms of weight >= 2^-16 kept and a1b2 + a2b1 + a2b2
// (<= ~2^-24 |a||b|, the size of one fp32 rounding of the product) dropped. Each bf16 x bf16
// product is exact in the fp32 accumulator, so the result carries fp32 accuracy (error bound
// tested against fp64 next to the native f32 MFMA path: tests/test_gemm_emu_gpu.py) at 6 x 32
// instead of 8 x 64 cycles per 32x32x16 step: a 2.67x higher matrix-core ceiling. The split
// runs on the VALU from the SAME fp32 LDS fragments the f32 path reads (v_cvt_pk_bf16_f32 does
// the RNE pair conversion), and overlaps the previous step's MFMAs.
// K order: the bf16 MFMA gives lane half h the k-slots 8h..8h+7; the f32 fragment reads give
// lane half h the k = 8q + 4h + s (s < 4) of two consecutive q -- the same permutation for A and
// B, so the dot products are unchanged.

// the pair split: (x0, x1) -> packed bf16 hi / mid / lo words
__device__ __forceinline__ void split3_bits(float x0, float x1, unsigned& h, unsigned& m,
                                            unsigned& l) {
  const unsigned hu = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, bf2));
  const float r0 = x0 - __uint_as_float(hu << 16), r1 = x1 - __uint_as_float(hu & 0xffff0000u);
  const unsigned mu = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{r0, r1}, bf2));
  const float s0 = r0 - __uint_as_float(mu << 16), s1 = r1 - __uint_as_float(mu & 0xffff0000u);
  h = hu;
  m = mu;
  l = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{s0, s1}, bf2));
}

// 8 fp32 (one lane's k-slots of a 32x32x16 step) -> three bf16x8 MFMA operands
__device__ __forceinline__ void split3_x8(float x0, float x1, float x2, float x3, float x4,
                                          float x5, float x6, float x7, bf8& h, bf8& m, bf8& l) {
  unsigned hs[4], ms[4], ls[4];
  split3_bits(x0, x1, hs[0], ms[0], ls[0]);
  split3_bits(x2, x3, hs[1], ms[1], ls[1]);
  split3_bits(x4, x5, hs[2], ms[2], ls[2]);
  split3_bits(x6, x7, hs[3], ms[3], ls[3]);
  h = __builtin_bit_cast(bf8, u32x4{hs[0], hs[1], hs[2], hs[3]});
  m = __builtin_bit_cast(bf8, u32x4{ms[0], ms[1], ms[2], ms[3]});
  l = __builtin_bit_cast(bf8, u32x4{ls[0], ls[1], ls[2], ls[3]});
}
// ... from two f32 k-steps of 4
__device__ __forceinline__ void split3_x8(const float (&a)[4], const float (&b)[4], bf8& h,
                                          bf8& m, bf8& l) {
  split3_x8(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], h, m, l);
}
__device__ __forceinline__ void split3_x8(const f32x4& a, const f32x4& b, bf8& h, bf8& m,
                                          bf8& l) {
  split3_x8(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], h, m, l);
}
__device__ __forceinline__ void split3_x8(const float (&x)[8], bf8& h, bf8& m, bf8& l) {
  split3_x8(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], h, m, l);
}

// acc += a*b over the six kept split terms (smallest first)
__device__ __forceinline__ f32x16 mfma_emu6(const bf8& ah, const bf8& am, const bf8& al,
                                            const bf8& bh, const bf8& bm, const bf8& bl,
                                            f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
  return acc;
}

// four adjacent values -> their planes at o, o + ps, o + 2 ps (8-B stores): the representation
// the planes GEMM (gemm_planes.hip) reads its activation operand in. Producers that write an
// activation for a skinny Linear emit the three planes next to the fp32 tensor.
__device__ __forceinline__ void store_planes4(uint16_t* o, long ps, float v0, float v1, float v2,
                                              float v3) {
  unsigned h0, m0, l0, h1, m1, l1;
  split3_bits(v0, v1, h0, m0, l0);
  split3_bits(v2, v3, h1, m1, l1);
  *reinterpret_cast<u32x2*>(o) = u32x2{h0, h1};
  *reinterpret_cast<u32x2*>(o + ps) = u32x2{m0, m1};
  *reinterpret_cast<u32x2*>(o + 2 * ps) = u32x2{l0, l1};
}

// ---- K-tile pipeline helpers ------------------------------------------------------------------
// 16 B per lane global -> LDS (global_load_lds_dwordx4: no VGPR staging, no ds_write)
__device__ __forceinline__ void glds16(const void* src, lds_char* dst) {
  __builtin_amdgcn_global_load_lds(
      src, (void __attribute__((address_space(3)))*)(
               (__attribute__((address_space(3))) char*)dst), 16, 0, 0);
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Row swizzle of K-contiguous fp32 tiles ([rows][32 k], 128-B rows): slot(row, chunk) =
// chunk ^ kswz(row). XOR-ing in row bits 3-5 makes every 16-lane group of a ds_read_b128 (rows
// r..r+31 of one fragment) hit 16 distinct (row parity, slot) pairs = all 64 banks:
// conflict-free (plain `row & 7` left a 2-way conflict, SQ_LDS_BANK_CONFLICT = 4 cycles per read
// in the first profile).
__device__ __forceinline__ int kswz(int row) { return (row ^ (row >> 3)) & 7; }

}  // namespace tdp
