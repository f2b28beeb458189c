// ToTensor + Normalize + RandomErasing in one launch, gfx950: uint8 [N][H][W][C] -> float32
// [N][C][H][W], plain contiguous (planar) or channels_last. It is the last step of
// crop (uint8) -> augment (uint8) -> this, torchvision's order, and the place to erase: the erased
// elements are never normalised, they are simply written as something else.
//
// Contract per element (n, c, i, j). Outside sample n's box: image_normalize(x, mean[c],
// inv_std[c]), the crop kernel's own expression (image_norm.h), so the uint8 crop followed by this
// kernel gives the float crop's bits. Inside: fill.value[c] as given (kEraseConst), or
// (kEraseRandom) z = sqrtf(-2 logf((u1 + 1) 2^-32)) * cosf(2 pi (u2 2^-32)), u1 / u2 = lane e & 3
// of Philox4x32-10 with key (seed_lo, seed_hi) and counter (e >> 2 low, e >> 2 high,
// n + n_offset, 0 / 1), e = (c H + i) W + j; u -> float, + 1, the scalings, the product with
// 2 pi, logf, sqrtf, cosf and the last product are each one rounded fp32 operation: _build.py
// compiles this file with -ffp-contract=off. z depends on (seed, n, c, i, j) alone: not on the
// layout, the grid or the rest of the batch.
//
// Design. grid (strips, N): blockIdx.y is the sample, so its box, mean and std are uniform
// (scalar) loads, and a 256-thread workgroup owns a strip of whole rows, i.e. one contiguous byte
// range of the sample. Whether the strip's rows meet the (clamped) box is a workgroup-uniform
// test: a strip that does not takes the instantiation with no box test and no Philox code at all.
// Bytes are read as 16-byte units where the address allows (single bytes up to the first
// boundary and after the last, so an unaligned base or W C % 16 != 0 costs a few byte loads).
//   channels_last  output element order is the input byte order: a thread turns one 16-byte unit
//                  into four float4 stores (scalar stores where the output is not 16-byte aligned).
//   planar         the strip goes through LDS kSegPx pixels at a time, placed at the global
//                  address's offset mod 16 so the LDS stores stay aligned; then one item = 4
//                  consecutive pixels of one channel, items of a plane on consecutive threads:
//                  strided byte reads from LDS, one float4 per item into the plane, so every plane
//                  is written in coalesced 1 KB pieces per wavefront. Items are aligned to the
//                  absolute pixel index; ragged groups and misaligned planes (H W % 4 != 0) take
//                  scalar stores.
// Philox runs only for elements inside the box, and once per four elements where they share
// e >> 2 (planar, H W % 4 == 0). No atomics, no scratch, every element written exactly once.
#include <algorithm>

#include "common.h"
#include "image_norm.h"
#include "kernels.h"

namespace tdp {
namespace {

constexpr int kT = 256;
constexpr int kStripPx = 4096;  // pixels a workgroup aims for (whole rows, at least one)
constexpr int kSegPx = 2048;    // pixels of the strip in LDS at once (planar): 8 KB at C = 4

struct FinishParams {
  const uint8_t* x;
  const int* box;  // [N][4] or nullptr
  float* out;
  int H, W, HW, rps;  // rps = rows per strip
  ImageNorm nrm;
  EraseFill fill;
};

// Four per-channel values as scalars, chosen by selects: a runtime index into an array of the
// kernel's arguments would move the arguments to scratch.
template <typename T>
struct Quad {
  T v0, v1, v2, v3;
  __device__ __forceinline__ T operator()(int c) const {
    return c == 0 ? v0 : c == 1 ? v1 : c == 2 ? v2 : v3;
  }
};
using Quadf = Quad<float>;
using Quadu = Quad<uint32_t>;

__device__ __forceinline__ Quadf quad(const float (&a)[4]) { return {a[0], a[1], a[2], a[3]}; }

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, Quadu& r) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0;
    const uint32_t h1 = __umulhi(M1, c2), l1 = M1 * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += W0;
    k1 += W1;
  }
  r = {c0, c1, c2, c3};
}

// The fill of the elements inside the box; for kEraseRandom it keeps the last counter's eight
// outputs, so four elements that share e >> 2 cost one pair of Philox calls.
struct Filler {
  Quadf value;
  uint32_t seed_lo, seed_hi, n;
  int mode;
  unsigned long long ctr;
  Quadu a, b;

  __device__ __forceinline__ float operator()(int c, long e) {
    if (mode != kEraseRandom) return value(c);
    const unsigned long long q = (unsigned long long)e >> 2;
    if (q != ctr) {
      ctr = q;
      philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), n, 0u, seed_lo, seed_hi, a);
      philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), n, 1u, seed_lo, seed_hi, b);
    }
    const int lane = (int)(e & 3);
    const uint32_t r1 = a(lane), r2 = b(lane);
    const float u1 = ((float)r1 + 1.f) * 0x1p-32f;
    const float ang = 6.2831855f * ((float)r2 * 0x1p-32f);
    return sqrtf(-2.f * logf(u1)) * cosf(ang);
  }
};

struct Norm {
  Quadf mean, inv_std;
  __device__ __forceinline__ float operator()(uint32_t byte, int c) const {
    return image_normalize((float)byte, mean(c), inv_std(c));
  }
};

struct Box {
  int t0, t1, l0, l1;  // clamped to the image; empty when t0 >= t1 or l0 >= l1
  __device__ __forceinline__ bool has(int i, int j) const {
    return i >= t0 && i < t1 && j >= l0 && j < l1;
  }
};

// ------------------------------------------------------------------------------- channels_last
// Bytes [b0, b1) of the sample: out[e] for byte e. (c, i, j) of a byte are only formed when ERASE.
template <int C, bool ERASE>
__device__ __forceinline__ void finish_cl(const uint8_t* src, float* dst, int W, int HW, int b0,
                                          int b1, const Norm& nrm, const Box& bx, Filler& fill) {
  const int tid = threadIdx.x;
  const int len = b1 - b0;
  const int head = min(len, (int)((16 - ((uintptr_t)(src + b0) & 15)) & 15));
  const int nunits = (len - head) >> 4;
  const int tail0 = b0 + head + (nunits << 4);
  auto one = [&](int e) {
    const int px = e / C, c = e - px * C;
    float v = nrm(src[e], c);
    if constexpr (ERASE) {
      const int i = px / W, j = px - i * W;
      if (bx.has(i, j)) v = fill(c, (long)c * HW + px);
    }
    dst[e] = v;
  };
  for (int e = b0 + tid; e < b0 + head; e += kT) one(e);
  for (int e = tail0 + tid; e < b1; e += kT) one(e);
  for (int u = tid; u < nunits; u += kT) {
    const int e0 = b0 + head + (u << 4);
    const uint4 q = *reinterpret_cast<const uint4*>(src + e0);
    int px = e0 / C, c = e0 - px * C;
    int i = 0, j = 0;
    if constexpr (ERASE) { i = px / W; j = px - i * W; }
    float* d = dst + e0;
    const bool vec = ((uintptr_t)d & 15) == 0;
    auto word = [&](uint32_t w, int k0) {  // four bytes -> four floats
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = nrm((w >> (k * 8)) & 255u, c);
        if constexpr (ERASE) {
          if (bx.has(i, j)) v[k] = fill(c, (long)c * HW + px);
        }
        if (++c == C) {
          c = 0;
          ++px;
          if constexpr (ERASE) { if (++j == W) { j = 0; ++i; } }
        }
      }
      if (vec) {
        *reinterpret_cast<f32x4*>(d + k0) = f32x4{v[0], v[1], v[2], v[3]};
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k0 + k] = v[k];
      }
    };
    if constexpr (ERASE) {  // one copy of the fill code per byte lane, not sixteen
#pragma unroll 1
      for (int wq = 0; wq < 4; ++wq)
        word(wq == 0 ? q.x : wq == 1 ? q.y : wq == 2 ? q.z : q.w, 4 * wq);
    } else {
      word(q.x, 0); word(q.y, 4); word(q.z, 8); word(q.w, 12);
    }
  }
}

// -------------------------------------------------------------------------------------- planar
// Pixels [p0, p1) of the sample, p1 - p0 <= kSegPx: bytes to LDS, planes out.
template <int C, bool ERASE>
__device__ __forceinline__ void finish_planar(const uint8_t* src, float* dst, int W, int HW,
                                              int p0, int p1, uint8_t* tile, const Norm& nrm,
                                              const Box& bx, Filler& fill) {
  const int tid = threadIdx.x;
  const uint8_t* s = src + (long)p0 * C;
  const int len = (p1 - p0) * C;
  const int shift = (int)((uintptr_t)s & 15);  // LDS byte of s[k] is shift + k
  const int head = min(len, (16 - shift) & 15);
  const int nunits = (len - head) >> 4;
  const int tail0 = head + (nunits << 4);
  for (int k = tid; k < head; k += kT) tile[shift + k] = s[k];
  for (int k = tail0 + tid; k < len; k += kT) tile[shift + k] = s[k];
  for (int u = tid; u < nunits; u += kT) {
    const int k = head + (u << 4);
    *reinterpret_cast<uint4*>(tile + shift + k) = *reinterpret_cast<const uint4*>(s + k);
  }
  __syncthreads();
  const int q0 = p0 >> 2, nq = ((p1 + 3) >> 2) - q0;  // groups of 4 pixels, absolute alignment
  for (int it = tid; it < nq * C; it += kT) {
    const int c = it / nq, g = it - c * nq;
    const int pg = (q0 + g) << 2;
    const int a = max(pg, p0), b = min(pg + 4, p1);
    const float mean = nrm.mean(c), inv_std = nrm.inv_std(c);
    const uint8_t* t = tile + shift + (pg - p0) * C + c;  // only [a, b) is read
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    int i = 0, j = 0;
    if constexpr (ERASE) { i = a / W; j = a - i * W; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (pg + k >= a && pg + k < b) {
        v[k] = image_normalize((float)t[k * C], mean, inv_std);
        if constexpr (ERASE) {
          if (bx.has(i, j)) v[k] = fill(c, (long)c * HW + pg + k);
          if (++j == W) { j = 0; ++i; }
        }
      }
    }
    float* d = dst + (long)c * HW + pg;
    if (b - a == 4 && ((uintptr_t)d & 15) == 0) {
      *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (pg + k >= a && pg + k < b) d[k] = v[k];
    }
  }
  __syncthreads();  // the next segment overwrites the tile
}

template <int C, bool CL>
__global__ __launch_bounds__(kT) void image_normalize_erase_kernel(FinishParams p) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[CL ? 16 : kSegPx * C + 16];
  const int n = blockIdx.y;
  const int W = p.W, HW = p.HW;
  const int r0 = blockIdx.x * p.rps, r1 = min(p.H, r0 + p.rps);
  Box bx{0, 0, 0, 0};
  if (p.box != nullptr) {
    const int* b = p.box + 4 * n;
    const long top = b[0], left = b[1], h = b[2], w = b[3];
    if (h > 0 && w > 0) {
      bx.t0 = (int)max(top, 0L);
      bx.t1 = (int)min(top + h, (long)p.H);
      bx.l0 = (int)max(left, 0L);
      bx.l1 = (int)min(left + w, (long)W);
    }
  }
  const bool hit = bx.l0 < bx.l1 && max(bx.t0, r0) < min(bx.t1, r1);  // workgroup-uniform
  const long L = (long)HW * C;
  const uint8_t* src = p.x + n * L;
  float* dst = p.out + n * L;
  const Norm nrm{quad(p.nrm.mean), quad(p.nrm.inv_std)};
  Filler fill{quad(p.fill.value), p.fill.seed_lo, p.fill.seed_hi, (uint32_t)n + p.fill.n_offset,
              p.fill.mode, ~0ull, {}, {}};
  if constexpr (CL) {
    const int b0 = r0 * W * C, b1 = r1 * W * C;
    if (hit) finish_cl<C, true>(src, dst, W, HW, b0, b1, nrm, bx, fill);
    else finish_cl<C, false>(src, dst, W, HW, b0, b1, nrm, bx, fill);
  } else {
    const int pe = r1 * W;
    for (int p0 = r0 * W; p0 < pe; p0 += kSegPx) {
      const int p1 = min(p0 + kSegPx, pe);
      if (hit) finish_planar<C, true>(src, dst, W, HW, p0, p1, tile, nrm, bx, fill);
      else finish_planar<C, false>(src, dst, W, HW, p0, p1, tile, nrm, bx, fill);
    }
  }
}

template <int C, bool CL>
void launch_finish(const FinishParams& p, int N, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(p.H, p.rps), (unsigned)N);
  hipLaunchKernelGGL((image_normalize_erase_kernel<C, CL>), grid, dim3(kT), 0, s, p);
}

}  // namespace

void image_normalize_erase(const uint8_t* x, const int* box, float* out, int N, int H, int W,
                           int C, const ImageNorm& nrm, const EraseFill& fill, bool channels_last,
                           hipStream_t s) {
  if ((long)N * H * W <= 0) return;
  FinishParams p{};
  p.x = x; p.box = box; p.out = out;
  p.H = H; p.W = W; p.HW = H * W;
  p.rps = std::min(H, std::max(1, kStripPx / W));
  p.nrm = nrm;
  p.fill = fill;
#define TDP_FINISH(CC) \
  (channels_last ? launch_finish<CC, true>(p, N, s) : launch_finish<CC, false>(p, N, s))
  if (C == 3) TDP_FINISH(3);
  else if (C == 1) TDP_FINISH(1);
  else if (C == 4) TDP_FINISH(4);
#undef TDP_FINISH
}

}  // namespace tdp
