// Per-sample augmentation of a uint8 NHWC batch (TrivialAugmentWide's op set), gfx950, out of
// place. params [N][8] int32 = (op, a0..a5, 0); sample n depends on sample n alone. The rules
// (kernels.h has the table) are integer, or fp32 with every operation rounded on its own: _build.py
// compiles this file with -ffp-contract=off (a pragma here would be disregarded under the other
// files' =fast), so f*a + g*b is two multiplies and an add as in eager torch, and the result
// equals data/augment.py's reference_augment bit for bit.
//
// Two launches, both with blockIdx.y = sample, so the sample's op and arguments are workgroup-
// uniform and come in through scalar loads; neither depends on N, allocates or synchronises.
//
// augment_stats_kernel, grid (chunks, N). Contrast, AutoContrast and Equalize all follow from
// 256-bin integer histograms (Contrast: of gray, sum = sum k hist[k]; the others: per channel).
// A workgroup whose sample needs none returns at once; the others histogram `rpc` rows in LDS with
// LDS integer atomics and write the partial to ws[n][chunk][slot][256] (slot = channel, 3 = gray)
// with plain stores: integer sums are exact in any order, nothing is zeroed beforehand and no
// global atomic is used. Only the slots the op needs are written, and only those are read later.
//
// augment_apply_kernel, grid (tiles, N), one workgroup-uniform switch, three paths:
//   byte table (Brightness, Contrast, Posterize, Solarize, AutoContrast, Equalize): each is a
//     per-channel 256-entry table once the statistics are known. The workgroup merges the partial
//     histograms chunk by chunk (thread k owns bin k), builds C x 256 bytes of table in LDS
//     (Contrast: a 64-bit tree sum; AutoContrast: LDS min / max; Equalize: a 256-wide scan) and
//     streams its byte range through it. The channel of a byte is (offset in the sample) % C, so
//     16-byte units need no pixel decoding. Identity is the same stream without a table.
//   pixel (Color): groups of 4 whole pixels, gray per pixel.
//   tile (Affine, Sharpness): a 16 x 64 output tile, 4 consecutive pixels of one row per thread.
//     Sharpness stages the tile plus a one-pixel halo in LDS; Affine evaluates U, V once per
//     thread in int64, steps them by 2 m0, 2 m3 per column and gathers from global memory, where
//     a source position outside the image selects 0 and is never read.
// Streams take 16-byte units where source and destination share their alignment (bytes up to the
// first boundary, 16-byte units, bytes after the last), single bytes otherwise; pixel groups take
// 4-byte words where the group's address allows. An unknown op, a statistics op without a
// workspace, Color on one channel and Sharpness on an image under 3 x 3 are Identity.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace tdp {
namespace {

constexpr int kT = 256;
constexpr int kTileH = 16, kTileW = 64, kPx = 4;  // 16 rows x 16 groups of 4 pixels = 256 threads
constexpr int kHaloW = kTileW + 2, kHaloH = kTileH + 2;
constexpr int kStatRange = 32768;  // bytes per workgroup on the table path of a statistics op

enum AugOp : int {
  kIdentity = 0, kAffine = 1, kBrightness = 2, kColor = 3, kContrast = 4, kSharpness = 5,
  kPosterize = 6, kSolarize = 7, kAutoContrast = 8, kEqualize = 9
};

struct AugParams {
  const uint8_t* x;
  uint8_t* out;
  const int* params;
  uint32_t* ws;  // [N][chunks][4][256] or nullptr
  int H, W, C;
  int L, HW;        // bytes / pixels per sample (< 2^31)
  int chunks, rpc;  // statistics chunks per sample, rows per chunk
  int tiles_x, T;   // apply grid: T = tiles_y * tiles_x workgroups per sample
};

__device__ __forceinline__ uint32_t trunc8(float t) {
  return (uint32_t)(int)fminf(fmaxf(t, 0.f), 255.f);
}

__device__ __forceinline__ uint32_t blend8(float a, float b, float f, float omf) {
  return trunc8(f * a + omf * b);
}

__device__ __forceinline__ uint32_t gray8(uint32_t r, uint32_t g, uint32_t b) {
  return trunc8(0.2989f * (float)r + 0.587f * (float)g + 0.114f * (float)b);
}

__device__ __forceinline__ bool needs_stats(int op) {
  return op == kContrast || op == kAutoContrast || op == kEqualize;
}

// Up to 12 bytes (kPx pixels) at p into w[0..2], byte k of the group in bits 8 (k % 4) of
// w[k / 4]; bytes past nbytes are never read.
__device__ __forceinline__ void load_group(const uint8_t* p, int nbytes, int full, uint32_t w[3]) {
  w[0] = w[1] = w[2] = 0;
  if (nbytes == full && ((uintptr_t)p & 3) == 0) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    w[0] = q[0];
    if (full == 12) { w[1] = q[1]; w[2] = q[2]; }
  } else {
    for (int k = 0; k < nbytes; ++k) w[k >> 2] |= (uint32_t)p[k] << ((k & 3) * 8);
  }
}

__device__ __forceinline__ void store_group(uint8_t* p, int nbytes, int full, const uint32_t w[3]) {
  if (nbytes == full && ((uintptr_t)p & 3) == 0) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = w[0];
    if (full == 12) { q[1] = w[1]; q[2] = w[2]; }
  } else {
    for (int k = 0; k < nbytes; ++k) p[k] = (uint8_t)(w[k >> 2] >> ((k & 3) * 8));
  }
}

__device__ __forceinline__ uint32_t group_byte(const uint32_t w[3], int k) {
  return (w[k >> 2] >> ((k & 3) * 8)) & 255u;
}

__device__ __forceinline__ void group_set(uint32_t w[3], int k, uint32_t v) {
  w[k >> 2] |= v << ((k & 3) * 8);
}

// ------------------------------------------------------------------------------------ statistics
__global__ __launch_bounds__(kT) void augment_stats_kernel(AugParams p) {
  const int n = blockIdx.y;
  const int op = p.params[8 * n];
  if (!needs_stats(op)) return;
  __shared__ uint32_t hist[3 * 256];
  const int tid = threadIdx.x;
  const int C = p.C;
  hist[tid] = hist[256 + tid] = hist[512 + tid] = 0;
  __syncthreads();
  const uint8_t* src = p.x + (long)n * p.L;
  const int row0 = blockIdx.x * p.rpc;
  const int row1 = min(p.H, row0 + p.rpc);
  const int px0 = row0 * p.W, px1 = row1 * p.W;  // this chunk's pixels, px0 < px1 <= HW
  if (op == kContrast) {
    const int full = kPx * C;
    const int g0 = px0 / kPx, g1 = (px1 + kPx - 1) / kPx;  // groups may straddle chunk ends
    for (int g = g0 + tid; g < g1; g += kT) {
      const int q0 = g * kPx;
      const int npx = min(kPx, p.HW - q0);
      uint32_t w[3];
      load_group(src + (long)q0 * C, npx * C, full, w);
      for (int q = 0; q < npx; ++q) {
        if (q0 + q < px0 || q0 + q >= px1) continue;  // the neighbour chunk counts that pixel
        const uint32_t gr = C == 3 ? gray8(group_byte(w, 3 * q), group_byte(w, 3 * q + 1),
                                           group_byte(w, 3 * q + 2))
                                   : group_byte(w, q);
        atomicAdd(&hist[gr], 1u);
      }
    }
  } else {
    const int r0 = px0 * C, r1 = px1 * C;  // byte range; the channel of byte e is e % C
    const int len = r1 - r0;
    const int head = min(len, (int)((16 - ((uintptr_t)(src + r0) & 15)) & 15));
    const int nunits = (len - head) >> 4;
    const int tail0 = r0 + head + (nunits << 4);
    for (int e = r0 + tid; e < r0 + head; e += kT)
      atomicAdd(&hist[(C == 3 ? e % 3 : 0) * 256 + src[e]], 1u);
    for (int u = tid; u < nunits; u += kT) {
      const int e = r0 + head + (u << 4);
      const uint4 v = *reinterpret_cast<const uint4*>(src + e);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      int c = C == 3 ? e % 3 : 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        atomicAdd(&hist[c * 256 + ((w[k >> 2] >> ((k & 3) * 8)) & 255u)], 1u);
        c = C == 3 ? (c == 2 ? 0 : c + 1) : 0;
      }
    }
    for (int e = tail0 + tid; e < r1; e += kT)
      atomicAdd(&hist[(C == 3 ? e % 3 : 0) * 256 + src[e]], 1u);
  }
  __syncthreads();
  uint32_t* o = p.ws + ((long)n * p.chunks + blockIdx.x) * 1024;
  if (op == kContrast) {
    o[3 * 256 + tid] = hist[tid];
  } else {
    for (int c = 0; c < C; ++c) o[c * 256 + tid] = hist[c * 256 + tid];
  }
}

// ----------------------------------------------------------------------------------------- apply
// Bytes [r0, r1) of the sample through tab (LDS, [C][256]) or, without one, copied.
template <bool TABLE>
__device__ __forceinline__ void stream_bytes(const uint8_t* src, uint8_t* dst, int r0, int r1,
                                             const uint8_t* tab, int C) {
  const int tid = threadIdx.x;
  const int len = r1 - r0;
  const bool vec = (((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0;
  const int head = vec ? min(len, (int)((16 - ((uintptr_t)(src + r0) & 15)) & 15)) : len;
  const int nunits = (len - head) >> 4;
  const int tail0 = r0 + head + (nunits << 4);
  for (int e = r0 + tid; e < r0 + head; e += kT)
    dst[e] = TABLE ? tab[(C == 3 ? e % 3 : 0) * 256 + src[e]] : src[e];
  for (int u = tid; u < nunits; u += kT) {
    const int e = r0 + head + (u << 4);
    uint4 v = *reinterpret_cast<const uint4*>(src + e);
    if constexpr (TABLE) {
      uint32_t w[4] = {v.x, v.y, v.z, v.w}, r[4] = {0, 0, 0, 0};
      int c = C == 3 ? e % 3 : 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        r[k >> 2] |= (uint32_t)tab[c * 256 + ((w[k >> 2] >> ((k & 3) * 8)) & 255u)]
                     << ((k & 3) * 8);
        c = C == 3 ? (c == 2 ? 0 : c + 1) : 0;
      }
      v = make_uint4(r[0], r[1], r[2], r[3]);
    }
    *reinterpret_cast<uint4*>(dst + e) = v;
  }
  for (int e = tail0 + tid; e < r1; e += kT)
    dst[e] = TABLE ? tab[(C == 3 ? e % 3 : 0) * 256 + src[e]] : src[e];
}

// Bin `tid` of histogram `slot`, merged over the chunks in index order.
__device__ __forceinline__ uint32_t merged_bin(const AugParams& p, int n, int slot) {
  const uint32_t* w = p.ws + (long)n * p.chunks * 1024 + slot * 256 + threadIdx.x;
  uint32_t h = 0;
  for (int ch = 0; ch < p.chunks; ++ch) h += w[ch * 1024];
  return h;
}

__global__ __launch_bounds__(kT) void augment_apply_kernel(AugParams p) {
  __shared__ uint8_t tab[3 * 256];
  __shared__ uint8_t tile[kHaloH * kHaloW * 3];
  __shared__ unsigned long long red[256];
  __shared__ uint32_t scan[2][256];
  __shared__ int lohi[2];

  const int n = blockIdx.y, tid = threadIdx.x, wg = blockIdx.x;
  const int* a = p.params + 8 * n;
  const int C = p.C, H = p.H, W = p.W;
  int op = a[0];
  if (op < 0 || op > kEqualize || (needs_stats(op) && p.ws == nullptr) ||
      (op == kColor && C != 3) || (op == kSharpness && (H < 3 || W < 3)))
    op = kIdentity;
  const uint8_t* src = p.x + (long)n * p.L;
  uint8_t* dst = p.out + (long)n * p.L;
  const float f = __int_as_float(a[1]);
  const float omf = 1.f - f;

  switch (op) {
    case kBrightness: case kContrast: case kPosterize: case kSolarize: case kAutoContrast:
    case kEqualize: {
      // the byte range first: a workgroup without one builds no table
      const int nb = needs_stats(op) ? min(p.T, (p.L + kStatRange - 1) / kStatRange) : p.T;
      const int R = (((p.L + nb - 1) / nb) + 15) & ~15;
      const long r0 = (long)wg * R;
      if (wg >= nb || r0 >= p.L) return;
      const int r1 = (int)min((long)p.L, r0 + R);
      const uint32_t k = tid;
      if (op == kBrightness) {
        const uint32_t v = blend8((float)k, 0.f, f, omf);
        for (int c = 0; c < C; ++c) tab[c * 256 + k] = (uint8_t)v;
      } else if (op == kPosterize) {
        const int bits = min(max(a[1], 0), 8);
        const uint32_t v = k & (0xFFu << (8 - bits)) & 0xFFu;
        for (int c = 0; c < C; ++c) tab[c * 256 + k] = (uint8_t)v;
      } else if (op == kSolarize) {
        const uint32_t v = (float)k >= f ? 255u - k : k;
        for (int c = 0; c < C; ++c) tab[c * 256 + k] = (uint8_t)v;
      } else if (op == kContrast) {
        red[k] = (unsigned long long)k * merged_bin(p, n, 3);
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
          if (tid < s) red[tid] += red[tid + s];
          __syncthreads();
        }
        const float mean = (float)((double)red[0] / (double)p.HW);
        const uint32_t v = blend8((float)k, mean, f, omf);
        for (int c = 0; c < C; ++c) tab[c * 256 + k] = (uint8_t)v;
      } else {
        for (int c = 0; c < C; ++c) {
          const uint32_t h = merged_bin(p, n, c);
          if (tid == 0) { lohi[0] = 256; lohi[1] = -1; }
          scan[0][k] = h;
          __syncthreads();
          if (h) { atomicMin(&lohi[0], (int)k); atomicMax(&lohi[1], (int)k); }
          __syncthreads();
          const int lo = lohi[0], hi = lohi[1];
          uint32_t v = k;
          if (op == kAutoContrast) {
            if (hi > lo) {
              // one IEEE division, as torch's: _build.py pins correctly rounded fp32 division
              const float scale = 255.0f / (float)(hi - lo);
              v = trunc8((float)((int)k - lo) * scale);
            }
          } else {
            const uint32_t step = ((uint32_t)p.HW - scan[0][max(hi, 0)]) / 255u;
            // inclusive scan of the 256 bins (Hillis-Steele, two buffers)
            int cur = 0;
            for (int d = 1; d < 256; d <<= 1) {
              const uint32_t s = scan[cur][k] + (k >= (uint32_t)d ? scan[cur][k - d] : 0u);
              scan[cur ^ 1][k] = s;
              cur ^= 1;
              __syncthreads();
            }
            const uint32_t below = scan[cur][k] - h;  // hist[0] + ... + hist[k-1]
            if (step) v = k == 0 ? 0u : min(255u, (below + step / 2) / step);
          }
          tab[c * 256 + k] = (uint8_t)v;
          __syncthreads();  // lohi and scan are reused by the next channel
        }
      }
      __syncthreads();
      stream_bytes<true>(src, dst, (int)r0, r1, tab, C);
      return;
    }
    case kColor: {
      const int ng = (p.HW + kPx - 1) / kPx;
      const int gpw = (ng + p.T - 1) / p.T;
      const long g0 = (long)wg * gpw;
      const int g1 = (int)min((long)ng, g0 + gpw);
      for (long g = g0 + tid; g < g1; g += kT) {
        const int q0 = (int)g * kPx;
        const int npx = min(kPx, p.HW - q0);
        uint32_t w[3], r[3] = {0, 0, 0};
        load_group(src + (long)q0 * 3, npx * 3, 12, w);
#pragma unroll
        for (int q = 0; q < kPx; ++q) {
          const uint32_t cr = group_byte(w, 3 * q), cg = group_byte(w, 3 * q + 1),
                         cb = group_byte(w, 3 * q + 2);
          const float gr = (float)gray8(cr, cg, cb);
          group_set(r, 3 * q, blend8((float)cr, gr, f, omf));
          group_set(r, 3 * q + 1, blend8((float)cg, gr, f, omf));
          group_set(r, 3 * q + 2, blend8((float)cb, gr, f, omf));
        }
        store_group(dst + (long)q0 * 3, npx * 3, 12, r);
      }
      return;
    }
    case kAffine: case kSharpness: {
      const int ti = wg / p.tiles_x, tj = wg - ti * p.tiles_x;
      const int i0 = ti * kTileH, j0t = tj * kTileW;
      const int i = i0 + (tid >> 4), j0 = j0t + (tid & 15) * kPx;
      const int rowb = W * C;  // bytes per image row
      if (op == kSharpness) {
        // tile + halo: LDS row rr is image row i0 - 1 + rr, LDS byte col is (j0t - 1) * C + ...
        const int lrow = kHaloW * C;
        for (int idx = tid; idx < kHaloH * lrow; idx += kT) {
          const int rr = idx / lrow, rem = idx - rr * lrow;
          const int gi = i0 - 1 + rr, gb = (j0t - 1) * C + rem;
          tile[idx] = (gi >= 0 && gi < H && gb >= 0 && gb < rowb) ? src[(long)gi * rowb + gb]
                                                                   : (uint8_t)0;
        }
        __syncthreads();
      }
      if (i >= H || j0 >= W) return;
      const int npx = min(kPx, W - j0);
      uint32_t r[3] = {0, 0, 0};
      if (op == kSharpness) {
        const int lrow = kHaloW * C;
        const uint8_t* t0 = tile + (tid >> 4) * lrow + (tid & 15) * kPx * C;  // row i-1, col j0-1
        const bool rin = i > 0 && i < H - 1;
        for (int c = 0; c < C; ++c) {
          uint32_t cs[kPx + 2], ctr[kPx + 2];
#pragma unroll
          for (int k = 0; k < kPx + 2; ++k) {
            ctr[k] = t0[lrow + k * C + c];
            cs[k] = (uint32_t)t0[k * C + c] + ctr[k] + (uint32_t)t0[2 * lrow + k * C + c];
          }
#pragma unroll
          for (int q = 0; q < kPx; ++q) {
            const int j = j0 + q;
            const uint32_t pc = ctr[q + 1];
            const uint32_t tsum = cs[q] + cs[q + 1] + cs[q + 2] + 4u * pc;
            const uint32_t blur = (rin && j > 0 && j < W - 1) ? (2u * tsum + 13u) / 26u : pc;
            group_set(r, q * C + c, blend8((float)pc, (float)blur, f, omf));
          }
        }
      } else {
        const long m0 = a[1], m1 = a[2], m2 = a[3], m3 = a[4], m4 = a[5], m5 = a[6];
        const long u = 2L * j0 + 1 - W, v = 2L * i + 1 - H;
        long U = m0 * u + m1 * v + m2 + ((long)W << 16);
        long V = m3 * u + m4 * v + m5 + ((long)H << 16);
        for (int q = 0; q < npx; ++q) {
          const long sx = U >> 17, sy = V >> 17;
          if (sx >= 0 && sx < W && sy >= 0 && sy < H) {
            const uint8_t* s = src + (sy * W + sx) * C;
            for (int c = 0; c < C; ++c) group_set(r, q * C + c, s[c]);
          }
          U += 2 * m0;
          V += 2 * m3;
        }
      }
      store_group(dst + ((long)i * W + j0) * C, npx * C, kPx * C, r);
      return;
    }
    default: {  // Identity
      const int R = (((p.L + p.T - 1) / p.T) + 15) & ~15;
      const long r0 = (long)wg * R;
      if (r0 >= p.L) return;
      stream_bytes<false>(src, dst, (int)r0, (int)min((long)p.L, r0 + R), nullptr, C);
      return;
    }
  }
}

AugParams make_params(const uint8_t* x, const int* params, uint32_t* ws, uint8_t* out, int H,
                      int W, int C) {
  AugParams p{};
  p.x = x; p.out = out; p.params = params; p.ws = ws;
  p.H = H; p.W = W; p.C = C;
  p.HW = H * W;
  p.L = H * W * C;
  p.chunks = image_augment_chunks(H, W);
  p.rpc = (H + p.chunks - 1) / p.chunks;
  p.tiles_x = ceil_div(W, kTileW);
  p.T = ceil_div(H, kTileH) * p.tiles_x;
  return p;
}

}  // namespace

int image_augment_chunks(int H, int W) {
  const long want = std::min<long>(8, std::max<long>(1, ((long)H * W + 4095) / 4096));
  const long rpc = (H + want - 1) / want;
  return (int)((H + rpc - 1) / rpc);
}

void image_augment_stats(const uint8_t* x, const int* params, uint32_t* ws, int N, int H, int W,
                         int C, hipStream_t s) {
  const AugParams p = make_params(x, params, ws, nullptr, H, W, C);
  hipLaunchKernelGGL(augment_stats_kernel, dim3((unsigned)p.chunks, (unsigned)N), dim3(kT), 0, s,
                     p);
}

void image_augment_apply(const uint8_t* x, const int* params, const uint32_t* ws, uint8_t* out,
                         int N, int H, int W, int C, hipStream_t s) {
  const AugParams p = make_params(x, params, const_cast<uint32_t*>(ws), out, H, W, C);
  hipLaunchKernelGGL(augment_apply_kernel, dim3((unsigned)p.T, (unsigned)N), dim3(kT), 0, s, p);
}

}  // namespace tdp
