// Fused crop + antialiased resize + flip + normalise: torchvision's RandomResizedCrop /
// RandomCrop(padding) / CenterCrop -> RandomHorizontalFlip -> ToTensor -> Normalize, one launch
// per uint8 batch with a box (top, left, h, w) per sample. image.hip's 2-tap bilinear is only the
// right filter when upsampling; here the triangle filter's support grows with the scale, as in
// F.interpolate(mode="bilinear", antialias=True, align_corners=False).
//
// Contract. Sample b sees the virtual image V[i, j] = x[b, top+i, left+j] inside the source and
// `fill` outside, 0 <= i < h, 0 <= j < w; the box may hang over any edge. Per axis, resizing
// n_in -> n_out with s = n_in / n_out, support = max(s, 1) and centre c = (o + 0.5) s, tap j has
// weight max(0, 1 - |j - c + 0.5| / support), the taps are clipped to [0, n_in) (the box, never
// the source image) and the weights kept are divided by their sum. Then: one rintf of the fully
// filtered value if round_u8 (no rounding between the passes), the horizontal flip, and
// (v / 255 - mean[c]) * inv_std[c].
//
// Exact weights. With D = 2 max(n_in, n_out) and num(j) = (2j + 1) n_out - (2o + 1) n_in, the
// weight above is (D - |num(j)|) / D: an integer over a constant. The kernel carries the integer
// D - |num| (one add per tap, exact in fp32 up to D = 2^24), accumulates integer-weight * pixel
// and divides once by the integer weight sum. No fp32 centre is ever formed, so the tap positions
// carry no rounding error at any size, and a weight sum of one tap (identity resize) returns the
// pixel bitwise. The nonzero-weight taps are exactly |num(j)| < D; that set, found by integer
// floor division, is what the clipped [int(c - support + 0.5), int(c + support + 0.5)) range holds
// apart from taps whose weight is zero.
//
// Design. A 256-thread workgroup owns one 16x16 output tile of one sample (grid z = sample); the
// sample's box comes through uniform (scalar) loads of box[4b..4b+3].
//   setup    32 threads build the tile's tap tables in LDS: for each of its 16 output columns and
//            16 output rows the first / last tap, num of the first tap and the weight sum (the
//            normaliser), computed once per tile in 64-bit integers.
//   phase 1  horizontal pass over the source rows [R0, R1) that the tile's vertical taps need,
//            kCropStageRows at a time: thread (row = tid / 16, column = tid % 16) walks the
//            column's taps along the uint8 source row (neighbouring lanes read neighbouring,
//            overlapping spans of the same row; C = 4 pixels are one 32-bit load), weights from
//            registers, and writes the normalised fp32 row value to the LDS stage
//            [kCropStageRows][16][C] (16 KB at C = 4).
//   phase 2  vertical pass from LDS: thread (tid / 16, tid % 16) accumulates its output pixel's
//            taps that lie in the staged chunk, in registers. A tile whose row span exceeds the
//            stage (200 rows -> 7) simply takes several chunks; no scale is refused.
//   store    divide by the vertical weight sum, round, normalise, flip by mirroring the store
//            column; every output element is written exactly once. channels_last: one thread
//            stores its pixel's C floats (one 16-byte store at C = 4); NCHW: 64-byte row pieces.
//   uint8    a third instantiation stops after the rounding and the flip and stores bytes into
//            [B][Ho][Wo][C], the layout image_augment.hip and image_finish.hip read: the tile's
//            bytes are laid out (mirrored when flipped) in the stage, which is free by then, and
//            each tile row leaves as aligned 32-bit words. image_finish.hip applies the same
//            image_normalize() to those bytes, so the two launches give the float form's bits.
// Summation order is fixed (ascending taps, ascending chunks) and there are no atomics, so two
// runs are bitwise equal. Every source read is bounds-checked against the image; the binding
// rejects boxes with h, w < 1 or beyond kCropMaxExtent, and the kernel clamps them only so that a
// box it was never meant to see cannot make the setup loop long.
#include "common.h"
#include "image_norm.h"
#include "kernels.h"

namespace tdp {
namespace {

constexpr int kT = kCropTile;

struct CropTaps {
  int lo[2][kT];     // [0] = horizontal (output columns), [1] = vertical (output rows)
  int hi[2][kT];
  int num0[2][kT];   // num of tap lo
  float sum[2][kT];  // sum of the integer weights of taps [lo, hi)
};

__device__ __forceinline__ long floor_div(long a, long b) {  // b > 0
  const long q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

// taps of output coordinate o for n_in -> n_out; an o outside [0, n_out) gets an empty range
__device__ void make_taps(CropTaps& t, int axis, int k, int o, int n_in, int n_out) {
  if (o >= n_out) {
    t.lo[axis][k] = t.hi[axis][k] = t.num0[axis][k] = 0;
    t.sum[axis][k] = 1.f;
    return;
  }
  const long D = 2L * max(n_in, n_out), A = (2L * o + 1) * n_in, step = 2L * n_out;
  long lo = floor_div(A - D - n_out, step) + 1;         // first j with (2j+1) n_out > A - D
  long hi = floor_div(A + D - n_out + step - 1, step);  // first j with (2j+1) n_out >= A + D
  lo = max(lo, 0L);
  hi = min(hi, (long)n_in);
  const long n0 = (2 * lo + 1) * n_out - A;
  unsigned long long sum = 0;
  long num = n0;
  for (long j = lo; j < hi; ++j, num += step) sum += (unsigned long long)(D - (num < 0 ? -num : num));
  t.lo[axis][k] = (int)lo;
  t.hi[axis][k] = (int)hi;
  t.num0[axis][k] = (int)n0;
  t.sum[axis][k] = (float)sum;
}

template <int C>
__device__ __forceinline__ void load_pixel(const uint8_t* p, float (&v)[C]) {
  if constexpr (C == 4) {
    const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
    v[0] = (float)(u & 0xffu);
    v[1] = (float)((u >> 8) & 0xffu);
    v[2] = (float)((u >> 16) & 0xffu);
    v[3] = (float)(u >> 24);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = (float)p[c];
  }
}

template <int C, bool CL, bool U8>
__global__ __launch_bounds__(256) void image_crop_resize_kernel(
    const uint8_t* __restrict__ x, const int* __restrict__ box, const uint8_t* __restrict__ flip,
    float* __restrict__ out, int Hs, int Ws, int Ho, int Wo, float fill, ImageNorm nrm,
    int round_u8) {
  __shared__ CropTaps taps;
  __shared__ float stage[kCropStageRows * kT * C];

  const int tid = threadIdx.x, b = blockIdx.z;
  const int tx0 = blockIdx.x * kT, ty0 = blockIdx.y * kT;
  const int top = box[4 * b + 0], left = box[4 * b + 1];
  const int bh = min(max(box[4 * b + 2], 1), kCropMaxExtent);
  const int bw = min(max(box[4 * b + 3], 1), kCropMaxExtent);

  if (tid < kT) make_taps(taps, 0, tid, tx0 + tid, bw, Wo);
  else if (tid < 2 * kT) make_taps(taps, 1, tid - kT, ty0 + tid - kT, bh, Ho);
  __syncthreads();

  const int oxl = tid & (kT - 1), sub = tid / kT;  // phase 1: (row slot, column); phase 2: pixel
  const int ox = tx0 + oxl, oy = ty0 + sub;
  const bool col_ok = ox < Wo, pix_ok = col_ok && oy < Ho;
  const int hlo = taps.lo[0][oxl], hhi = taps.hi[0][oxl], hnum0 = taps.num0[0][oxl];
  const int vlo = taps.lo[1][sub], vhi = taps.hi[1][sub], vnum0 = taps.num0[1][sub];
  const float hsum = taps.sum[0][oxl], vsum = taps.sum[1][sub];
  const int Dh = 2 * max(bw, Wo), Dv = 2 * max(bh, Ho), hstep = 2 * Wo, vstep = 2 * Ho;
  // source rows the tile needs: first tap of its first row .. last tap of its last valid row
  const int R0 = taps.lo[1][0], R1 = taps.hi[1][min(kT, Ho - ty0) - 1];
  const uint8_t* img = x + (long)b * Hs * Ws * C;

  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;

  for (int r0 = R0; r0 < R1; r0 += kCropStageRows) {
    const int r1 = min(r0 + kCropStageRows, R1);
    if (col_ok) {
      for (int r = r0 + sub; r < r1; r += 256 / kT) {
        const long sy = (long)top + r;
        const bool row_in = sy >= 0 && sy < Hs;
        const uint8_t* row = img + (row_in ? sy : 0) * Ws * C;
        float a[C];
#pragma unroll
        for (int c = 0; c < C; ++c) a[c] = 0.f;
        int num = hnum0;
        for (int j = hlo; j < hhi; ++j, num += hstep) {
          const float wi = (float)(Dh - abs(num));
          const long sx = (long)left + j;
          float p[C];
          if (row_in && sx >= 0 && sx < Ws) {
            load_pixel<C>(row + sx * C, p);
          } else {
#pragma unroll
            for (int c = 0; c < C; ++c) p[c] = fill;
          }
#pragma unroll
          for (int c = 0; c < C; ++c) a[c] += wi * p[c];
        }
        float* dst = stage + ((r - r0) * kT + oxl) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) dst[c] = a[c] / hsum;
      }
    }
    __syncthreads();
    if (pix_ok) {
      const int ra = max(vlo, r0), rb = min(vhi, r1);
      int num = ra < rb ? vnum0 + vstep * (ra - vlo) : 0;  // |num| < Dv inside the tap range
      for (int r = ra; r < rb; ++r, num += vstep) {
        const float wi = (float)(Dv - abs(num));
        const float* src = stage + ((r - r0) * kT + oxl) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += wi * src[c];
      }
    }
    __syncthreads();  // the next chunk overwrites the stage
  }

  if constexpr (U8) {
    // uint8 form: stop after the flip. The stage is free after the loop's last barrier; the tile's
    // bytes go there, mirrored inside the tile when flipped, and each tile row leaves as aligned
    // 32-bit words, with single bytes at a ragged end.
    uint8_t* tile8 = reinterpret_cast<uint8_t*>(stage);
    uint8_t* o8 = reinterpret_cast<uint8_t*>(out);  // [B][Ho][Wo][C]
    const bool fl = flip != nullptr && flip[b];
    const int ncols = min(kT, Wo - tx0), len = ncols * C;
    if (pix_ok) {
      uint8_t* t = tile8 + (sub * kT + (fl ? ncols - 1 - oxl : oxl)) * C;
#pragma unroll
      for (int c = 0; c < C; ++c)
        t[c] = (uint8_t)(int)fminf(fmaxf(rintf(acc[c] / vsum), 0.f), 255.f);
    }
    __syncthreads();
    if (oy >= Ho) return;
    const uint8_t* trow = tile8 + sub * kT * C;
    uint8_t* orow = o8 + (((long)b * Ho + oy) * Wo + (fl ? Wo - tx0 - ncols : tx0)) * C;
    const int mis = (int)((uintptr_t)orow & 3);
    for (int e0 = 4 * oxl - mis; e0 < len; e0 += 4 * kT) {
      if (e0 >= 0 && e0 + 4 <= len) {
        *reinterpret_cast<uint32_t*>(orow + e0) =
            (uint32_t)trow[e0] | ((uint32_t)trow[e0 + 1] << 8) | ((uint32_t)trow[e0 + 2] << 16) |
            ((uint32_t)trow[e0 + 3] << 24);
      } else {
        for (int e = max(e0, 0); e < min(e0 + 4, len); ++e) orow[e] = trow[e];
      }
    }
    return;
  }
  if (!pix_ok) return;
  const int wo = (flip != nullptr && flip[b]) ? Wo - 1 - ox : ox;
  float v[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    v[c] = acc[c] / vsum;
    if (round_u8) v[c] = rintf(v[c]);
    v[c] = image_normalize(v[c], nrm.mean[c], nrm.inv_std[c]);
  }
  if (CL) {  // [B][Ho][Wo][C]
    float* dst = out + (((long)b * Ho + oy) * Wo + wo) * C;
    if constexpr (C == 4) {
      *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) dst[c] = v[c];
    }
  } else {   // [B][C][Ho][Wo]
#pragma unroll
    for (int c = 0; c < C; ++c) out[(((long)b * C + c) * Ho + oy) * Wo + wo] = v[c];
  }
}

template <int C, bool CL, bool U8 = false>
void launch_crop(const uint8_t* x, const int* box, const uint8_t* flip, float* out, int B, int Hs,
                 int Ws, int Ho, int Wo, float fill, const ImageNorm& nrm, int round_u8,
                 hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(Wo, kT), (unsigned)ceil_div(Ho, kT), (unsigned)B);
  hipLaunchKernelGGL((image_crop_resize_kernel<C, CL, U8>), grid, dim3(256), 0, s, x, box, flip, out,
                     Hs, Ws, Ho, Wo, fill, nrm, round_u8);
}

}  // namespace

void image_crop_resize(const uint8_t* x, const int* box, const uint8_t* flip, float* out, int B,
                       int Hs, int Ws, int C, int Ho, int Wo, float fill, const ImageNorm& nrm,
                       bool round_u8, bool channels_last, hipStream_t s) {
  if ((long)B * Ho * Wo <= 0) return;
  const int r = round_u8 ? 1 : 0;
#define TDP_CROP(CC, LL) \
  launch_crop<CC, LL>(x, box, flip, out, B, Hs, Ws, Ho, Wo, fill, nrm, r, s)
  if (C == 3) {
    if (channels_last) TDP_CROP(3, true); else TDP_CROP(3, false);
  } else if (C == 1) {
    if (channels_last) TDP_CROP(1, true); else TDP_CROP(1, false);
  } else if (C == 4) {
    if (channels_last) TDP_CROP(4, true); else TDP_CROP(4, false);
  }
#undef TDP_CROP
}

void image_crop_resize_u8(const uint8_t* x, const int* box, const uint8_t* flip, uint8_t* out,
                          int B, int Hs, int Ws, int C, int Ho, int Wo, float fill,
                          hipStream_t s) {
  if ((long)B * Ho * Wo <= 0) return;
  float* o = reinterpret_cast<float*>(out);  // the uint8 form reads it back as bytes
  const ImageNorm nrm{};
#define TDP_CROP8(CC) \
  launch_crop<CC, true, true>(x, box, flip, o, B, Hs, Ws, Ho, Wo, fill, nrm, 1, s)
  if (C == 3) TDP_CROP8(3);
  else if (C == 1) TDP_CROP8(1);
  else if (C == 4) TDP_CROP8(4);
#undef TDP_CROP8
}

}  // namespace tdp
