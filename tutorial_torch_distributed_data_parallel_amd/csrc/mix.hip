// Batch mixing for MixUp / CutMix (fp32, gfx950), out of place:
//   out[b, :, i, j] = inside(box_b, i, j) ? x[perm[b]]
//                                         : (lam_b == 1 ? x[b] : lam_b x[b] + (1 - lam_b) x[perm[b]])
// MixUp is an empty box, CutMix is lam == 1 with a real box; one launch serves a batch that holds
// both. box = (top, left, h, w), clipped to the image here; a perm[b] outside [0, N) is read as
// b (nothing is read out of bounds). Every pure-copy element (inside a box, or outside with
// lam == 1) is a select, never arithmetic: bitwise the source.
//
// Layout. In both memory layouts the project uses (contiguous [N][C][H][W] and channels_last
// [N][H][W][C]) sample b is the dense run of L = C*H*W floats at b*L, so the kernel walks that
// run in units of V floats and only the decoding of a unit's (i, j) differs:
//   NCHW: e = (c*H + i)*W + j -- a 16-byte unit may cross a row end, so (i, j) steps per element;
//   NHWC: e = (i*W + j)*C + c -- the same odometer with the channel innermost.
// V = 4 (16-byte accesses) needs L % 4 == 0 and aligned bases, so that every sample and its
// partner start on a 16-byte boundary; anything else takes V = 1 (4-byte accesses), the host
// chooses. A unit loads only what it needs: the partner is skipped when no element is inside the
// box and lam == 1, the sample itself when every element is inside.
//
// Work split: blockIdx.y is the sample, so perm / lam / box are workgroup-uniform and come in
// through scalar loads; blockIdx.x walks the sample in chunks of 256 threads x 4 units (16 KB of
// output per workgroup at V = 4), a thread's units 256 apart so that every access of the wave is
// one dense run.
#include "common.h"
#include "kernels.h"

namespace tdp {
namespace {

constexpr int kT = 256;
constexpr int kUnitsPerThread = 4;

struct MixParams {
  const float* x;
  float* out;
  const void* perm;
  const float* lam;
  const int* box;
  int N, C, H, W;
  int L;   // floats per sample (< 2^31)
  int nu;  // units per sample: L / V
  FastDiv dW, dIn;  // dIn: H*W (NCHW: plane size) or C (NHWC: pixel size)
};

template <bool NHWC, int V, typename I>
__global__ __launch_bounds__(kT) void mix_kernel(MixParams p) {
  const int b = blockIdx.y;
  long pb = (long)reinterpret_cast<const I*>(p.perm)[b];
  if (pb < 0 || pb >= p.N) pb = b;
  const float lam = p.lam[b], oml = 1.f - lam;
  const bool keep = lam == 1.f;
  // the box clipped to the image (64-bit: top + h of any two ints)
  const long top = p.box[4 * b], left = p.box[4 * b + 1];
  const long bot = top + p.box[4 * b + 2], right = left + p.box[4 * b + 3];
  const int i0 = (int)(top < 0 ? 0 : top), i1 = (int)(bot > p.H ? p.H : bot);
  const int j0 = (int)(left < 0 ? 0 : left), j1 = (int)(right > p.W ? p.W : right);
  const float* xb = p.x + (long)b * p.L;
  const float* xp = p.x + pb * p.L;
  float* o = p.out + (long)b * p.L;
#pragma unroll
  for (int q = 0; q < kUnitsPerThread; ++q) {
    const int u = (blockIdx.x * kUnitsPerThread + q) * kT + threadIdx.x;
    if (u >= p.nu) return;
    const uint32_t e = (uint32_t)u * V;
    // (i, j) of the unit's first element, and the innermost coordinate that steps first
    int i, j, c = 0;
    if constexpr (NHWC) {
      const uint32_t pix = fdiv(e, p.dIn);
      c = (int)(e - pix * (uint32_t)p.C);
      i = (int)fdiv(pix, p.dW);
      j = (int)(pix - (uint32_t)i * (uint32_t)p.W);
    } else {
      const uint32_t hw = e - fdiv(e, p.dIn) * (uint32_t)(p.H * p.W);
      i = (int)fdiv(hw, p.dW);
      j = (int)(hw - (uint32_t)i * (uint32_t)p.W);
    }
    bool in[V];
    bool any = false, all = true;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      in[k] = i >= i0 && i < i1 && j >= j0 && j < j1;
      any = any || in[k];
      all = all && in[k];
      if constexpr (NHWC) {
        if (++c == p.C) { c = 0; if (++j == p.W) { j = 0; ++i; } }
      } else {
        if (++j == p.W) { j = 0; if (++i == p.H) i = 0; }
      }
    }
    float vb[V], vp[V], r[V];
#pragma unroll
    for (int k = 0; k < V; ++k) vb[k] = vp[k] = 0.f;
    if (!all) {
      if constexpr (V == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xb + e);
        vb[0] = v[0]; vb[1] = v[1]; vb[2] = v[2]; vb[3] = v[3];
      } else {
        vb[0] = xb[e];
      }
    }
    if (any || !keep) {
      if constexpr (V == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xp + e);
        vp[0] = v[0]; vp[1] = v[1]; vp[2] = v[2]; vp[3] = v[3];
      } else {
        vp[0] = xp[e];
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
      r[k] = in[k] ? vp[k] : (keep ? vb[k] : lam * vb[k] + oml * vp[k]);
    if constexpr (V == 4) {
      f32x4 v;
      v[0] = r[0]; v[1] = r[1]; v[2] = r[2]; v[3] = r[3];
      *reinterpret_cast<f32x4*>(o + e) = v;
    } else {
      o[e] = r[0];
    }
  }
}

template <bool NHWC, int V>
void launch_mix(const MixParams& p, bool perm64, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(p.nu, kT * kUnitsPerThread), (unsigned)p.N), block(kT);
  if (perm64) hipLaunchKernelGGL((mix_kernel<NHWC, V, int64_t>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((mix_kernel<NHWC, V, int>), grid, block, 0, s, p);
}

}  // namespace

void mix_batch(const float* x, const void* perm, bool perm64, const float* lam, const int* box,
               float* out, int N, int C, int H, int W, bool nhwc, hipStream_t s) {
  const long L = (long)C * H * W;
  const bool vec = L % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0;
  MixParams p{x, out, perm, lam, box, N, C, H, W, (int)L, (int)(vec ? L / 4 : L),
              make_fastdiv((uint32_t)W), make_fastdiv((uint32_t)(nhwc ? C : H * W))};
  if (nhwc) {
    if (vec) launch_mix<true, 4>(p, perm64, s);
    else launch_mix<true, 1>(p, perm64, s);
  } else {
    if (vec) launch_mix<false, 4>(p, perm64, s);
    else launch_mix<false, 1>(p, perm64, s);
  }
}

}  // namespace tdp
