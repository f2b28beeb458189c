// Layer-wise adaptive optimizers: LAMB (Adam with a per-tensor trust ratio) and LARS (SGD with
// one). Neither is elementwise: the update of every element of a tensor is scaled by
// ||p|| / ||update|| of the whole tensor, so a step is a reduction per tensor feeding an
// elementwise pass. Three launches, no host synchronisation, no float atomics (kernels.h):
//
//   stage 1  one workgroup per run of the work table. LAMB reads p, g, m, v, writes m and v and
//            forms u; LARS reads p and g. Each chunk's (sum p^2, sum u^2) goes to
//            partials[chunk]: per lane in element order, across the wave by a fixed butterfly,
//            across the four waves in wave order.
//   finish   one wave per tensor: lane l adds partials l, l + 64, ... of the tensor in order, the
//            butterfly adds the lanes; norms and the trust ratio go to the workspace.
//   stage 2  LAMB recomputes u from the stored m, v and the unchanged p (lamb_u: same bits as
//            stage 1) so the gradient is never overwritten; LARS runs lars_elem. Both scale by
//            ratio[tensor].
//
// The partition is the table's alone: nothing depends on the grid size or the CU count, so the
// norms are bitwise reproducible and equal on every rank that holds equal values. Bytes per
// element: LAMB 16 + 8 in stage 1 and 12 + 4 in stage 2 (40; Adam 28), LARS 8 in stage 1 and
// 12 + 8 in stage 2 (28 with momentum). Norms are plain fp32 sums of squares, not rescaled: a
// norm that overflows gives a non-finite update, as the same formula would in torch.
//
// Lane t of a workgroup owns the quads (4 consecutive elements) t, t + 256, ... of its chunk (a
// wave: l, l + 64, ...). The 16-byte instantiation and the scalar one (views that are only
// 4-byte aligned) assign elements to lanes alike, so both give the same bits. No store reaches
// past a chunk's n: the arena's gaps stay zero.
#include "common.h"
#include "kernels.h"
#include "optim_elem.h"

namespace tdp {
namespace {

template <bool VEC>
__device__ __forceinline__ f32x4 ld4(const float* x, int i, int n) {
  if (VEC && i + 4 <= n) return *reinterpret_cast<const f32x4*>(x + i);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i + e < n) r[e] = x[i + e];
  return r;
}

template <bool VEC>
__device__ __forceinline__ void st4(float* x, int i, int n, const f32x4& v) {
  if (VEC && i + 4 <= n) {
    *reinterpret_cast<f32x4*>(x + i) = v;
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i + e < n) x[i + e] = v[e];
}

// ---- stage 1 of one quad: sp += p^2, su += u^2 (LARS: g'^2) in element order
template <bool VEC>
__device__ __forceinline__ void quad1(const LwChunk& c, int i, const AdamHyper& h, float wd,
                                      float& sp, float& su) {
  const f32x4 p = ld4<VEC>(c.p, i, c.n), g = ld4<VEC>(c.g, i, c.n);
  f32x4 m = ld4<VEC>(c.s0, i, c.n), v = ld4<VEC>(c.s1, i, c.n);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (i + e < c.n) {
      float me = m[e], ve = v[e];
      const float u = lamb_update_elem(p[e], g[e], me, ve, h, wd);
      m[e] = me;
      v[e] = ve;
      sp = fmaf(p[e], p[e], sp);
      su = fmaf(u, u, su);
    }
  }
  st4<VEC>(c.s0, i, c.n, m);
  st4<VEC>(c.s1, i, c.n, v);
}

template <bool VEC>
__device__ __forceinline__ void quad1(const LwChunk& c, int i, const SgdHyper& h, float,
                                      float& sp, float& su) {
  const f32x4 p = ld4<VEC>(c.p, i, c.n), g = ld4<VEC>(c.g, i, c.n);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (i + e < c.n) {
      const float ge = lars_grad(g[e], h);
      sp = fmaf(p[e], p[e], sp);
      su = fmaf(ge, ge, su);
    }
  }
}

// ---- stage 2 of one quad
template <bool VEC>
__device__ __forceinline__ void quad2(const LwChunk& c, int i, const AdamHyper& h, float wd,
                                      float ratio) {
  f32x4 p = ld4<VEC>(c.p, i, c.n);
  const f32x4 m = ld4<VEC>(c.s0, i, c.n), v = ld4<VEC>(c.s1, i, c.n);
  const float step = h.lr * ratio;
#pragma unroll
  for (int e = 0; e < 4; ++e) p[e] = fmaf(-step, lamb_u(p[e], m[e], v[e], h, wd), p[e]);
  st4<VEC>(c.p, i, c.n, p);
}

template <bool VEC>
__device__ __forceinline__ void quad2(const LwChunk& c, int i, const SgdHyper& h, float wd,
                                      float ratio) {
  f32x4 p = ld4<VEC>(c.p, i, c.n);
  const f32x4 g = ld4<VEC>(c.g, i, c.n);
  const bool mom = h.momentum != 0.f;
  f32x4 b = {0.f, 0.f, 0.f, 0.f};
  if (mom && !h.first_step) b = ld4<VEC>(c.s0, i, c.n);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float pe = p[e], be = b[e];
    lars_elem(pe, g[e], be, ratio, h, wd);
    p[e] = pe;
    b[e] = be;
  }
  st4<VEC>(c.p, i, c.n, p);
  if (mom) st4<VEC>(c.s0, i, c.n, b);
}

template <class H, bool VEC>
__global__ __launch_bounds__(256) void lw_stage1_kernel(const LwChunk* __restrict__ chunks,
                                                        const LwRun* __restrict__ runs,
                                                        float2* __restrict__ partials, H h) {
  load_hyper(h);
  __shared__ float red[8];
  const LwRun r = runs[blockIdx.x];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (r.count == 1 && chunks[r.first].n > kLwSmall) {  // workgroup-uniform
    const LwChunk c = chunks[r.first];
    const float wd = c.skip ? 0.f : h.weight_decay;
    float sp = 0.f, su = 0.f;
    for (int i = threadIdx.x * 4; i < c.n; i += 1024) quad1<VEC>(c, i, h, wd, sp, su);
    sp = wave_sum(sp);
    su = wave_sum(su);
    if (lane == 0) {
      red[wid] = sp;
      red[4 + wid] = su;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      partials[r.first] = make_float2(((red[0] + red[1]) + red[2]) + red[3],
                                      ((red[4] + red[5]) + red[6]) + red[7]);
    return;
  }
  for (int ci = r.first + wid; ci < r.first + r.count; ci += 4) {  // wave-uniform
    const LwChunk c = chunks[ci];
    const float wd = c.skip ? 0.f : h.weight_decay;
    float sp = 0.f, su = 0.f;
    for (int i = lane * 4; i < c.n; i += 256) quad1<VEC>(c, i, h, wd, sp, su);
    sp = wave_sum(sp);
    su = wave_sum(su);
    if (lane == 0) partials[ci] = make_float2(sp, su);
  }
}

// kind 0 LAMB: ratio = ||p|| / ||u||; kind 1 LARS: trust * ||p|| / (||g'|| + wd ||p|| + eps);
// 1 when either norm is not positive, and for a skipped tensor.
__global__ __launch_bounds__(256) void lw_finish_kernel(const LwTensor* __restrict__ tensors,
                                                        int T,
                                                        const float2* __restrict__ partials,
                                                        float* __restrict__ ws, int kind,
                                                        float wd, float eps, float trust,
                                                        const float* dev) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;  // wave-uniform
  const LwTensor tt = tensors[t];
  float sp = 0.f, su = 0.f;
  for (int k = lane; k < tt.count; k += 64) {
    const float2 v = partials[tt.first + k];
    sp += v.x;
    su += v.y;
  }
  sp = wave_sum(sp);
  su = wave_sum(su);
  if (lane != 0) return;
  if (dev != nullptr) {
    wd = dev[kHWd];
    eps = dev[kHEps];
  }
  const float np = sqrtf(sp), nu = sqrtf(su);
  float ratio = 1.f;
  if (!tt.skip && np > 0.f && nu > 0.f)
    ratio = kind == 0 ? np / nu : (trust * np) / (fmaf(wd, np, nu) + eps);
  ws[t] = np;
  ws[T + t] = nu;
  ws[2 * T + t] = ratio;
}

template <class H, bool VEC>
__global__ __launch_bounds__(256) void lw_stage2_kernel(const LwChunk* __restrict__ chunks,
                                                        const LwRun* __restrict__ runs,
                                                        const float* __restrict__ ratio, H h) {
  load_hyper(h);
  const LwRun r = runs[blockIdx.x];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (r.count == 1 && chunks[r.first].n > kLwSmall) {
    const LwChunk c = chunks[r.first];
    const float wd = c.skip ? 0.f : h.weight_decay;
    const float q = ratio[c.tensor];
    for (int i = threadIdx.x * 4; i < c.n; i += 1024) quad2<VEC>(c, i, h, wd, q);
    return;
  }
  for (int ci = r.first + wid; ci < r.first + r.count; ci += 4) {
    const LwChunk c = chunks[ci];
    const float wd = c.skip ? 0.f : h.weight_decay;
    const float q = ratio[c.tensor];
    for (int i = lane * 4; i < c.n; i += 256) quad2<VEC>(c, i, h, wd, q);
  }
}

template <class H>
void launch(const LwTable& t, const H& h, int kind, float trust, float eps, int stages,
            hipStream_t s) {
  if (t.nruns <= 0 || t.ntensors <= 0) return;
  float2* parts = reinterpret_cast<float2*>(t.partials);
  if (stages & 1) {
    if (t.vec)
      hipLaunchKernelGGL((lw_stage1_kernel<H, true>), dim3(t.nruns), dim3(256), 0, s, t.chunks,
                         t.runs, parts, h);
    else
      hipLaunchKernelGGL((lw_stage1_kernel<H, false>), dim3(t.nruns), dim3(256), 0, s, t.chunks,
                         t.runs, parts, h);
  }
  if (stages & 2)
    hipLaunchKernelGGL(lw_finish_kernel, dim3((t.ntensors + 3) / 4), dim3(256), 0, s, t.tensors,
                       t.ntensors, parts, t.ws, kind, h.weight_decay, eps, trust, h.dev);
  if (stages & 4) {
    const float* ratio = t.ws + 2 * (long)t.ntensors;
    if (t.vec)
      hipLaunchKernelGGL((lw_stage2_kernel<H, true>), dim3(t.nruns), dim3(256), 0, s, t.chunks,
                         t.runs, ratio, h);
    else
      hipLaunchKernelGGL((lw_stage2_kernel<H, false>), dim3(t.nruns), dim3(256), 0, s, t.chunks,
                         t.runs, ratio, h);
  }
}

}  // namespace

void lamb_layerwise(const LwTable& t, const AdamHyper& h, int stages, hipStream_t s) {
  launch(t, h, 0, 0.f, h.eps, stages, s);
}

void lars_layerwise(const LwTable& t, const SgdHyper& h, float trust, float eps, int stages,
                    hipStream_t s) {
  launch(t, h, 1, trust, eps, stages, s);
}

}  // namespace tdp
