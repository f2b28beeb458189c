// Per-element optimizer updates shared by the flat / multi-tensor optimizer kernels (optim.hip)
// and the weight-gradient GEMM epilogue that applies the update in place of storing the gradient
// (gemm_f32_fast.hip, OptEpilogue). Semantics are torch's: TORCH/optim/sgd.py (momentum buffer
// initialised to the first gradient, dampening, nesterov, maximize, L2 weight decay) and
// TORCH/optim/adam.py (bias-corrected, L2 vs decoupled weight decay, amsgrad).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace tdp {

// Take the per-step scalars from the device hyper block when there is one (kernels.h HyperSlot).
// Uniform loads at kernel start; the structural flags stay as launched.
__device__ __forceinline__ void load_hyper(SgdHyper& h) {
  const float* d = h.dev;
  if (d == nullptr) return;
  h.lr = d[kHLr];
  if (h.momentum != 0.f) h.momentum = d[kHMom];  // zero momentum is structural (no buffer)
  h.dampening = d[kHDamp];
  h.weight_decay = d[kHWd];
  h.first_step = d[kHFirst] != 0.f;
  h.grad_scale *= d[kHScale];
}

__device__ __forceinline__ void load_hyper(AdamHyper& h) {
  const float* d = h.dev;
  if (d == nullptr) return;
  h.lr = d[kHLr];
  h.beta1 = d[kHMom];
  h.beta2 = d[kHDamp];
  h.weight_decay = d[kHWd];
  h.eps = d[kHEps];
  h.bc1 = d[kHBc1];
  h.bc2_sqrt = d[kHBc2];
  h.grad_scale *= d[kHScale];
}

__device__ __forceinline__ void sgd_elem(float& p, float g, float& b, const SgdHyper& h) {
  g *= h.grad_scale;
  if (h.maximize) g = -g;
  if (h.weight_decay != 0.f) g = fmaf(h.weight_decay, p, g);
  if (h.momentum != 0.f) {
    b = h.first_step ? g : fmaf(b, h.momentum, (1.f - h.dampening) * g);
    g = h.nesterov ? fmaf(h.momentum, b, g) : b;
  }
  p = fmaf(-h.lr, g, p);
}

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float* vmax,
                                          const AdamHyper& h) {
  g *= h.grad_scale;
  if (h.maximize) g = -g;
  if (h.weight_decay != 0.f) {
    if (h.decoupled) p *= (1.f - h.lr * h.weight_decay);
    else g = fmaf(h.weight_decay, p, g);
  }
  m = fmaf(1.f - h.beta1, g - m, m);  // lerp(m, g, 1-beta1)
  v = fmaf(v, h.beta2, (1.f - h.beta2) * g * g);
  float vv = v;
  if (h.amsgrad) {
    vv = fmaxf(*vmax, v);
    *vmax = vv;
  }
  const float denom = sqrtf(vv) / h.bc2_sqrt + h.eps;
  p = fmaf(-(h.lr / h.bc1), m / denom, p);
}

// ---------------------------------------------------------------- layer-wise (optim_layerwise.hip)
// LAMB and LARS scale each tensor's update by a trust ratio built from whole-tensor norms, so the
// element functions come in the two halves the norm reduction separates. `wd` is the weight decay
// of THIS tensor (0 for a tensor skipped by skip_1d), `ratio` its trust ratio from the workspace.

// The LAMB direction from the moments: u = (m / bc1) / (sqrt(v) / bc2_sqrt + eps) + wd * p.
__device__ __forceinline__ float lamb_u(float p, float m, float v, const AdamHyper& h, float wd) {
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  float u = (m / h.bc1) / denom;
  if (wd != 0.f) u = fmaf(wd, p, u);
  return u;
}

// Stage 1: advance m and v by the gradient and return u. Stage 2 calls lamb_u on the stored m, v
// and the still-unchanged p, which gives the same bits.
__device__ __forceinline__ float lamb_update_elem(float p, float g, float& m, float& v,
                                                  const AdamHyper& h, float wd) {
  g *= h.grad_scale;
  if (h.maximize) g = -g;
  m = fmaf(1.f - h.beta1, g - m, m);
  v = fmaf(v, h.beta2, (1.f - h.beta2) * g * g);
  return lamb_u(p, m, v, h, wd);
}

// g' of the LARS norm: the gradient as lars_elem sees it before weight decay.
__device__ __forceinline__ float lars_grad(float g, const SgdHyper& h) {
  g *= h.grad_scale;
  return h.maximize ? -g : g;
}

// d = ratio * (g' + wd * p), then torch-SGD momentum / dampening / nesterov on d.
__device__ __forceinline__ void lars_elem(float& p, float g, float& b, float ratio,
                                          const SgdHyper& h, float wd) {
  g = lars_grad(g, h);
  if (wd != 0.f) g = fmaf(wd, p, g);
  g *= ratio;
  if (h.momentum != 0.f) {
    b = h.first_step ? g : fmaf(b, h.momentum, (1.f - h.dampening) * g);
    g = h.nesterov ? fmaf(h.momentum, b, g) : b;
  }
  p = fmaf(-h.lr, g, p);
}

}  // namespace tdp
