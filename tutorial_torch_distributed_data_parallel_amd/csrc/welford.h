// Welford accumulation and Chan's pairwise merge of (count, mean, M2) triples: the statistics
// arithmetic shared by the batch-norm (norm.hip) and group-norm (groupnorm.hip) kernels. Never
// E[x^2] - E[x]^2: a large-mean / small-spread input would cancel to nothing.
#pragma once
#include "common.h"

namespace tdp {
namespace {

struct Wf {
  float n, mean, m2;
};

__device__ __forceinline__ Wf wf_merge(Wf a, Wf b) {
  const float n = a.n + b.n;
  if (n == 0.f) return a;
  const float d = b.mean - a.mean;
  const float fb = b.n / n;
  Wf r;
  r.n = n;
  r.mean = fmaf(d, fb, a.mean);
  r.m2 = a.m2 + b.m2 + d * d * a.n * fb;
  return r;
}

__device__ __forceinline__ void wf_push(Wf& w, float x) {
  w.n += 1.f;
  const float d = x - w.mean;
  w.mean = fmaf(d, 1.f / w.n, w.mean);
  w.m2 = fmaf(d, x - w.mean, w.m2);
}

__device__ __forceinline__ Wf wf_wave(Wf w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Wf t;
    t.n = __shfl_xor(w.n, o, 64);
    t.mean = __shfl_xor(w.mean, o, 64);
    t.m2 = __shfl_xor(w.m2, o, 64);
    w = wf_merge(w, t);
  }
  return w;
}

}  // namespace
}  // namespace tdp
