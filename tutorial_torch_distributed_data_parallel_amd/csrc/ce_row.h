// One cross-entropy row by one lane (a classifier head with few classes): shared by the fused
// loss kernels (csrc/loss.hip ce_fwd) and the fused head + loss kernel (csrc/gemm_skinny.hip
// head_ce), so both produce bit-identical per-row values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdp {

struct RowOut {
  float lse;
  float res;  // lse_split's rounding residual
  float loss;
  float correct;
  float valid;
};

// lse = max + log(sum exp(x - max)) as an unevaluated fp32 pair: lse holds the rounded sum, res
// what the rounding dropped (Knuth's two-sum: mx + l == lse + res exactly). At |max| ~ 100 the
// rounding of lse alone is ulp(100) ~ 8e-6, which would go straight into every probability.
// Below |lse| = kLseResMin the residual is at most 2^-22 (half an ulp of [4, 8)), inside what an
// fp32 probability carries anyway, and is dropped: res == 0 leaves every consumer's arithmetic
// exactly the single-float form, so training at ordinary logits keeps its trajectory bit for bit
// (a 1-ulp change of the toy MLP's first gradient grows to 1e-2 of the weights in 120 steps).
constexpr float kLseResMin = 8.f;
__device__ inline void lse_split(float mx, float l, float& lse, float& res) {
  lse = mx + l;
  const float lv = lse - mx;
  const float mv = lse - lv;
  res = fabsf(lse) >= kLseResMin ? (mx - mv) + (l - lv) : 0.f;
}

// softmax probability of one logit from the row's (lse, res): exp(x - (lse + res)), the small
// term applied after the large ones cancel. One formula for every producer of the logits
// gradient (ce_fwd's two dpre branches, ce_bwd, head_ce), so they stay bit-identical.
__device__ inline float ce_prob(float x, float lse, float res) {
  return __expf((x - lse) - res);
}

// the row's loss term; a zero smoothing weight never multiplies sumx (a masked class's -inf logit
// or an overflowed sum would turn 0 * sumx into NaN). Without smoothing the residual of lse goes
// in after the large terms cancel: a row with two logits at 3e38 has lse == 3e38 in fp32, and
// its loss log 2 is all in res.
__device__ inline float ce_row_loss(float lse, float res, float xy, float sumx, float eps, int C) {
  return eps != 0.f ? (lse - (1.f - eps) * xy - (eps / C) * sumx) : ((lse - xy) + res);
}

// One row handled by one lane (small C) -- logits row in registers-free sequential scan.
__device__ inline RowOut row_serial(const float* x, int C, int64_t y, int ignore_index, float eps) {
  float mx = -INFINITY;
  int arg = 0;
  float sumx = 0.f;
  for (int c = 0; c < C; ++c) {
    const float v = x[c];
    if (v > mx) { mx = v; arg = c; }
    sumx += v;
  }
  float se = 0.f;
  for (int c = 0; c < C; ++c) se += __expf(x[c] - mx);
  RowOut o;
  lse_split(mx, __logf(se), o.lse, o.res);
  const bool valid = (y != ignore_index) && y >= 0 && y < C;
  o.valid = valid ? 1.f : 0.f;
  o.loss = valid ? ce_row_loss(o.lse, o.res, x[y], sumx, eps, C) : 0.f;
  o.correct = (valid && arg == (int)y) ? 1.f : 0.f;
  return o;
}

}  // namespace tdp
