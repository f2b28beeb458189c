// Cross-entropy against a class-probability target (fp32, gfx950): forward, the logits gradient
// for a unit upstream gradient in the same launch, and the accuracy count. What MixUp / CutMix
// training needs and the index-target kernels of csrc/loss.hip cannot read.
//
// Two target forms, one kernel family:
//   dense -- t is [B, C]; semantics of F.cross_entropy(logits, probs, label_smoothing=eps):
//            t' = (1 - eps) t + eps / C, row loss = lse * sum(t') - sum(t'_c x_c), row gradient
//            g * (p_c * sum(t') - t'_c). sum(t) is whatever the row holds, never assumed 1.
//   pair  -- (ya, yb, lam) per row: t = lam * onehot(ya) + (1 - lam) * onehot(yb), never
//            materialised. Only the two named logits are multiplied, so at eps == 0 a -inf logit
//            on any other class leaves the loss finite, as the index form does. A row whose ya
//            or yb lies outside [0, C) reads nothing out of bounds and gives NaN.
// The per-row primitives are ce_row.h's, unchanged: lse_split, ce_prob, and the rule that a zero
// weight never multiplies a logit (a zero t_c, lam, 1 - lam or eps skips its product).
//
// Work split: one 64-lane wave owns one row, a 256-thread workgroup four rows, the grid is
// ceil(B / 4); waves share nothing (no LDS, no barrier). A row is cut into units of four
// consecutive classes; lane l owns units l, l + 64, l + 128, ... and walks them in ascending
// order, in every form, so a row's sums are a function of C alone:
//   register  -- C <= kSoftCeCap: the lane's units of the logits row (and of the dense target)
//                are loaded once and stay in registers (NV = 1 / 4 / 16 units per lane, from C).
//                One sweep gives max + argmax (lowest index on ties), sum x, sum t, sum t x and
//                the target's argmax; sum exp and the gradient are sweeps over registers only:
//                logits and target are read exactly once.
//   streaming -- C > kSoftCeCap: the same units in the same order, re-read per sweep.
//   each with 16-byte unit loads (C % 4 == 0, row strides % 4 == 0, 16-byte aligned bases) or
//   four 4-byte loads per unit (anything else; the last unit may be part-filled). The host
//   chooses from (C, strides, pointers), never per row, and both give bitwise the same values.
//
// g is 1 / B (mean) or 1 (sum), known on the host: unlike the index form there is no batch-wide
// count to wait for, so the gradient is written by the wave that owns the row. Per-row loss and
// correct flags go to rows[2][B]; soft_ce_finish (one workgroup) adds them in a fixed order
// (thread t: rows t, t + 256, ...; then the block tree). No atomics: two runs agree bitwise, and
// row r of a batch is bitwise that row run alone (loss term, and gradient at reduction = sum).
#include "ce_row.h"
#include "common.h"
#include "kernels.h"

namespace tdp {
namespace {

constexpr int kT = 256;  // 4 waves = 4 rows per workgroup

struct SoftCeParams {
  const float* x;      // logits [B][C], row stride ld
  const float* t;      // dense target [B][C], row stride ldt (dense form)
  const int64_t* ya;   // pair form
  const int64_t* yb;
  const float* lam;
  float* rows;         // [2][B]: row loss | argmax(logits) == argmax(target)
  float* dpre;         // optional [B][C] dense: the gradient for a unit upstream gradient
  long ld, ldt;
  int B, C;
  float eps, g;
};

// one unit = classes 4u .. 4u + 3. V = 4: one 16-byte access (every class exists);
// V = 1: four 4-byte accesses, classes >= C skipped.
template <int V>
__device__ __forceinline__ void ld_unit(const float* row, int u, int C, float (&r)[4]) {
  if constexpr (V == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * u);
    r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = 4 * u + j < C ? row[4 * u + j] : 0.f;
  }
}

template <int V>
__device__ __forceinline__ void st_unit(float* row, int u, int C, const float (&r)[4]) {
  if constexpr (V == 4) {
    f32x4 v;
    v[0] = r[0]; v[1] = r[1]; v[2] = r[2]; v[3] = r[3];
    *reinterpret_cast<f32x4*>(row + 4 * u) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * u + j < C) row[4 * u + j] = r[j];
  }
}

struct RowAcc {
  float mx;    // max logit and its lowest index
  int arg;
  float sumx;
  float st;    // dense: sum t, sum t x, max t and its lowest index
  float stx;
  float tmx;
  int targ;
};

template <bool DENSE, int V>
__device__ __forceinline__ void acc_unit(RowAcc& a, const float (&x)[4], const float (&t)[4],
                                         int u, int C) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = 4 * u + j;
    if (V == 4 || c < C) {
      if (x[j] > a.mx) { a.mx = x[j]; a.arg = c; }
      a.sumx += x[j];
      if constexpr (DENSE) {
        a.st += t[j];
        if (t[j] != 0.f) a.stx = fmaf(t[j], x[j], a.stx);
        if (t[j] > a.tmx) { a.tmx = t[j]; a.targ = c; }
      }
    }
  }
}

// the wave's maximum with the lowest index on ties (torch.max's first maximal element)
__device__ __forceinline__ void wave_argmax(float& m, int& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, kWave);
    const int oa = __shfl_xor(a, o, kWave);
    if (om > m || (om == m && oa < a)) { m = om; a = oa; }
  }
}

// NV > 0: register form with NV units per lane; NV == 0: streaming form.
template <bool DENSE, int V, int NV>
__global__ __launch_bounds__(kT) void soft_ce_kernel(SoftCeParams p) {
  const int row = blockIdx.x * (kT / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= p.B) return;  // the whole wave: waves share nothing
  const int C = p.C, nu = (C + 3) >> 2;
  const float* x = p.x + (long)row * p.ld;
  const float* t = DENSE ? p.t + (long)row * p.ldt : nullptr;
  constexpr int NR = NV ? NV : 1;
  float xv[NR][4], tv[NR][4];
  RowAcc a{-INFINITY, 0x7fffffff, 0.f, 0.f, 0.f, -INFINITY, 0x7fffffff};

  // ---- sweep 1: the only read of the row in the register form
  if constexpr (NV > 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int u = i * kWave + lane;
#pragma unroll
      for (int j = 0; j < 4; ++j) xv[i][j] = tv[i][j] = 0.f;
      if (u < nu) {
        ld_unit<V>(x, u, C, xv[i]);
        if constexpr (DENSE) ld_unit<V>(t, u, C, tv[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int u = i * kWave + lane;
      if (u < nu) acc_unit<DENSE, V>(a, xv[i], tv[i], u, C);
    }
  } else {
    for (int u = lane; u < nu; u += kWave) {
      ld_unit<V>(x, u, C, xv[0]);
      if constexpr (DENSE) ld_unit<V>(t, u, C, tv[0]);
      acc_unit<DENSE, V>(a, xv[0], tv[0], u, C);
    }
  }
  wave_argmax(a.mx, a.arg);
  const float sumx = wave_sum(a.sumx);

  // ---- sweep 2: sum exp(x - max)
  float se = 0.f;
  if constexpr (NV > 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int u = i * kWave + lane;
      if (u < nu) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (V == 4 || 4 * u + j < C) se += __expf(xv[i][j] - a.mx);
      }
    }
  } else {
    for (int u = lane; u < nu; u += kWave) {
      ld_unit<V>(x, u, C, xv[0]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (V == 4 || 4 * u + j < C) se += __expf(xv[0][j] - a.mx);
    }
  }
  se = wave_sum(se);
  float lse, res;
  lse_split(a.mx, __logf(se), lse, res);

  // ---- the row's target sums
  const float eps = p.eps, ome = 1.f - eps, k = eps / C;
  float St, Stx, lam = 0.f, oml = 0.f;
  int targ, ia = -1, ib = -1;
  bool ok = true;
  if constexpr (DENSE) {
    wave_argmax(a.tmx, a.targ);
    St = wave_sum(a.st);
    Stx = wave_sum(a.stx);
    targ = a.targ;
  } else {
    const int64_t ya = p.ya[row], yb = p.yb[row];
    lam = p.lam[row];
    oml = 1.f - lam;
    ok = ya >= 0 && ya < C && yb >= 0 && yb < C;
    ia = ok ? (int)ya : -1;
    ib = ok ? (int)yb : -1;
    const float xa = ok && lam != 0.f ? lam * x[ia] : 0.f;
    const float xb = ok && oml != 0.f ? oml * x[ib] : 0.f;
    St = 1.f;
    Stx = xa + xb;
    targ = lam >= 0.5f ? ia : ib;
  }
  if (eps != 0.f) {
    Stx = ome * Stx + k * sumx;
    if constexpr (DENSE) St = fmaf(ome, St, eps);
  }
  // lse's rounding residual goes in after the large terms cancel (ce_row.h ce_row_loss)
  const float loss = (lse * St - Stx) + res * St;

  // ---- sweep 3: the gradient for a unit upstream gradient
  if (p.dpre) {
    float* d = p.dpre + (long)row * C;
    const float g = p.g;
    auto grad_unit = [&](const float (&xu)[4], const float (&tu)[4], int u) {
      float r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * u + j;
        const float pr = ce_prob(xu[j], lse, res);
        float tc;
        if constexpr (DENSE) tc = tu[j];
        else tc = (c == ia ? lam : 0.f) + (c == ib ? oml : 0.f);
        const float tp = eps != 0.f ? fmaf(ome, tc, k) : tc;
        r[j] = ok ? g * (pr * St - tp) : NAN;
      }
      st_unit<V>(d, u, C, r);
    };
    if constexpr (NV > 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int u = i * kWave + lane;
        if (u < nu) grad_unit(xv[i], tv[i], u);
      }
    } else {
      for (int u = lane; u < nu; u += kWave) {
        ld_unit<V>(x, u, C, xv[0]);
        if constexpr (DENSE) ld_unit<V>(t, u, C, tv[0]);
        grad_unit(xv[0], tv[0], u);
      }
    }
  }
  if (lane == 0) {
    p.rows[row] = ok ? loss : NAN;
    p.rows[p.B + row] = (ok && a.arg == targ) ? 1.f : 0.f;
  }
}

// rows[2][B] -> loss scalar and the metric block, in a fixed order
__global__ __launch_bounds__(kT) void soft_ce_finish_kernel(const float* __restrict__ rows, int B,
                                                            int mean, float* out_loss,
                                                            float* acc) {
  __shared__ float red[kT / kWave];
  float ls = 0.f, cr = 0.f;
  for (int r = threadIdx.x; r < B; r += kT) {
    ls += rows[r];
    cr += rows[B + r];
  }
  ls = block_sum<kT>(ls, red);
  cr = block_sum<kT>(cr, red);
  if (threadIdx.x == 0) {
    out_loss[0] = mean ? ls / (float)B : ls;
    if (acc) { acc[0] += ls; acc[1] += cr; acc[2] += (float)B; }
  }
}

// d = gout[0] * dpre: the backward for an upstream gradient that is not the unit seed
__global__ __launch_bounds__(kT) void soft_ce_scale_kernel(const float* __restrict__ dpre,
                                                           const float* __restrict__ gout, long n,
                                                           float* __restrict__ d) {
  const float g = gout[0];
  for (long i = blockIdx.x * (long)kT + threadIdx.x; i < n; i += (long)gridDim.x * kT)
    d[i] = g * dpre[i];
}

inline bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

template <bool DENSE, int V>
void launch_form(const SoftCeParams& p, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(p.B, kT / kWave)), block(kT);
  if (p.C <= 256)
    hipLaunchKernelGGL((soft_ce_kernel<DENSE, V, 1>), grid, block, 0, s, p);
  else if (p.C <= 1024)
    hipLaunchKernelGGL((soft_ce_kernel<DENSE, V, 4>), grid, block, 0, s, p);
  else if (p.C <= kSoftCeCap)
    hipLaunchKernelGGL((soft_ce_kernel<DENSE, V, kSoftCeCap / (4 * kWave)>), grid, block, 0, s, p);
  else
    hipLaunchKernelGGL((soft_ce_kernel<DENSE, V, 0>), grid, block, 0, s, p);
}

}  // namespace

void soft_ce_fwd(const float* logits, long ld, const float* target, long ldt, const int64_t* ya,
                 const int64_t* yb, const float* lam, int B, int C, float label_smoothing,
                 bool mean, float* rows, float* out_loss, float* acc, float* dpre,
                 hipStream_t s) {
  SoftCeParams p{logits, target, ya, yb, lam, rows, dpre, ld, ldt, B, C, label_smoothing,
                 mean ? 1.f / (float)B : 1.f};
  const bool vec = C % 4 == 0 && ld % 4 == 0 && al16(logits) &&
                   (!target || (ldt % 4 == 0 && al16(target))) && (!dpre || al16(dpre));
  if (target) {
    if (vec) launch_form<true, 4>(p, s);
    else launch_form<true, 1>(p, s);
  } else {
    if (vec) launch_form<false, 4>(p, s);
    else launch_form<false, 1>(p, s);
  }
  hipLaunchKernelGGL(soft_ce_finish_kernel, dim3(1), dim3(kT), 0, s, rows, B, mean ? 1 : 0,
                     out_loss, acc);
}

void soft_ce_scale(const float* dpre, const float* gout, long n, float* d, hipStream_t s) {
  int grid = ceil_div(n, kT);
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(soft_ce_scale_kernel, dim3(grid), dim3(kT), 0, s, dpre, gout, n, d);
}

}  // namespace tdp
