// The row pieces of BatchNorm1d over the rows of x f32 [n, D], shared by the fViT head (unfold.hip) and the DINO head's fused
// BatchNorm + GELU kernels (head_bn.hip): one arithmetic, so that both give the same bits wherever they compute the same thing.
// One workgroup per 64 columns (lane = column: a wave reads 256 contiguous bytes of a
// row), rows strided over the BN_WAVES waves; the waves' partial sums meet in LDS and are added in wave order.
// Variance without cancellation: the column is shifted by its first row before it is summed (mean = x0 + sum(x - x0) / n: the sum is
// of the spread, not of the level), and the squares are of (x - mean) in a second pass.
#pragma once
#include "common.hpp"

namespace {

constexpr int BN_WAVES = 8;

__device__ __forceinline__ float bn_combine(float (*red)[64], float v, int w, int lane) {
  __syncthreads();                                        // (the previous round's readers are done with `red`)
  red[w][lane] = v;
  __syncthreads();
  float s = red[0][lane];
#pragma unroll
  for (int i = 1; i < BN_WAVES; ++i) s += red[i][lane];
  return s;
}

// The pieces of one group of rows through the forward.  lafs_bn1d_fwd, the grouped kernel and the cross-rank pair (statistics /
// sync forward) are all made of them, so that they give the same bits wherever they compute the same thing.  Every thread of the
// workgroup calls them (barriers inside bn_moments_rows); `on`: this lane has a column.
// mean = x0 + sum(x - x0) / n and M2 = sum (x - mean)^2 of the n rows
__device__ __forceinline__ void bn_moments_rows(float (*red)[64], const float* __restrict__ x, int ldx, int n, int col, bool on, int w,
                                                int lane, float& mean, float& m2) {
  const float x0 = on ? x[col] : 0.f;
  float s = 0.f;
  if (on) for (int r = w; r < n; r += BN_WAVES) s += x[(size_t)r * ldx + col] - x0;
  s = bn_combine(red, s, w, lane);
  mean = x0 + s / (float)n;
  float q = 0.f;
  if (on) for (int r = w; r < n; r += BN_WAVES) { const float d = x[(size_t)r * ldx + col] - mean; q = __builtin_fmaf(d, d, q); }
  m2 = bn_combine(red, q, w, lane);
}

// rstd of the batch statistics (mean, M2) of nf rows; wave 0's lane of the column steps the running buffers (unbiased variance)
__device__ __forceinline__ float bn_batch_rstd(float mean, float m2, float nf, float eps, float momentum, float* __restrict__ running_mean,
                                               float* __restrict__ running_var, int col, bool on, int w) {
  const float var = m2 / nf;
  const float rstd = 1.0f / sqrtf(var + eps);
  if (on && w == 0 && running_mean != nullptr) {
    running_mean[col] = (1.0f - momentum) * running_mean[col] + momentum * mean;
    running_var[col] = (1.0f - momentum) * running_var[col] + momentum * (var * (nf / (nf - 1.0f)));
  }
  return rstd;
}

__device__ __forceinline__ void bn_apply_rows(const float* __restrict__ x, int ldx, int n, float mean, float rstd,
                                              const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y, int ldy,
                                              float* __restrict__ save_mean, float* __restrict__ save_rstd, int col, bool on, int w) {
  if (!on) return;
  if (w == 0) { save_mean[col] = mean; save_rstd[col] = rstd; }
  const float g = gamma[col], bt = beta[col];
  for (int r = w; r < n; r += BN_WAVES) y[(size_t)r * ldy + col] = (x[(size_t)r * ldx + col] - mean) * rstd * g + bt;
}

// One group of rows through the forward: the whole arithmetic of lafs_bn1d_fwd, shared by the single-group kernel and the grouped one.
__device__ __forceinline__ void bn_fwd_rows(float (*red)[64], const float* __restrict__ x, int ldx, int n, const float* __restrict__ gamma,
                                            const float* __restrict__ beta, float eps, float momentum, int training,
                                            float* __restrict__ running_mean, float* __restrict__ running_var, float* __restrict__ y, int ldy,
                                            float* __restrict__ save_mean, float* __restrict__ save_rstd, int col, bool on, int w, int lane) {
  float mean = 0.f, rstd = 0.f;
  if (training) {
    float m2;
    bn_moments_rows(red, x, ldx, n, col, on, w, lane, mean, m2);
    rstd = bn_batch_rstd(mean, m2, (float)n, eps, momentum, running_mean, running_var, col, on, w);
  } else if (on) {
    mean = running_mean[col];
    rstd = 1.0f / sqrtf(running_var[col] + eps);
  }
  bn_apply_rows(x, ldx, n, mean, rstd, gamma, beta, y, ldy, save_mean, save_rstd, col, on, w);
}

// training: dx = gamma rstd (dy - mean(dy) - xhat mean(dy xhat));  eval (statistics are constants): dx = gamma rstd dy
// The two halves of one group's backward, shared like the forward's pieces: the column sums of dy and dy xhat (added into dgamma /
// dbeta by wave 0's lane of the column) and dx from the two means mb = sum dy / N, mg = sum dy xhat / N.
__device__ __forceinline__ void bn_bwd_sums_rows(float (*red)[64], const float* __restrict__ dy, int lddy, const float* __restrict__ x,
                                                 int ldx, int n, float mean, float rstd, float* __restrict__ dgamma,
                                                 float* __restrict__ dbeta, int accumulate, int col, bool on, int w, int lane, float& sb,
                                                 float& sg) {
  sb = 0.f; sg = 0.f;
  if (on)
    for (int r = w; r < n; r += BN_WAVES) {
      const float d = dy[(size_t)r * lddy + col];
      sb += d;
      sg = __builtin_fmaf(d, (x[(size_t)r * ldx + col] - mean) * rstd, sg);
    }
  sb = bn_combine(red, sb, w, lane);
  sg = bn_combine(red, sg, w, lane);
  if (on && w == 0) {
    dgamma[col] = accumulate ? dgamma[col] + sg : sg;
    dbeta[col] = accumulate ? dbeta[col] + sb : sb;
  }
}

__device__ __forceinline__ void bn_bwd_apply_rows(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx, int n,
                                                  float mean, float rstd, const float* __restrict__ gamma, float mb, float mg,
                                                  float* __restrict__ dx, int lddx, int col, bool on, int w) {
  if (!on) return;
  const float gr = gamma[col] * rstd;
  for (int r = w; r < n; r += BN_WAVES) {
    const float xh = (x[(size_t)r * ldx + col] - mean) * rstd;
    dx[(size_t)r * lddx + col] = gr * (dy[(size_t)r * lddy + col] - mb - xh * mg);
  }
}

__device__ __forceinline__ void bn_bwd_rows(float (*red)[64], const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx,
                                            int n, const float* __restrict__ save_mean, const float* __restrict__ save_rstd,
                                            const float* __restrict__ gamma, int training, float* __restrict__ dx, int lddx,
                                            float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate, int col, bool on, int w,
                                            int lane) {
  const float mean = on ? save_mean[col] : 0.f, rstd = on ? save_rstd[col] : 0.f;
  float sb, sg;
  bn_bwd_sums_rows(red, dy, lddy, x, ldx, n, mean, rstd, dgamma, dbeta, accumulate, col, on, w, lane, sb, sg);
  const float mb = training ? sb / (float)n : 0.f, mg = training ? sg / (float)n : 0.f;
  bn_bwd_apply_rows(dy, lddy, x, ldx, n, mean, rstd, gamma, mb, mg, dx, lddx, col, on, w);
}

}  // namespace
