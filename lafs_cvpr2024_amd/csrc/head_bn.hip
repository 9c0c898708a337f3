// DINO head with BatchNorm (vision_transformer.py:272-281 with use_bn=True): the hidden activations of the head's MLP are
//   :274,279  nn.BatchNorm1d(hidden_dim)  followed by  :275,280  nn.GELU()      -> bn1d_gelu_fwd_kernel / bn1d_gelu_bwd_kernel
// on the f32 output u of the Linear in front (lafs_gemm_nt, LAFS_EPI_F32).  The BatchNorm output y = xhat gamma + beta lives in
// registers only: the forward stores a = bf16(gelu(y)), the next GEMM's operand; the backward recomputes xhat and y from u and the
// saved statistics, forms g = da gelu'(y) on the fly (twice: once for the column sums, once for du) and never stores it.
// The statistics, the running-buffer update and the wave-order LDS fold are the row pieces of bn_rows.hpp, the arithmetic of
// lafs_bn1d_fwd: one workgroup per 64 columns, rows strided over the BN_WAVES waves, no atomics, the same bits run to run.
#include "common.hpp"
#include "bn_rows.hpp"
#include "lafs_hip.h"

namespace {

__global__ __launch_bounds__(64 * BN_WAVES) void bn1d_gelu_fwd_kernel(const float* __restrict__ u, int ldu, int n, int D,
                                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      float eps, float momentum, int training,
                                                                      float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                      bf16_t* __restrict__ a, int lda, float* __restrict__ save_mean,
                                                                      float* __restrict__ save_rstd) {
  __shared__ float red[BN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;                 // (no early return: every lane reaches the barriers)
  const bool on = col < D;
  float mean = 0.f, rstd = 0.f;
  if (training) {
    float m2;
    bn_moments_rows(red, u, ldu, n, col, on, w, lane, mean, m2);
    rstd = bn_batch_rstd(mean, m2, (float)n, eps, momentum, running_mean, running_var, col, on, w);
  } else if (on) {
    mean = running_mean[col];
    rstd = 1.0f / sqrtf(running_var[col] + eps);
  }
  if (!on) return;                                        // (behind the last barrier)
  if (w == 0) { save_mean[col] = mean; save_rstd[col] = rstd; }
  const float g = gamma[col], bt = beta[col];
  for (int r = w; r < n; r += BN_WAVES) {
    const float y = (u[(size_t)r * ldu + col] - mean) * rstd * g + bt;
    a[(size_t)r * lda + col] = f2bf(gelu_f(y));
  }
}

// g = da gelu'(y) of one element, with the xhat it was formed from
__device__ __forceinline__ float bn_gelu_grad(float da, float uv, float mean, float rstd, float g, float bt, float& xh) {
  xh = (uv - mean) * rstd;
  return da * gelu_grad_f(xh * g + bt);
}

__global__ __launch_bounds__(64 * BN_WAVES) void bn1d_gelu_bwd_kernel(const float* __restrict__ da, int ldda, const float* __restrict__ u,
                                                                      int ldu, int n, int D, const float* __restrict__ save_mean,
                                                                      const float* __restrict__ save_rstd, const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, int training,
                                                                      bf16_t* __restrict__ du, int lddu, float* __restrict__ dgamma,
                                                                      float* __restrict__ dbeta, int accumulate) {
  __shared__ float red[BN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  const bool on = col < D;
  const float mean = on ? save_mean[col] : 0.f, rstd = on ? save_rstd[col] : 0.f;
  const float g = on ? gamma[col] : 0.f, bt = on ? beta[col] : 0.f;
  // first pass: the column sums of g and g xhat, as bn_bwd_sums_rows forms them of a stored dy
  float sb = 0.f, sg = 0.f;
  if (on)
    for (int r = w; r < n; r += BN_WAVES) {
      float xh;
      const float d = bn_gelu_grad(da[(size_t)r * ldda + col], u[(size_t)r * ldu + col], mean, rstd, g, bt, xh);
      sb += d;
      sg = __builtin_fmaf(d, xh, sg);
    }
  sb = bn_combine(red, sb, w, lane);
  sg = bn_combine(red, sg, w, lane);
  if (!on) return;                                        // (behind the last barrier)
  if (w == 0) {
    dgamma[col] = accumulate ? dgamma[col] + sg : sg;
    dbeta[col] = accumulate ? dbeta[col] + sb : sb;
  }
  // second pass: du, the expression of bn_bwd_apply_rows on the recomputed g
  const float mb = training ? sb / (float)n : 0.f, mg = training ? sg / (float)n : 0.f;
  const float gr = g * rstd;
  for (int r = w; r < n; r += BN_WAVES) {
    float xh;
    const float d = bn_gelu_grad(da[(size_t)r * ldda + col], u[(size_t)r * ldu + col], mean, rstd, g, bt, xh);
    du[(size_t)r * lddu + col] = f2bf(gr * (d - mb - xh * mg));
  }
}

}  // namespace

extern "C" int lafs_bn1d_gelu_fwd(const float* u, int ldu, int n, int D, const float* gamma, const float* beta, float eps, float momentum,
                                  int training, float* running_mean, float* running_var, void* a_bf16, int lda, float* save_mean,
                                  float* save_rstd, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(u && gamma && beta && a_bf16 && save_mean && save_rstd, "null operand");
  LAFS_CHECK_ARG(n > 0 && D > 0 && D <= 65535 * 64 && ldu >= D && lda >= D, "n >= 1, D >= 1 and row strides >= D");
  LAFS_CHECK_ARG(!training || n >= 2, "batch statistics need more than one row (nn.BatchNorm1d: Expected more than 1 value per channel when training)");
  LAFS_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "running_mean and running_var come together");
  LAFS_CHECK_ARG(training || running_mean != nullptr, "the eval forward normalises with the running statistics");
  hipLaunchKernelGGL(bn1d_gelu_fwd_kernel, dim3(ceil_div(D, 64)), dim3(64 * BN_WAVES), 0, stream, u, ldu, n, D, gamma, beta, eps, momentum,
                     training ? 1 : 0, running_mean, running_var, (bf16_t*)a_bf16, lda, save_mean, save_rstd);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_bn1d_gelu_bwd(const float* da, int ldda, const float* u, int ldu, int n, int D, const float* save_mean,
                                  const float* save_rstd, const float* gamma, const float* beta, int training, void* du_bf16, int lddu,
                                  float* dgamma, float* dbeta, int accumulate, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(da && u && save_mean && save_rstd && gamma && beta && du_bf16 && dgamma && dbeta, "null operand");
  LAFS_CHECK_ARG(n > 0 && D > 0 && D <= 65535 * 64 && ldda >= D && ldu >= D && lddu >= D, "n >= 1, D >= 1 and row strides >= D");
  LAFS_CHECK_ARG(!training || n >= 2, "batch statistics need more than one row");
  hipLaunchKernelGGL(bn1d_gelu_bwd_kernel, dim3(ceil_div(D, 64)), dim3(64 * BN_WAVES), 0, stream, da, ldda, u, ldu, n, D, save_mean,
                     save_rstd, gamma, beta, training ? 1 : 0, (bf16_t*)du_bf16, lddu, dgamma, dbeta, accumulate ? 1 : 0);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}
