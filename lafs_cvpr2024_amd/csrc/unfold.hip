// fViT front end and head (face_pre_pro/ViT_face.py:1506-1613): overlapping patch embedding and the BatchNorm1d head.
//   :1517,1582  nn.Unfold(kernel_size=k, stride, padding) + transpose   -> unfold_kernel (+ its adjoint fold_kernel)
//   :1530-1533  mlp_head = BatchNorm1d(dim) on the cls rows             -> bn1d_fwd_kernel / bn1d_bwd_kernel
// All four are HBM-bound glue: the window vectors leave as bf16 rows of ldp columns (3 k^2 padded to the MFMA GEMM's K granule of 32)
// that lafs_gemm_nt consumes directly.  No atomics anywhere: every sum below runs in a fixed order.
#include "common.hpp"
#include "bn_rows.hpp"
#include "lafs_hip.h"

namespace {

// grid (window row wy, image b).  The k image rows of the three channels that window row covers are staged in LDS once, zero where
// the window hangs over the image edge (scalar loads: with pad % 4 != 0 or S % 4 != 0 a row starts at an arbitrary float); then the
// n finished rows of this window row -- contiguous in the output -- leave as 16-byte stores, consecutive lanes on consecutive chunks.
// tile[c][i][x] at (c * k + i) * ldt + x, x = image column + pad; ldt is odd, so the k-strided walk of the writers spreads over the banks.
__global__ __launch_bounds__(256) void unfold_kernel(const float* __restrict__ img, int S, int k, int stride, int pad, int n, int ldt,
                                                     bf16_t* __restrict__ out, int ldp) {
  extern __shared__ float tile[];
  const int wy = blockIdx.x, b = blockIdx.y;
  const int wl = (n - 1) * stride + k;                    // staged columns: image columns -pad .. wl - pad - 1
  const int y0 = wy * stride - pad;
  const int lane = threadIdx.x & 63;
  for (int ci = threadIdx.x >> 6; ci < 3 * k; ci += 4) {  // one wave per staged row ci = c * k + i: the lanes walk along the image row
    const int c = ci / k, i = ci - c * k;
    const int y = y0 + i;
    const bool row_in = y >= 0 && y < S;
    const float* src = img + (((size_t)b * 3 + c) * S + (row_in ? y : 0)) * S;
    for (int x = lane; x < wl; x += 64) {
      const int xs = x - pad;
      float v = 0.f;
      if (row_in && xs >= 0 && xs < S) v = src[xs];
      tile[ci * ldt + x] = v;
    }
  }
  __syncthreads();
  const int per = ldp >> 3, kk = k * k, K = 3 * kk;
  bf16_t* dst = out + ((size_t)b * n + wy) * n * ldp;
  for (int q = threadIdx.x; q < n * per; q += 256) {
    const int wx = q / per, col0 = (q - wx * per) * 8;
    int c = col0 / kk, r = col0 - c * kk;
    int i = r / k, j = r - i * k;
    const float* base = tile + wx * stride;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] = (col0 + e < K) ? base[(c * k + i) * ldt + j] : 0.f;
      if (++j == k) { j = 0; if (++i == k) { i = 0; ++c; } }
    }
    *reinterpret_cast<uint4*>(dst + (size_t)q * 8) =
        make_uint4(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7]));
  }
}

// the adjoint as a gather: one thread per pixel adds the window entries that cover it, window rows then window columns ascending
__global__ __launch_bounds__(256) void fold_kernel(const float* __restrict__ dp, int ld, int B, int S, int k, int stride, int pad, int n,
                                                   float* __restrict__ dimg) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)B * 3 * S * S) return;
  const int x = (int)(t % S), y = (int)((t / S) % S), c = (int)((t / ((size_t)S * S)) % 3), b = (int)(t / ((size_t)3 * S * S));
  const int py = y + pad, px = x + pad;                   // window w covers p  <=>  w * stride <= p < w * stride + k
  const int wy0 = py >= k ? (py - k) / stride + 1 : 0, wy1 = min(n - 1, py / stride);
  const int wx0 = px >= k ? (px - k) / stride + 1 : 0, wx1 = min(n - 1, px / stride);
  float acc = 0.f;
  for (int wy = wy0; wy <= wy1; ++wy)
    for (int wx = wx0; wx <= wx1; ++wx)
      acc += dp[(((size_t)b * n + wy) * n + wx) * ld + (c * k + (py - wy * stride)) * k + (px - wx * stride)];
  dimg[t] = acc;
}

// src f32 [rows, cols] -> dst bf16 [rows, ldd], columns [cols, ldd) zero: one thread per 8 output columns
__global__ __launch_bounds__(256) void pad_cast_kernel(const float* __restrict__ src, int lds_, int rows, int cols, bf16_t* __restrict__ dst,
                                                       int ldd) {
  const int per = ldd >> 3;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (size_t)rows * per) return;
  const int r = (int)(q / per), c0 = (int)(q % per) * 8;
  const float* s = src + (size_t)r * lds_;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (c0 + e < cols) ? s[c0 + e] : 0.f;
  *reinterpret_cast<uint4*>(dst + (size_t)r * ldd + c0) =
      make_uint4(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7]));
}

// dst[r, c] = (accumulate ? dst[r, c] : 0) + src[r, c] for c < cols: the first 3 k^2 columns of the padded weight gradient
__global__ __launch_bounds__(256) void add_cols_kernel(const float* __restrict__ src, int lds_, int rows, int cols, float* __restrict__ dst,
                                                       int ldd, int accumulate) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)rows * cols) return;
  const int r = (int)(t / cols), c = (int)(t % cols);
  const float v = src[(size_t)r * lds_ + c];
  float* d = dst + (size_t)r * ldd + c;
  *d = accumulate ? *d + v : v;
}

// ---- BatchNorm1d over the rows of x f32 [n, D]: the kernels below are made of the row pieces of bn_rows.hpp (bn_fwd_rows / bn_bwd_rows
// and their halves), which the DINO head's fused BatchNorm + GELU kernels (head_bn.hip) share.
__global__ __launch_bounds__(64 * BN_WAVES) void bn1d_fwd_kernel(const float* __restrict__ x, int ldx, int n, int D,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                 float momentum, int training, float* __restrict__ running_mean,
                                                                 float* __restrict__ running_var, float* __restrict__ y, int ldy,
                                                                 float* __restrict__ save_mean, float* __restrict__ save_rstd) {
  __shared__ float red[BN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;                 // (no early return: every lane reaches the barriers)
  bn_fwd_rows(red, x, ldx, n, gamma, beta, eps, momentum, training, running_mean, running_var, y, ldy, save_mean, save_rstd, col, col < D,
              w, lane);
}

__global__ __launch_bounds__(64 * BN_WAVES) void bn1d_bwd_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx,
                                                                 int n, int D, const float* __restrict__ save_mean,
                                                                 const float* __restrict__ save_rstd, const float* __restrict__ gamma,
                                                                 int training, float* __restrict__ dx, int lddx, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta, int accumulate) {
  __shared__ float red[BN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  bn_bwd_rows(red, dy, lddy, x, ldx, n, save_mean, save_rstd, gamma, training, dx, lddx, dgamma, dbeta, accumulate, col, col < D, w, lane);
}

// ---- The same over G row ranges [rows[g], rows[g + 1]) of one packed buffer (a crop group each: reference :1556-1569 runs the head once
// per group, in list order).  One workgroup per 64 columns walks the groups in order, so what is ordered -- the running buffers' chain
// of (1 - m) old + m new updates, dgamma / dbeta summed group by group -- is read and written by the same thread (wave 0's lane of the
// column) in program order: one launch, the bits of G single-group launches.  The row table travels in the kernel arguments.
struct BnGroupRows { int rows[LAFS_BN1D_MAX_GROUPS + 1]; };

__global__ __launch_bounds__(64 * BN_WAVES) void bn1d_groups_fwd_kernel(const float* __restrict__ x, int ldx, BnGroupRows gr, int G, int D,
                                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                        float eps, float momentum, int training,
                                                                        float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                        float* __restrict__ y, int ldy, float* __restrict__ save_mean,
                                                                        float* __restrict__ save_rstd) {
  __shared__ float red[BN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  for (int g = 0; g < G; ++g) {
    const int r0 = gr.rows[g];
    bn_fwd_rows(red, x + (size_t)r0 * ldx, ldx, gr.rows[g + 1] - r0, gamma, beta, eps, momentum, training, running_mean, running_var,
                y + (size_t)r0 * ldy, ldy, save_mean + (size_t)g * D, save_rstd + (size_t)g * D, col, col < D, w, lane);
  }
}

__global__ __launch_bounds__(64 * BN_WAVES) void bn1d_groups_bwd_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ x,
                                                                        int ldx, BnGroupRows gr, int G, int D,
                                                                        const float* __restrict__ save_mean,
                                                                        const float* __restrict__ save_rstd, const float* __restrict__ gamma,
                                                                        int training, float* __restrict__ dx, int lddx,
                                                                        float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate) {
  __shared__ float red[BN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  for (int g = 0; g < G; ++g) {
    const int r0 = gr.rows[g];
    bn_bwd_rows(red, dy + (size_t)r0 * lddy, lddy, x + (size_t)r0 * ldx, ldx, gr.rows[g + 1] - r0, save_mean + (size_t)g * D,
                save_rstd + (size_t)g * D, gamma, training, dx + (size_t)r0 * lddx, lddx, dgamma, dbeta, (g > 0 || accumulate) ? 1 : 0, col,
                col < D, w, lane);
  }
}


// ---- The grouped head in training mode with the statistics of ALL ranks (the reference's SyncBatchNorm conversion, lafs_train.py:
// 362-364): forward and backward are each cut where the ranks meet.  A rank's partial of a group is {count, mean[D], M2[D]} (f32
// [G, 1 + 2 D]); the W partials of a group are folded in rank order 0 .. W-1 by the pairwise update (Chan et al.), the same sequence
// of operations on every rank: bit-identical statistics and running buffers everywhere.  One partial (W = 1) is taken as it is.
__global__ __launch_bounds__(64 * BN_WAVES) void bn1d_groups_stats_kernel(const float* __restrict__ x, int ldx, BnGroupRows gr, int G, int D,
                                                                          float* __restrict__ partial) {
  __shared__ float red[BN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  const bool on = col < D;
  for (int g = 0; g < G; ++g) {
    const int r0 = gr.rows[g], n = gr.rows[g + 1] - r0;
    float mean, m2;
    bn_moments_rows(red, x + (size_t)r0 * ldx, ldx, n, col, on, w, lane, mean, m2);
    float* p = partial + (size_t)g * (1 + 2 * D);
    if (w == 0 && on) { p[1 + col] = mean; p[1 + D + col] = m2; }
    if (w == 0 && col == 0) p[0] = (float)n;
  }
}

__global__ __launch_bounds__(64 * BN_WAVES) void bn1d_groups_sync_fwd_kernel(const float* __restrict__ x, int ldx, BnGroupRows gr, int G,
                                                                             int D, const float* __restrict__ partials, int W, size_t ldw,
                                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                             float eps, float momentum, float* __restrict__ running_mean,
                                                                             float* __restrict__ running_var, float* __restrict__ y, int ldy,
                                                                             float* __restrict__ save_mean, float* __restrict__ save_rstd) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  const bool on = col < D;
  for (int g = 0; g < G; ++g) {
    const float* p = partials + (size_t)g * (1 + 2 * D);
    float nf = p[0], mean = on ? p[1 + col] : 0.f, m2 = on ? p[1 + D + col] : 0.f;
    for (int r = 1; r < W; ++r) {                         // (every wave folds its own copy: W small numbers, no barrier)
      const float* q = p + (size_t)r * ldw;
      const float nb = q[0], mean_b = on ? q[1 + col] : 0.f, m2_b = on ? q[1 + D + col] : 0.f;
      const float nn = nf + nb, delta = mean_b - mean;
      mean = mean + delta * nb / nn;
      m2 = m2 + m2_b + delta * delta * nf * nb / nn;
      nf = nn;
    }
    const float rstd = bn_batch_rstd(mean, m2, nf, eps, momentum, running_mean, running_var, col, on, w);
    const int r0 = gr.rows[g];
    bn_apply_rows(x + (size_t)r0 * ldx, ldx, gr.rows[g + 1] - r0, mean, rstd, gamma, beta, y + (size_t)r0 * ldy, ldy,
                  save_mean + (size_t)g * D, save_rstd + (size_t)g * D, col, on, w);
  }
}

__global__ __launch_bounds__(64 * BN_WAVES) void bn1d_groups_bwd_sums_kernel(const float* __restrict__ dy, int lddy,
                                                                             const float* __restrict__ x, int ldx, BnGroupRows gr, int G,
                                                                             int D, const float* __restrict__ save_mean,
                                                                             const float* __restrict__ save_rstd, float* __restrict__ sums,
                                                                             float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                             int accumulate) {
  __shared__ float red[BN_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  const bool on = col < D;
  for (int g = 0; g < G; ++g) {
    const int r0 = gr.rows[g];
    const float mean = on ? save_mean[(size_t)g * D + col] : 0.f, rstd = on ? save_rstd[(size_t)g * D + col] : 0.f;
    float sb, sg;
    bn_bwd_sums_rows(red, dy + (size_t)r0 * lddy, lddy, x + (size_t)r0 * ldx, ldx, gr.rows[g + 1] - r0, mean, rstd, dgamma, dbeta,
                     (g > 0 || accumulate) ? 1 : 0, col, on, w, lane, sb, sg);
    if (w == 0 && on) { sums[(size_t)g * 2 * D + col] = sb; sums[(size_t)g * 2 * D + D + col] = sg; }
  }
}

__global__ __launch_bounds__(64 * BN_WAVES) void bn1d_groups_sync_bwd_kernel(const float* __restrict__ dy, int lddy,
                                                                             const float* __restrict__ x, int ldx, BnGroupRows gr,
                                                                             BnGroupRows total, int G, int D,
                                                                             const float* __restrict__ save_mean,
                                                                             const float* __restrict__ save_rstd,
                                                                             const float* __restrict__ gamma, const float* __restrict__ sums,
                                                                             float* __restrict__ dx, int lddx) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  const bool on = col < D;
  for (int g = 0; g < G; ++g) {
    const int r0 = gr.rows[g];
    const float mean = on ? save_mean[(size_t)g * D + col] : 0.f, rstd = on ? save_rstd[(size_t)g * D + col] : 0.f;
    const float sb = on ? sums[(size_t)g * 2 * D + col] : 0.f, sg = on ? sums[(size_t)g * 2 * D + D + col] : 0.f;
    const float mb = sb / (float)total.rows[g], mg = sg / (float)total.rows[g];
    bn_bwd_apply_rows(dy + (size_t)r0 * lddy, lddy, x + (size_t)r0 * ldx, ldx, gr.rows[g + 1] - r0, mean, rstd, gamma, mb, mg,
                      dx + (size_t)r0 * lddx, lddx, col, on, w);
  }
}

}  // namespace

static int unfold_windows(int S, int k, int stride, int pad) { return (S + 2 * pad - k) / stride + 1; }

extern "C" int lafs_unfold_bf16(const float* img, int B, int S, int k, int stride, int pad, void* patches, int ldp, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(img && patches && B > 0 && B <= 65535 && S > 0, "bad operand");
  LAFS_CHECK_ARG(k >= 1 && stride >= 1 && pad >= 0 && pad < k, "window needs k >= 1, stride >= 1, 0 <= pad < k");
  LAFS_CHECK_ARG(S + 2 * pad >= k, "the padded image is smaller than one window");
  const int n = unfold_windows(S, k, stride, pad);
  LAFS_CHECK_ARG(n >= 1 && (long)3 * k * k <= ldp && ldp % 32 == 0, "ldp must be a multiple of 32 and hold the 3 k^2 window values");
  LAFS_CHECK_ARG(((uintptr_t)patches & 15) == 0, "patches must be 16-byte aligned (16-byte row stores)");
  const int ldt = ((n - 1) * stride + k) | 1;
  const size_t lds_bytes = (size_t)3 * k * ldt * sizeof(float);
  LAFS_CHECK_ARG(lds_bytes <= 65536, "3 k image-row strips must fit the 64 KB of LDS");
  hipLaunchKernelGGL(unfold_kernel, dim3(n, B), dim3(256), lds_bytes, stream, img, S, k, stride, pad, n, ldt, (bf16_t*)patches, ldp);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_fold_f32(const float* dpatches, int ld, int B, int S, int k, int stride, int pad, float* dimg, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(dpatches && dimg && B > 0 && S > 0, "bad operand");
  LAFS_CHECK_ARG(k >= 1 && stride >= 1 && pad >= 0 && pad < k, "window needs k >= 1, stride >= 1, 0 <= pad < k");
  LAFS_CHECK_ARG(S + 2 * pad >= k, "the padded image is smaller than one window");
  const int n = unfold_windows(S, k, stride, pad);
  LAFS_CHECK_ARG(n >= 1 && (long)3 * k * k <= ld, "ld must hold the 3 k^2 window values");
  const size_t total = (size_t)B * 3 * S * S;
  LAFS_CHECK_ARG(total < ((size_t)1 << 31) * 256, "image batch too large");
  hipLaunchKernelGGL(fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, dpatches, ld, B, S, k, stride, pad, n, dimg);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_pad_cast_bf16(const float* src, int lds, int rows, int cols, void* dst, int ldd, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(src && dst && rows > 0 && cols > 0 && lds >= cols, "bad operand");
  LAFS_CHECK_ARG(ldd >= cols && ldd % 8 == 0 && ((uintptr_t)dst & 15) == 0, "ldd must be a multiple of 8 and dst 16-byte aligned");
  const size_t total = (size_t)rows * (ldd / 8);
  hipLaunchKernelGGL(pad_cast_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, lds, rows, cols, (bf16_t*)dst, ldd);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_add_cols_f32(const float* src, int lds, int rows, int cols, float* dst, int ldd, int accumulate, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(src && dst && rows > 0 && cols > 0 && lds >= cols && ldd >= cols, "bad operand");
  const size_t total = (size_t)rows * cols;
  hipLaunchKernelGGL(add_cols_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, lds, rows, cols, dst, ldd, accumulate);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_bn1d_fwd(const float* x, int ldx, int n, int D, const float* gamma, const float* beta, float eps, float momentum,
                             int training, float* running_mean, float* running_var, float* y, int ldy, float* save_mean, float* save_rstd,
                             hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(x && gamma && beta && y && save_mean && save_rstd, "null operand");
  LAFS_CHECK_ARG(n > 0 && D > 0 && D <= 2048 && ldx >= D && ldy >= D, "1 <= D <= 2048 and row strides >= D");
  LAFS_CHECK_ARG(!training || n >= 2, "batch statistics need more than one row (nn.BatchNorm1d: Expected more than 1 value per channel when training)");
  LAFS_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "running_mean and running_var come together");
  LAFS_CHECK_ARG(training || running_mean != nullptr, "the eval forward normalises with the running statistics");
  hipLaunchKernelGGL(bn1d_fwd_kernel, dim3(ceil_div(D, 64)), dim3(64 * BN_WAVES), 0, stream, x, ldx, n, D, gamma, beta, eps, momentum,
                     training ? 1 : 0, running_mean, running_var, y, ldy, save_mean, save_rstd);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_bn1d_bwd(const float* dy, int lddy, const float* x, int ldx, int n, int D, const float* save_mean, const float* save_rstd,
                             const float* gamma, int training, float* dx, int lddx, float* dgamma, float* dbeta, int accumulate,
                             hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(dy && x && save_mean && save_rstd && gamma && dx && dgamma && dbeta, "null operand");
  LAFS_CHECK_ARG(n > 0 && D > 0 && D <= 2048 && lddy >= D && ldx >= D && lddx >= D, "1 <= D <= 2048 and row strides >= D");
  LAFS_CHECK_ARG(!training || n >= 2, "batch statistics need more than one row");
  hipLaunchKernelGGL(bn1d_bwd_kernel, dim3(ceil_div(D, 64)), dim3(64 * BN_WAVES), 0, stream, dy, lddy, x, ldx, n, D, save_mean, save_rstd,
                     gamma, training ? 1 : 0, dx, lddx, dgamma, dbeta, accumulate ? 1 : 0);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

// validates the host row table and copies it into the launch argument; the reason of a refusal, or nullptr
static const char* bn_group_rows(const int* group_rows, int G, int min_rows, BnGroupRows* out) {
  if (group_rows == nullptr) return "null operand";
  if (G < 1 || G > LAFS_BN1D_MAX_GROUPS) return "1 <= G <= LAFS_BN1D_MAX_GROUPS";
  if (group_rows[0] != 0) return "group_rows[0] must be 0";
  for (int g = 0; g < G; ++g) {
    if (group_rows[g + 1] <= group_rows[g]) return "group_rows must ascend strictly (no empty group)";
    if (group_rows[g + 1] - group_rows[g] < min_rows) return "batch statistics need more than one row in every group";
  }
  for (int g = 0; g <= LAFS_BN1D_MAX_GROUPS; ++g) out->rows[g] = g <= G ? group_rows[g] : group_rows[G];
  return nullptr;
}

extern "C" int lafs_bn1d_groups_fwd(const float* x, int ldx, const int* group_rows, int G, int D, const float* gamma, const float* beta,
                                    float eps, float momentum, int training, float* running_mean, float* running_var, float* y, int ldy,
                                    float* save_mean, float* save_rstd, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(x && gamma && beta && y && save_mean && save_rstd, "null operand");
  LAFS_CHECK_ARG(D > 0 && D <= 2048 && ldx >= D && ldy >= D, "1 <= D <= 2048 and row strides >= D");
  BnGroupRows gr;
  const char* why = bn_group_rows(group_rows, G, training ? 2 : 1, &gr);
  LAFS_CHECK_ARG(why == nullptr, why);
  LAFS_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "running_mean and running_var come together");
  LAFS_CHECK_ARG(training || running_mean != nullptr, "the eval forward normalises with the running statistics");
  hipLaunchKernelGGL(bn1d_groups_fwd_kernel, dim3(ceil_div(D, 64)), dim3(64 * BN_WAVES), 0, stream, x, ldx, gr, G, D, gamma, beta, eps,
                     momentum, training ? 1 : 0, running_mean, running_var, y, ldy, save_mean, save_rstd);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_bn1d_groups_bwd(const float* dy, int lddy, const float* x, int ldx, const int* group_rows, int G, int D,
                                    const float* save_mean, const float* save_rstd, const float* gamma, int training, float* dx, int lddx,
                                    float* dgamma, float* dbeta, int accumulate, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(dy && x && save_mean && save_rstd && gamma && dx && dgamma && dbeta, "null operand");
  LAFS_CHECK_ARG(D > 0 && D <= 2048 && lddy >= D && ldx >= D && lddx >= D, "1 <= D <= 2048 and row strides >= D");
  BnGroupRows gr;
  const char* why = bn_group_rows(group_rows, G, training ? 2 : 1, &gr);
  LAFS_CHECK_ARG(why == nullptr, why);
  hipLaunchKernelGGL(bn1d_groups_bwd_kernel, dim3(ceil_div(D, 64)), dim3(64 * BN_WAVES), 0, stream, dy, lddy, x, ldx, gr, G, D, save_mean,
                     save_rstd, gamma, training ? 1 : 0, dx, lddx, dgamma, dbeta, accumulate ? 1 : 0);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

// the total row counts of the groups over all ranks (host table of G entries, by value like the row table); the reason of a refusal
static const char* bn_group_totals(const int* group_total, const BnGroupRows& gr, int G, BnGroupRows* out) {
  if (group_total == nullptr) return "null operand";
  for (int g = 0; g < G; ++g) {
    if (group_total[g] < gr.rows[g + 1] - gr.rows[g]) return "a group's total row count is below this rank's own";
    if (group_total[g] < 2) return "batch statistics need more than one row per group over all ranks";
    if (group_total[g] > (1 << 24)) return "a group's total row count must be exact in f32 (<= 2^24)";
  }
  for (int g = 0; g <= LAFS_BN1D_MAX_GROUPS; ++g) out->rows[g] = g < G ? group_total[g] : 0;
  return nullptr;
}

extern "C" int lafs_bn1d_groups_stats(const float* x, int ldx, const int* group_rows, int G, int D, float* partial, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(x && partial, "null operand");
  LAFS_CHECK_ARG(D > 0 && D <= 2048 && ldx >= D, "1 <= D <= 2048 and row strides >= D");
  BnGroupRows gr;
  const char* why = bn_group_rows(group_rows, G, 1, &gr);
  LAFS_CHECK_ARG(why == nullptr, why);
  hipLaunchKernelGGL(bn1d_groups_stats_kernel, dim3(ceil_div(D, 64)), dim3(64 * BN_WAVES), 0, stream, x, ldx, gr, G, D, partial);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_bn1d_groups_sync_fwd(const float* x, int ldx, const int* group_rows, const int* group_total, int G, int D,
                                         const float* partials, int W, int64_t ldw, const float* gamma, const float* beta, float eps,
                                         float momentum, float* running_mean, float* running_var, float* y, int ldy, float* save_mean,
                                         float* save_rstd, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(x && partials && gamma && beta && y && save_mean && save_rstd, "null operand");
  LAFS_CHECK_ARG(D > 0 && D <= 2048 && ldx >= D && ldy >= D, "1 <= D <= 2048 and row strides >= D");
  LAFS_CHECK_ARG(W >= 1 && W <= LAFS_BN1D_MAX_RANKS, "1 <= W <= LAFS_BN1D_MAX_RANKS");
  LAFS_CHECK_ARG(G >= 1 && G <= LAFS_BN1D_MAX_GROUPS && (W == 1 || ldw >= (int64_t)G * (1 + 2 * D)),
                 "1 <= G <= LAFS_BN1D_MAX_GROUPS and the ranks' partials must not overlap (ldw >= G (1 + 2 D))");
  BnGroupRows gr, total;
  const char* why = bn_group_rows(group_rows, G, 1, &gr);
  LAFS_CHECK_ARG(why == nullptr, why);
  why = bn_group_totals(group_total, gr, G, &total);
  LAFS_CHECK_ARG(why == nullptr, why);
  LAFS_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "running_mean and running_var come together");
  hipLaunchKernelGGL(bn1d_groups_sync_fwd_kernel, dim3(ceil_div(D, 64)), dim3(64 * BN_WAVES), 0, stream, x, ldx, gr, G, D, partials, W,
                     (size_t)ldw, gamma, beta, eps, momentum, running_mean, running_var, y, ldy, save_mean, save_rstd);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_bn1d_groups_bwd_sums(const float* dy, int lddy, const float* x, int ldx, const int* group_rows, int G, int D,
                                         const float* save_mean, const float* save_rstd, float* sums, float* dgamma, float* dbeta,
                                         int accumulate, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(dy && x && save_mean && save_rstd && sums && dgamma && dbeta, "null operand");
  LAFS_CHECK_ARG(D > 0 && D <= 2048 && lddy >= D && ldx >= D, "1 <= D <= 2048 and row strides >= D");
  BnGroupRows gr;
  const char* why = bn_group_rows(group_rows, G, 1, &gr);
  LAFS_CHECK_ARG(why == nullptr, why);
  hipLaunchKernelGGL(bn1d_groups_bwd_sums_kernel, dim3(ceil_div(D, 64)), dim3(64 * BN_WAVES), 0, stream, dy, lddy, x, ldx, gr, G, D,
                     save_mean, save_rstd, sums, dgamma, dbeta, accumulate ? 1 : 0);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_bn1d_groups_sync_bwd(const float* dy, int lddy, const float* x, int ldx, const int* group_rows, const int* group_total,
                                         int G, int D, const float* save_mean, const float* save_rstd, const float* gamma,
                                         const float* sums, float* dx, int lddx, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(dy && x && save_mean && save_rstd && gamma && sums && dx, "null operand");
  LAFS_CHECK_ARG(D > 0 && D <= 2048 && lddy >= D && ldx >= D && lddx >= D, "1 <= D <= 2048 and row strides >= D");
  BnGroupRows gr, total;
  const char* why = bn_group_rows(group_rows, G, 1, &gr);
  LAFS_CHECK_ARG(why == nullptr, why);
  why = bn_group_totals(group_total, gr, G, &total);
  LAFS_CHECK_ARG(why == nullptr, why);
  hipLaunchKernelGGL(bn1d_groups_sync_bwd_kernel, dim3(ceil_div(D, 64)), dim3(64 * BN_WAVES), 0, stream, dy, lddy, x, ldx, gr, total, G, D,
                     save_mean, save_rstd, gamma, sums, dx, lddx);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}
