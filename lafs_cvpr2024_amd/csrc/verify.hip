// Face verification on the device (LFW / CFP-FP / AgeDB .bin sets): reference util/utils.py:292-397 (perform_val) and
// util/verification.py (evaluate, calculate_roc, calculate_accuracy).  Two launches around the extraction:
//   lafs_eval_flip_normalize  u8 [B,3,S,S] -> f32 [2B,3,S,S]: the batch scaled, then the same batch mirrored along W
//   lafs_verify_tail          trunk output of those 2B rows -> per-copy norms, flip-summed L2-normalised embeddings, pair
//                             distances and a per-fold / per-class histogram of the threshold index each distance falls in
// lafs_cvpr2024_amd/verification.py turns the histogram into the reference's fold statistics on the host.
#include "common.hpp"
#include "lafs_hip.h"

// every float / double operation is rounded on its own: the scaling is bit-identical to torch's CPU arithmetic
#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int FLIP_THREADS = 256;
constexpr int TAIL_THREADS = 256;                       // 4 waves, one pair per wave at a time
constexpr int TAIL_MAX_D = 1024;                        // 16 values per lane and image
constexpr int TAIL_MAX_LDS = 64 * 1024;

// One thread per 16 bytes of a row: one 16-byte load, four 16-byte stores of the scaled row segment, four 16-byte stores of the
// same values in reverse order at the mirrored position of the second copy (the reversal happens in registers).
__global__ __launch_bounds__(FLIP_THREADS) void eval_flip_norm_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int B,
                                                                      int S, float div, float mul, float add) {
#pragma clang fp contract(off)
  const int cpr = S >> 4;
  const size_t rows = (size_t)B * 3 * S;
  const size_t total = rows * cpr;
  const size_t half = rows * S;
  for (size_t i = (size_t)blockIdx.x * FLIP_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * FLIP_THREADS) {
    const size_t row = i / cpr;
    const int c = (int)(i - row * cpr);
    const uint4 v = *reinterpret_cast<const uint4*>(src + row * S + 16 * c);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    float y[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float x = (float)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
      const float q = x / div;
      const float m = q * mul;
      y[k] = m + add;
    }
    float4* o = reinterpret_cast<float4*>(dst + row * S + 16 * c);
    float4* f = reinterpret_cast<float4*>(dst + half + row * S + (S - 16 - 16 * c));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = make_float4(y[4 * j], y[4 * j + 1], y[4 * j + 2], y[4 * j + 3]);
      f[j] = make_float4(y[15 - 4 * j], y[14 - 4 * j], y[13 - 4 * j], y[12 - 4 * j]);
    }
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// One wave per pair (images 2j and 2j+1 of the batch; rows B + 2j, B + 2j + 1 hold their mirrored copies).  The threshold table and
// the workgroup's histogram live in LDS; the histogram leaves with one integer atomic per non-zero bin.
__global__ __launch_bounds__(TAIL_THREADS) void verify_tail_kernel(const float* __restrict__ feat, int ldf, int B, int D, int pair0,
                                                                   int n_pairs, const double* __restrict__ thr, int n_thr,
                                                                   const int32_t* __restrict__ fold_start, int n_folds,
                                                                   const uint8_t* __restrict__ issame, int32_t* __restrict__ hist,
                                                                   double* __restrict__ norms, int norm_ld, double* __restrict__ dist_out,
                                                                   float* __restrict__ emb_out) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem[];
  double* s_thr = reinterpret_cast<double*>(smem);
  int32_t* s_hist = reinterpret_cast<int32_t*>(smem + (size_t)n_thr * sizeof(double));
  const int nbin = n_folds * 2 * (n_thr + 1);
  for (int k = threadIdx.x; k < n_thr; k += TAIL_THREADS) s_thr[k] = thr[k];
  for (int k = threadIdx.x; k < nbin; k += TAIL_THREADS) s_hist[k] = 0;
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = (D + 63) >> 6;
  const int n_local = B >> 1;
  for (int j = blockIdx.x * (TAIL_THREADS / 64) + wave; j < n_local; j += gridDim.x * (TAIL_THREADS / 64)) {
    const int pg = pair0 + j;
    if (pg >= n_pairs) break;
    double e[2][TAIL_MAX_D / 64];
    double nrm_e[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float* fo = feat + (size_t)(2 * j + i) * ldf;
      const float* ff = feat + (size_t)(B + 2 * j + i) * ldf;
      double so = 0.0, sf = 0.0, se = 0.0;
#pragma unroll
      for (int k = 0; k < TAIL_MAX_D / 64; ++k) {
        const int d = lane + 64 * k;
        double a = 0.0, b = 0.0;
        if (k < per && d < D) { a = (double)fo[d]; b = (double)ff[d]; }
        so += a * a;
        sf += b * b;
        e[i][k] = a + b;
        se += e[i][k] * e[i][k];
      }
      so = wave_sum_f64(so);
      sf = wave_sum_f64(sf);
      se = wave_sum_f64(se);
      const double nrm = sqrt(se);
      nrm_e[i] = nrm == 0.0 ? 1.0 : nrm;                 // sklearn.preprocessing.normalize: a zero row is left as it is
      if (lane == 0) {
        const size_t img = 2 * (size_t)pg + i;
        norms[img] = sqrt(so);
        norms[(size_t)norm_ld + img] = sqrt(sf);
      }
    }
    double dd = 0.0;
#pragma unroll
    for (int k = 0; k < TAIL_MAX_D / 64; ++k) {
      const int d = lane + 64 * k;
      const double a = e[0][k] / nrm_e[0], b = e[1][k] / nrm_e[1];
      if (emb_out != nullptr && k < per && d < D) {
        emb_out[(2 * (size_t)pg) * D + d] = (float)a;
        emb_out[(2 * (size_t)pg + 1) * D + d] = (float)b;
      }
      const double t = a - b;
      dd += t * t;
    }
    dd = wave_sum_f64(dd);
    if (lane == 0) {
      if (dist_out != nullptr) dist_out[pg] = dd;
      // k0 = #{k : thr[k] <= dist}: the pair is predicted "same" (dist < thr[k]) exactly for k >= k0.  NaN: never.
      int k0 = n_thr;
      if (dd == dd) {
        int lo = 0, hi = n_thr;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_thr[mid] <= dd) lo = mid + 1; else hi = mid;
        }
        k0 = lo;
      }
      int f = -1;
      for (int q = 0; q < n_folds; ++q)
        if (pg >= fold_start[q] && pg < fold_start[q + 1]) { f = q; break; }
      if (f >= 0) atomicAdd(&s_hist[(f * 2 + (issame[pg] ? 1 : 0)) * (n_thr + 1) + k0], 1);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nbin; k += TAIL_THREADS) {
    const int v = s_hist[k];
    if (v != 0) atomicAdd(&hist[k], v);
  }
}

}  // namespace

extern "C" int lafs_eval_flip_normalize(const uint8_t* src_u8, float* dst, int B, int S, float div, float mul, float add,
                                        hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(src_u8 && dst && B > 0 && S > 0 && S % 16 == 0, "S must be a positive multiple of 16");
  LAFS_CHECK_ARG(((uintptr_t)src_u8 & 15) == 0 && ((uintptr_t)dst & 15) == 0, "operands must be 16-byte aligned");
  const size_t total = (size_t)B * 3 * S * (S / 16);
  size_t blocks = (total + FLIP_THREADS - 1) / FLIP_THREADS;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(eval_flip_norm_kernel, dim3((unsigned)blocks), dim3(FLIP_THREADS), 0, stream, src_u8, dst, B, S, div, mul, add);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_verify_tail(const float* feat, int ldf, int B, int D, int pair0, int n_pairs, const double* thresholds, int n_thr,
                                const int32_t* fold_start, int n_folds, const uint8_t* issame, int32_t* hist, double* norms,
                                double* dist, float* emb, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(feat && thresholds && fold_start && issame && hist && norms, "bad operand");
  LAFS_CHECK_ARG(B > 0 && B % 2 == 0, "B must be a positive even number (pairs never straddle a batch)");
  LAFS_CHECK_ARG(D > 0 && D <= TAIL_MAX_D && ldf >= D, "D must be in [1, 1024] and ldf >= D");
  LAFS_CHECK_ARG(pair0 >= 0 && n_pairs > 0 && pair0 + B / 2 <= n_pairs, "the batch's pairs must lie inside [0, n_pairs)");
  LAFS_CHECK_ARG(n_thr > 0 && n_folds > 0, "bad threshold / fold count");
  const size_t lds = (size_t)n_thr * sizeof(double) + (size_t)n_folds * 2 * (n_thr + 1) * sizeof(int32_t);
  LAFS_CHECK_ARG(lds <= (size_t)TAIL_MAX_LDS, "threshold table + histogram exceed 64 KiB of LDS");
  const int waves = B / 2;
  int blocks = (waves + TAIL_THREADS / 64 - 1) / (TAIL_THREADS / 64);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(verify_tail_kernel, dim3(blocks), dim3(TAIL_THREADS), lds, stream, feat, ldf, B, D, pair0, n_pairs, thresholds, n_thr,
                     fold_start, n_folds, issame, hist, norms, 2 * n_pairs, dist, emb);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}
