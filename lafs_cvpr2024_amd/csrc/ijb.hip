// IJB-B / IJB-C template verification on the device: reference IJB_evaluation.py:198-247 (Embedding.get / forward_db), :501-535
// (image2template_feature), :541-567 (verification).  Three launches:
//   lafs_ijb_align_flip_normalize  packed u8 HWC loose crops + inverse affine maps -> f32 [2B,3,112,112] (aligned batch, then mirrored)
//   lafs_ijb_template_pool         f32 [N,2D] image features + CSR of (template, media, image) -> f32 sums [T,D], f64 unit rows [T,D]
//   lafs_ijb_pair_scores           f64 [T,D] unit rows + two index lists -> f64 [P] dot products
// lafs_cvpr2024_amd/ijb_evaluation.py builds the maps and the CSR on the host and turns the scores into the TAR@FAR table.
#include "common.hpp"
#include "lafs_hip.h"

// every float / double operation is rounded on its own: the float32 results are bit-identical to numpy's
#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int ALIGN_THREADS = 256;
constexpr int POOL_THREADS = 256;
constexpr int POOL_MAX_D = 1024;                        // four columns per thread
constexpr int PAIR_THREADS = 256;                       // 4 waves, one pair per wave at a time

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// One thread per output pixel (b, y, x), all three channels.  Operation order (tests/ijb_oracle.py performs the same float32 steps):
//   sx = (m0 * x + m1 * y) + m2,  sy = (m3 * x + m4 * y) + m5
//   a pixel whose (sx, sy) is not inside (-1, W) x (-1, H) has no tap in the image: value 0
//   x0 = floor(sx), fx = sx - x0, gx = 1 - fx (and the same in y); a tap outside the image reads 0
//   top = v00 * gx + v01 * fx,  bot = v10 * gx + v11 * fx,  v = top * gy + bot * fy
//   u = clamp(rint(v), 0, 255)  (nearest even),  out = u / div * mul + add
__global__ __launch_bounds__(ALIGN_THREADS) void ijb_align_kernel(const uint8_t* __restrict__ src, size_t src_bytes,
                                                                  const int64_t* __restrict__ offs, const int32_t* __restrict__ hw,
                                                                  const float* __restrict__ coef, int B, int S, float div, float mul,
                                                                  float add, float* __restrict__ dst, uint8_t* __restrict__ aligned) {
#pragma clang fp contract(off)
  const size_t total = (size_t)B * S * S;
  const size_t plane = (size_t)S * S;
  const size_t half = (size_t)B * 3 * plane;
  for (size_t i = (size_t)blockIdx.x * ALIGN_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * ALIGN_THREADS) {
    const int b = (int)(i / plane);
    const int r = (int)(i - (size_t)b * plane);
    const int y = r / S, x = r - y * S;
    const int H = hw[2 * b], W = hw[2 * b + 1];
    const int64_t off = offs[b];
    const float* m = coef + 6 * b;
    const float xf = (float)x, yf = (float)y;
    const float ax = m[0] * xf, bx = m[1] * yf, cx = ax + bx;
    const float sx = cx + m[2];
    const float ay = m[3] * xf, by = m[4] * yf, cy = ay + by;
    const float sy = cy + m[5];
    float u[3] = {0.f, 0.f, 0.f};
    const bool image_ok = H > 0 && W > 0 && off >= 0 && (size_t)off + (size_t)H * W * 3 <= src_bytes;
    if (image_ok && sx > -1.0f && sx < (float)W && sy > -1.0f && sy < (float)H) {
      const float x0f = floorf(sx), y0f = floorf(sy);
      const float fx = sx - x0f, fy = sy - y0f;
      const float gx = 1.0f - fx, gy = 1.0f - fy;
      const int x0 = (int)x0f, y0 = (int)y0f;
      const uint8_t* img = src + off;
      float v[2][2][3];
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int yy = y0 + dy, xx = x0 + dx;
          const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
          const size_t p = in ? ((size_t)yy * W + xx) * 3 : 0;
#pragma unroll
          for (int c = 0; c < 3; ++c) v[dy][dx][c] = in ? (float)img[p + c] : 0.0f;
        }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float t0 = v[0][0][c] * gx, t1 = v[0][1][c] * fx, top = t0 + t1;
        const float b0 = v[1][0][c] * gx, b1 = v[1][1][c] * fx, bot = b0 + b1;
        const float p0 = top * gy, p1 = bot * fy, val = p0 + p1;
        u[c] = fminf(fmaxf(rintf(val), 0.0f), 255.0f);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t row = ((size_t)b * 3 + c) * plane + (size_t)y * S;
      const float q = u[c] / div;
      const float s = q * mul;
      const float o = s + add;
      dst[row + x] = o;
      dst[half + row + (S - 1 - x)] = o;
      if (aligned != nullptr) aligned[row + x] = (uint8_t)u[c];
    }
  }
}

// One workgroup per template; thread t owns columns t, t + 256, t + 512, t + 768.  Per column, in float32 and in (media, image)
// order: x = (a + b) * s per image, sequential adds inside a media starting from its first image, one division by the count when it
// exceeds 1 (np.mean), sequential adds over the media starting from the first (np.sum).  Then float64: the row's sum of squares
// through LDS, one sqrt, one division per entry; a zero row is left as it is (sklearn.preprocessing.normalize).
__global__ __launch_bounds__(POOL_THREADS) void ijb_pool_kernel(const float* __restrict__ feats, int ldf, const float* __restrict__ faceness,
                                                                int n_img, const int32_t* __restrict__ order,
                                                                const int32_t* __restrict__ media_start, int n_media,
                                                                const int32_t* __restrict__ tmpl_start, int D, int flip, int det,
                                                                float* __restrict__ sums, double* __restrict__ unit) {
#pragma clang fp contract(off)
  __shared__ double s_part[POOL_THREADS / 64];
  const int t = blockIdx.x;
  const int tid = threadIdx.x;
  int m0 = tmpl_start[t], m1 = tmpl_start[t + 1];
  m0 = max(0, min(m0, n_media));
  m1 = max(m0, min(m1, n_media));
  float acc[POOL_MAX_D / POOL_THREADS] = {0.f, 0.f, 0.f, 0.f};
  for (int mi = m0; mi < m1; ++mi) {
    int i0 = media_start[mi], i1 = media_start[mi + 1];
    i0 = max(0, min(i0, n_img));
    i1 = max(i0, min(i1, n_img));
    float macc[POOL_MAX_D / POOL_THREADS] = {0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    for (int ii = i0; ii < i1; ++ii) {
      const int row = order[ii];
      if (row < 0 || row >= n_img) continue;               // (the host builds a permutation; never taken)
      const float* fr = feats + (size_t)row * ldf;
      const float s = faceness[row];
#pragma unroll
      for (int k = 0; k < POOL_MAX_D / POOL_THREADS; ++k) {
        const int d = tid + POOL_THREADS * k;
        if (d < D) {
          float x = fr[d];
          if (flip) x = x + fr[D + d];
          if (det) x = x * s;
          macc[k] = cnt == 0 ? x : macc[k] + x;
        }
      }
      ++cnt;
    }
    if (cnt == 0) continue;
    const float cf = (float)cnt;
#pragma unroll
    for (int k = 0; k < POOL_MAX_D / POOL_THREADS; ++k) {
      const float v = cnt > 1 ? macc[k] / cf : macc[k];
      acc[k] = mi == m0 ? v : acc[k] + v;
    }
  }
  double w[POOL_MAX_D / POOL_THREADS];
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < POOL_MAX_D / POOL_THREADS; ++k) {
    const int d = tid + POOL_THREADS * k;
    w[k] = d < D ? (double)acc[k] : 0.0;
    ss += w[k] * w[k];
  }
  ss = wave_sum_f64(ss);
  if ((tid & 63) == 0) s_part[tid >> 6] = ss;
  __syncthreads();
  double tot = 0.0;
#pragma unroll
  for (int q = 0; q < POOL_THREADS / 64; ++q) tot += s_part[q];
  const double nrm = sqrt(tot);
  const double den = nrm == 0.0 ? 1.0 : nrm;
#pragma unroll
  for (int k = 0; k < POOL_MAX_D / POOL_THREADS; ++k) {
    const int d = tid + POOL_THREADS * k;
    if (d < D) {
      sums[(size_t)t * D + d] = acc[k];
      unit[(size_t)t * D + d] = w[k] / den;
    }
  }
}

// One wave per pair, grid-stride.  A lane reads 16 bytes (two doubles) of each row per step, 1 KiB per wave and row; all the loads of
// a pair (12 per lane at D = 768) are independent and issued before the reduction.  A pair whose index is outside [0, T) scores NaN.
template <bool VEC>
__global__ __launch_bounds__(PAIR_THREADS) void ijb_pair_kernel(const double* __restrict__ unit, int T, int D, const int32_t* __restrict__ i1,
                                                                const int32_t* __restrict__ i2, size_t P, double* __restrict__ score) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const size_t wave = (size_t)blockIdx.x * (PAIR_THREADS / 64) + (threadIdx.x >> 6);
  const size_t n_waves = (size_t)gridDim.x * (PAIR_THREADS / 64);
  for (size_t p = wave; p < P; p += n_waves) {
    const int a = i1[p], b = i2[p];
    if (a < 0 || a >= T || b < 0 || b >= T) {
      if (lane == 0) score[p] = __longlong_as_double(0x7ff8000000000000LL);
      continue;
    }
    const double* ra = unit + (size_t)a * D;
    const double* rb = unit + (size_t)b * D;
    double s = 0.0;
    if (VEC) {
      const double2* va = reinterpret_cast<const double2*>(ra);
      const double2* vb = reinterpret_cast<const double2*>(rb);
      const int n2 = D >> 1;
#pragma unroll 8
      for (int k = lane; k < n2; k += 64) {
        const double2 x = va[k], y = vb[k];
        const double p0 = x.x * y.x, p1 = x.y * y.y;
        s += p0;
        s += p1;
      }
    } else {
      for (int k = lane; k < D; k += 64) {
        const double p0 = ra[k] * rb[k];
        s += p0;
      }
    }
    s = wave_sum_f64(s);
    if (lane == 0) score[p] = s;
  }
}

// ---- 1:N search.  One workgroup (4 waves) owns SR_TQ = 64 probes, wave w the 16 probes 16 w .. 16 w + 15.  The gallery list is
// streamed in tiles of SR_TG = 64 positions; a tile is a 64 x 64 float64 GEMM block over D in chunks of SR_KC = 32 columns: both
// operands' chunks go through LDS (rows of SR_LD = 34 doubles: the 16 rows x 2 columns a half wave reads cover the 64 banks once),
// the next chunk is fetched into registers while v_mfma_f64_16x16x4_f64 works on the current one.  Lane l supplies
// A[probe l & 15][k = l >> 4] and B[k = l >> 4][gallery l & 15] and receives C[probe (l >> 4) + 4 reg][gallery l & 15] (the f64 map).
// Summation order of every score: chunks in order, four columns per MFMA in order, the columns from D up to the next multiple of 32
// are zeros -- the same instruction sequence for every (probe, gallery) pair, so the same rows give the same bits anywhere.
// The mates' scores come from one more tile in front of the stream whose row j is the mate of probe j (the diagonal of that block),
// through the very same code.  After a tile the wave parks its 16 x 64 scores in LDS (over the operand chunks) and lane p < 16 walks
// probe p's row in position order: counts what precedes the mate, keeps the best non-mate, and inserts into the probe's sorted top-k
// list (LDS, [64][k]); the Q x G matrix never exists.  Results leave in the epilogue through plain stores.
constexpr int SR_THREADS = 256;
constexpr int SR_TQ = 64, SR_TG = 64, SR_KC = 32, SR_LD = 34, SR_SLD = 65, SR_MAX_K = 64;
constexpr int SR_ROWS = SR_THREADS / SR_KC;            // 8 rows of a chunk per pass of the workgroup
constexpr int SR_PASSES = SR_TQ / SR_ROWS;             // 8 values per thread, chunk and operand
static_assert(SR_TQ == SR_TG && 4 * 16 * SR_SLD <= (SR_TQ + SR_TG) * SR_LD, "the score scratch lies over the operand chunks");
typedef __attribute__((ext_vector_type(4))) double f64x4_t;

__device__ __forceinline__ double qnan_f64() { return __longlong_as_double(0x7ff8000000000000LL); }

// the ranking order: larger score first, equal scores by position, NaN after every number (among NaNs by position)
__device__ __forceinline__ bool rank_before(double a, int ia, double b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na || nb) return na ? (nb && ia < ib) : true;
  return a > b || (a == b && ia < ib);
}

// rows[i] >= 0: a row of unit; -1: NaN (an index outside the table); -2: zeros (no such row)
__device__ __forceinline__ void sr_fetch(const double* __restrict__ unit, int D, const int (&rows)[SR_PASSES], int col, double (&v)[SR_PASSES]) {
#pragma unroll
  for (int i = 0; i < SR_PASSES; ++i) {
    const int r = rows[i];
    v[i] = (r >= 0 && col < D) ? unit[(size_t)r * D + col] : (r == -1 ? qnan_f64() : 0.0);
  }
}

__global__ __launch_bounds__(SR_THREADS) void ijb_search_kernel(const double* __restrict__ unit, int T, int D,
                                                                const int32_t* __restrict__ probe_idx, int Q,
                                                                const int32_t* __restrict__ gallery_idx, int G,
                                                                const int32_t* __restrict__ mate, int k, double* __restrict__ top_score,
                                                                int32_t* __restrict__ top_idx, double* __restrict__ mate_score,
                                                                int32_t* __restrict__ mate_rank, double* __restrict__ best_nonmate) {
  extern __shared__ __align__(16) unsigned char sr_lds[];
  __shared__ int32_t s_mpos[SR_TQ];
  double* sP = reinterpret_cast<double*>(sr_lds);        // [SR_TQ][SR_LD]
  double* sG = sP + SR_TQ * SR_LD;                       // [SR_TG][SR_LD]
  double* sLs = sG + SR_TG * SR_LD;                      // [SR_TQ][k] list scores
  int32_t* sLi = reinterpret_cast<int32_t*>(sLs + SR_TQ * k);   // [SR_TQ][k] list positions
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double* sS = sP + w * 16 * SR_SLD;                     // [16][SR_SLD] of this wave, valid between the barriers after a tile
  const int q0 = blockIdx.x * SR_TQ;                     // (the host keeps the grid inside int)

  if (tid < SR_TQ) {
    int m = -1;
    if (q0 + tid < Q) {
      m = mate[q0 + tid];
      if (m < 0 || m >= G) m = -1;
    }
    s_mpos[tid] = m;
  }
  __syncthreads();

  const int r0 = tid / SR_KC, cl = tid % SR_KC;
  int prow[SR_PASSES], grow[SR_PASSES];
#pragma unroll
  for (int i = 0; i < SR_PASSES; ++i) {
    const int q = q0 + r0 + SR_ROWS * i;
    const int pi = q < Q ? probe_idx[q] : -1;
    prow[i] = (pi >= 0 && pi < T) ? pi : -2;
  }
  auto tile_rows = [&](int t) {                          // t = -1: the mates of this workgroup's probes
#pragma unroll
    for (int i = 0; i < SR_PASSES; ++i) {
      const int row = r0 + SR_ROWS * i;
      int pos = t < 0 ? s_mpos[row] : t * SR_TG + row;
      if (pos >= G) pos = -1;
      int r = -2;
      if (pos >= 0) {
        const int gi = gallery_idx[pos];
        r = (gi >= 0 && gi < T) ? gi : -1;
      }
      grow[i] = r;
    }
  };

  // selection state of probe p = lane of this wave (lanes 0 .. 15)
  const int my_row = w * 16 + (lane & 15);
  const bool sel = lane < 16 && q0 + my_row < Q;
  const int mpos = s_mpos[my_row];
  double ms = qnan_f64(), thr_s = 0.0, bn_s = qnan_f64();
  int thr_i = -1, bn_i = -1, cnt = 0, rank = 0;
  double* Ls = sLs + my_row * k;
  int32_t* Li = sLi + my_row * k;

  const int n_tiles = (G + SR_TG - 1) / SR_TG;
  const int n_chunks = (D + SR_KC - 1) / SR_KC;
  double pv[SR_PASSES], gv[SR_PASSES];
  tile_rows(-1);
  sr_fetch(unit, D, prow, cl, pv);
  sr_fetch(unit, D, grow, cl, gv);

  for (int t = -1; t < n_tiles; ++t) {
    f64x4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < n_chunks; ++c) {
      __syncthreads();                                   // the chunk (or the score scratch) in LDS has been read
#pragma unroll
      for (int i = 0; i < SR_PASSES; ++i) {
        sP[(r0 + SR_ROWS * i) * SR_LD + cl] = pv[i];
        sG[(r0 + SR_ROWS * i) * SR_LD + cl] = gv[i];
      }
      __syncthreads();
      if (c + 1 < n_chunks) {
        sr_fetch(unit, D, prow, (c + 1) * SR_KC + cl, pv);
        sr_fetch(unit, D, grow, (c + 1) * SR_KC + cl, gv);
      } else if (t + 1 < n_tiles) {
        tile_rows(t + 1);
        sr_fetch(unit, D, prow, cl, pv);
        sr_fetch(unit, D, grow, cl, gv);
      }
      const double* pa = sP + (w * 16 + (lane & 15)) * SR_LD + (lane >> 4);
      const double* pb = sG + (lane & 15) * SR_LD + (lane >> 4);
#pragma unroll
      for (int kk = 0; kk < SR_KC / 4; ++kk) {
        const double a = pa[4 * kk];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, pb[j * 16 * SR_LD + 4 * kk], acc[j], 0, 0, 0);
      }
    }
    __syncthreads();                                     // every wave has read the last chunk: its place becomes the score scratch
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) sS[((lane >> 4) + 4 * r) * SR_SLD + 16 * j + (lane & 15)] = acc[j][r];
    __syncthreads();
    if (sel) {
      const double* row = sS + lane * SR_SLD;
      if (t < 0) {
        ms = row[my_row];                                // row j of the mate tile is the mate of probe j
      } else {
        const int g0 = t * SR_TG;
        const int n = min(SR_TG, G - g0);
        for (int j = 0; j < n; ++j) {
          const int pos = g0 + j;
          double s = row[j];
          if (s != s) s = qnan_f64();
          if (pos != mpos) {
            if (mpos >= 0 && rank_before(s, pos, ms, mpos)) ++rank;
            if (bn_i < 0 || rank_before(s, pos, bn_s, bn_i)) { bn_s = s; bn_i = pos; }
          }
          if (cnt < k || rank_before(s, pos, thr_s, thr_i)) {
            int i = cnt < k ? cnt : k - 1;
            while (i > 0 && rank_before(s, pos, Ls[i - 1], Li[i - 1])) {
              Ls[i] = Ls[i - 1];
              Li[i] = Li[i - 1];
              --i;
            }
            Ls[i] = s;
            Li[i] = pos;
            if (cnt < k) ++cnt;
            thr_s = Ls[cnt - 1];
            thr_i = Li[cnt - 1];
          }
        }
      }
    }
  }

  if (sel) {
    const int q = q0 + my_row;
    const int pi = probe_idx[q];
    const bool ok = pi >= 0 && pi < T;
    for (int i = 0; i < k; ++i) {
      const bool have = ok && i < cnt;
      top_score[(size_t)q * k + i] = have ? Ls[i] : qnan_f64();
      top_idx[(size_t)q * k + i] = have ? Li[i] : -1;
    }
    const bool mated = ok && mpos >= 0;
    mate_score[q] = mated ? (ms != ms ? qnan_f64() : ms) : qnan_f64();
    mate_rank[q] = mated ? rank : -1;
    best_nonmate[q] = (ok && bn_i >= 0) ? bn_s : qnan_f64();
  }
}

}  // namespace

extern "C" int lafs_ijb_align_flip_normalize(const uint8_t* src_u8, int64_t src_bytes, const int64_t* offsets, const int32_t* hw,
                                             const float* inv_maps, int B, int S, float div, float mul, float add, float* dst,
                                             uint8_t* aligned_u8, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(src_u8 && offsets && hw && inv_maps && dst, "bad operand");
  LAFS_CHECK_ARG(B > 0 && S > 0 && S <= 1024 && src_bytes > 0, "B, S and src_bytes must be positive (S <= 1024)");
  const size_t total = (size_t)B * S * S;
  size_t blocks = (total + ALIGN_THREADS - 1) / ALIGN_THREADS;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(ijb_align_kernel, dim3((unsigned)blocks), dim3(ALIGN_THREADS), 0, stream, src_u8, (size_t)src_bytes, offsets, hw,
                     inv_maps, B, S, div, mul, add, dst, aligned_u8);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_ijb_template_pool(const float* feats, int ldf, const float* faceness, int n_images, const int32_t* order,
                                      const int32_t* media_start, int n_media, const int32_t* template_start, int n_templates, int D,
                                      int flip, int detector_score, float* sums, double* unit, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(feats && faceness && order && media_start && template_start && sums && unit, "bad operand");
  LAFS_CHECK_ARG(n_images > 0 && n_media > 0 && n_media <= n_images && n_templates > 0 && n_templates <= n_media,
                 "need 0 < n_templates <= n_media <= n_images");
  LAFS_CHECK_ARG(D > 0 && D <= POOL_MAX_D && ldf >= (flip ? 2 * D : D), "D must be in [1, 1024] and ldf >= 2 D (D without the flip copy)");
  hipLaunchKernelGGL(ijb_pool_kernel, dim3((unsigned)n_templates), dim3(POOL_THREADS), 0, stream, feats, ldf, faceness, n_images, order,
                     media_start, n_media, template_start, D, flip ? 1 : 0, detector_score ? 1 : 0, sums, unit);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_ijb_pair_scores(const double* unit, int n_templates, int D, const int32_t* idx1, const int32_t* idx2, int64_t n_pairs,
                                    double* scores, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(unit && idx1 && idx2 && scores, "bad operand");
  LAFS_CHECK_ARG(n_templates > 0 && D > 0 && n_pairs > 0, "n_templates, D and n_pairs must be positive");
  const size_t per = PAIR_THREADS / 64;
  size_t blocks = ((size_t)n_pairs + per - 1) / per;
  if (blocks > 256 * 8) blocks = 256 * 8;                // 8 workgroups = 32 waves per CU: every wave slot holds one pair's 12 loads
  const bool vec = D % 2 == 0 && ((uintptr_t)unit & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(ijb_pair_kernel<true>, dim3((unsigned)blocks), dim3(PAIR_THREADS), 0, stream, unit, n_templates, D, idx1, idx2,
                       (size_t)n_pairs, scores);
  else
    hipLaunchKernelGGL(ijb_pair_kernel<false>, dim3((unsigned)blocks), dim3(PAIR_THREADS), 0, stream, unit, n_templates, D, idx1, idx2,
                       (size_t)n_pairs, scores);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int64_t lafs_ijb_search_workspace(int n_probes, int n_gallery, int k) {
  (void)n_probes; (void)n_gallery; (void)k;
  return 0;                                              // the running lists live in LDS; nothing is merged across workgroups
}

extern "C" int lafs_ijb_search(const double* unit, int n_templates, int D, const int32_t* probe_idx, int n_probes,
                               const int32_t* gallery_idx, int n_gallery, const int32_t* mate, int k, double* top_score, int32_t* top_idx,
                               double* mate_score, int32_t* mate_rank, double* best_nonmate, void* workspace, size_t workspace_bytes,
                               hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(unit && probe_idx && gallery_idx && mate && top_score && top_idx && mate_score && mate_rank && best_nonmate, "bad operand");
  LAFS_CHECK_ARG(n_templates > 0 && n_probes > 0 && n_gallery > 0, "n_templates, n_probes and n_gallery must be positive");
  LAFS_CHECK_ARG(D >= 1 && D <= POOL_MAX_D, "D must be in [1, 1024]");
  LAFS_CHECK_ARG(k >= 1 && k <= SR_MAX_K, "k must be in [1, 64]");
  const size_t need = (size_t)lafs_ijb_search_workspace(n_probes, n_gallery, k);
  LAFS_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace != nullptr), "workspace smaller than lafs_ijb_search_workspace()");
  const size_t lds = (size_t)(SR_TQ + SR_TG) * SR_LD * sizeof(double) + (size_t)SR_TQ * k * (sizeof(double) + sizeof(int32_t));
  {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ijb_search_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { lafs_set_error("lafs_ijb_search: cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e)); return (int)e; }
  }
  const unsigned blocks = (unsigned)(((size_t)n_probes + SR_TQ - 1) / SR_TQ);
  hipLaunchKernelGGL(ijb_search_kernel, dim3(blocks), dim3(SR_THREADS), lds, stream, unit, n_templates, D, probe_idx, n_probes, gallery_idx,
                     n_gallery, mate, k, top_score, top_idx, mate_score, mate_rank, best_nonmate);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}
