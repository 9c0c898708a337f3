// Weighted k-NN on frozen features (DINO's eval_knn.py protocol; no counterpart in the reference).  Three launches at most:
//   knn_search_kernel   f32 bank rows x f32 query rows -> per (query, bank split) the first k positions of the ranking order
//   knn_merge_kernel    the splits' partial lists (and, with merge, the caller's earlier result) -> one list per query
//   knn_vote_kernel     a list + the bank's labels -> the five best classes of the exp(score / T)-weighted vote, per ks[i]
// lafs_cvpr2024_amd/knn.py streams the bank through lafs_knn_search in chunks and turns the votes into top-1 / top-5 accuracies.
#include "common.hpp"
#include "lafs_hip.h"

namespace {

// ---- search.  One workgroup (4 waves) owns KN_TQ = 64 queries and streams its share of the bank in tiles of KN_TB = 128 rows; a
// tile is a 64 x 128 f32 GEMM block over D in chunks of KN_KC = 32 columns.  Both operands' chunks go through LDS (rows of
// KN_LD = 33 floats: the 32 rows a half wave reads at one column cover the 32 banks once); the next chunk is fetched into registers
// while v_mfma_f32_32x32x2_f32 works on the current one.  Wave w computes queries 32 (w & 1) .. + 31 against tile rows
// 64 (w >> 1) .. + 63 as two 32 x 32 accumulators.  Lane l supplies A[query l & 31][k = l >> 5] and B[k = l >> 5][row l & 31] and
// receives C[query (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)][row l & 31].
// Summation order of every score: chunks in order, two columns per MFMA in order (a k-ordered fmaf chain from 0), the columns
// from D up to the next multiple of 32 are zeros -- the same instruction sequence for every (query, bank row) pair, so the same two
// rows give the same 32 bits in any tile, workgroup, chunk or split.
// After a tile the waves park the 64 x 128 scores in LDS (over the operand chunks) and wave w selects for queries 16 w .. 16 w + 15,
// one query at a time: the 64 lanes compare two candidates each against the query's k-th entry (held by lane `query & 15` in
// registers) and ballot.  An empty ballot -- almost every one after the first tiles -- ends the query's turn.  A survivor is
// inserted by the whole wave: lane j holds list entries j, j + 64, j + 128, j + 192, a popcount of "ranks before the candidate"
// gives the slot, the entries behind it move down by one.  The lists live in global memory ([k] per query: the output rows
// themselves, or this split's rows of the workspace) and stay in L2; only their owner wave touches them.
constexpr int KN_THREADS = 256;
constexpr int KN_TQ = 64, KN_TB = 128, KN_KC = 32, KN_LD = 33, KN_SLD = 129;
constexpr int KN_MAX_K = 256, KN_MAX_D = 1024, KN_MAX_SPLITS = 32, KN_PER_LANE = KN_MAX_K / 64;
constexpr int KN_OPERAND_FLOATS = (KN_TQ + KN_TB) * KN_LD, KN_SCORE_FLOATS = KN_TQ * KN_SLD;
constexpr int KN_LDS_FLOATS = KN_OPERAND_FLOATS > KN_SCORE_FLOATS ? KN_OPERAND_FLOATS : KN_SCORE_FLOATS;
constexpr int KN_VOTE_THREADS = 256, KN_MAX_KS = 8, KN_TOP = 5;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

struct knn_ks { int n; int v[KN_MAX_KS]; };

__device__ __forceinline__ float qnan_f32() { return __int_as_float(0x7fc00000); }

// the ranking order: larger score first, equal scores by position, NaN after every number (among NaNs by position)
__device__ __forceinline__ bool knn_before(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na || nb) return na ? (nb && ia < ib) : true;
  return a > b || (a == b && ia < ib);
}

// four columns col .. col + 3 of one row; row < 0 or a column >= D reads nothing and gives 0
__device__ __forceinline__ void knn_fetch(const float* __restrict__ base, int ld, int row, int col, int D, float (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.0f;
  if (row < 0 || col >= D) return;
  const float* p = base + (size_t)row * ld + col;
  if (col + 4 <= D) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (col + j < D) v[j] = p[j];
  }
}

__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }

// The wave inserts (s, pos) into the sorted list Ls / Li of `cnt` entries (at most k are kept); cnt, ts, ti (the k-th entry once the
// list is full) are wave-uniform and updated.  The candidate ranks before the k-th entry or the list is not full.
__device__ __forceinline__ void knn_insert(float* Ls, int32_t* Li, int k, int lane, float s, int pos, int& cnt, float& ts, int& ti) {
  float es[KN_PER_LANE];
  int ei[KN_PER_LANE];
  int p = 0;
  const int per = (k + 63) >> 6;
#pragma unroll
  for (int m = 0; m < KN_PER_LANE; ++m) {
    es[m] = 0.0f; ei[m] = -1;
    if (m < per) {
      const int i = lane + 64 * m;
      const bool have = i < cnt;
      if (have) { es[m] = Ls[i]; ei[m] = Li[i]; }
      p += wave_count(have && knn_before(es[m], ei[m], s, pos));
    }
  }
#pragma unroll
  for (int m = 0; m < KN_PER_LANE; ++m) {
    if (m < per) {
      const int i = lane + 64 * m;
      if (i < cnt && i >= p && i + 1 < k) { Ls[i + 1] = es[m]; Li[i + 1] = ei[m]; }
    }
  }
  if (lane == 0) { Ls[p] = s; Li[p] = pos; }
  if (cnt < k) ++cnt;
  if (cnt == k) {
    if (p == k - 1) {
      ts = s; ti = pos;
    } else {                                               // the old entry k - 2 is the new last one
      const int j = k - 2, m2 = j >> 6, l2 = j & 63;
      float fs = es[0];
      int fi = ei[0];
#pragma unroll
      for (int m = 1; m < KN_PER_LANE; ++m)
        if (m2 == m) { fs = es[m]; fi = ei[m]; }
      ts = __shfl(fs, l2, 64);
      ti = __shfl(fi, l2, 64);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the next insert of this wave reads what this one wrote
}

__global__ __launch_bounds__(KN_THREADS) void knn_search_kernel(const float* __restrict__ bank, int ldb, int n_bank, int pos0,
                                                                const float* __restrict__ query, int ldq, int Q, int D, int k,
                                                                const int32_t* __restrict__ exclude, int seeded, int tiles_per_split,
                                                                float* out_s, int32_t* out_i, size_t split_stride) {
  extern __shared__ __align__(16) unsigned char kn_lds[];
  float* sQ = reinterpret_cast<float*>(kn_lds);            // [KN_TQ][KN_LD]
  float* sB = sQ + KN_TQ * KN_LD;                          // [KN_TB][KN_LD]
  float* sS = sQ;                                          // [KN_TQ][KN_SLD], valid between the barriers after a tile
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int q0 = blockIdx.x * KN_TQ;
  const int n_tiles = (n_bank + KN_TB - 1) / KN_TB;
  const int t0 = min(n_tiles, (int)blockIdx.y * tiles_per_split);
  const int t1 = min(n_tiles, t0 + tiles_per_split);
  out_s += (size_t)blockIdx.y * split_stride;
  out_i += (size_t)blockIdx.y * split_stride;

  // selection state of query 16 w + lane (lanes 0 .. 15)
  const int my_q = q0 + w * 16 + (lane & 15);
  int cnt = 0, thi = -1, exc = -1;
  float ths = 0.0f;
  if (my_q < Q && exclude != nullptr) exc = exclude[my_q];
  if (seeded) {                                            // the rows already hold a valid result: go on from it
    for (int qi = 0; qi < 16; ++qi) {
      const int q = q0 + w * 16 + qi;
      if (q >= Q) break;
      const int32_t* Li = out_i + (size_t)q * k;
      int c = 0;
      for (int i = lane; i < k + lane; i += 64) c += wave_count(i < k && Li[i] >= 0);
      if (lane == qi) {
        cnt = c;
        if (c == k) { ths = out_s[(size_t)q * k + k - 1]; thi = Li[k - 1]; }
      }
    }
  }

  const int r = tid >> 3, c4 = (tid & 7) * 4;
  int qrow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) qrow[i] = q0 + r + 32 * i < Q ? q0 + r + 32 * i : -1;
  const int n_chunks = (D + KN_KC - 1) / KN_KC;
  float qv[2][4], bv[4][4];
  auto fetch = [&](int t, int c) {
#pragma unroll
    for (int i = 0; i < 2; ++i) knn_fetch(query, ldq, qrow[i], c * KN_KC + c4, D, qv[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long row = (long long)t * KN_TB + r + 32 * i;
      knn_fetch(bank, ldb, row < n_bank ? (int)row : -1, c * KN_KC + c4, D, bv[i]);
    }
  };
  if (t0 < t1) fetch(t0, 0);

  const int qh = w & 1, bh = w >> 1;
  for (int t = t0; t < t1; ++t) {
    f32x16_t acc0, acc1;
#pragma unroll
    for (int j = 0; j < 16; ++j) { acc0[j] = 0.0f; acc1[j] = 0.0f; }
    for (int c = 0; c < n_chunks; ++c) {
      __syncthreads();                                     // the chunk (or the score scratch) in LDS has been read
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) sQ[(r + 32 * i) * KN_LD + c4 + j] = qv[i][j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) sB[(r + 32 * i) * KN_LD + c4 + j] = bv[i][j];
      __syncthreads();
      if (c + 1 < n_chunks) fetch(t, c + 1);
      else if (t + 1 < t1) fetch(t + 1, 0);
      const float* pa = sQ + (qh * 32 + (lane & 31)) * KN_LD + (lane >> 5);
      const float* pb = sB + (bh * 64 + (lane & 31)) * KN_LD + (lane >> 5);
#pragma unroll
      for (int kk = 0; kk < KN_KC / 2; ++kk) {
        const float a = pa[2 * kk];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pb[2 * kk], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pb[32 * KN_LD + 2 * kk], acc1, 0, 0, 0);
      }
    }
    __syncthreads();                                       // every wave has read the last chunk: its place becomes the score scratch
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int row = qh * 32 + (j & 3) + 8 * (j >> 2) + 4 * (lane >> 5);
      sS[row * KN_SLD + bh * 64 + (lane & 31)] = acc0[j];
      sS[row * KN_SLD + bh * 64 + 32 + (lane & 31)] = acc1[j];
    }
    __syncthreads();

    for (int qi = 0; qi < 16; ++qi) {
      const int q = q0 + w * 16 + qi;
      if (q >= Q) break;
      int c = __shfl(cnt, qi, 64), ti = __shfl(thi, qi, 64);
      float ts = __shfl(ths, qi, 64);
      const int ex = __shfl(exc, qi, 64);
      float* Ls = out_s + (size_t)q * k;
      int32_t* Li = out_i + (size_t)q * k;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const long long row = (long long)t * KN_TB + h * 64 + lane;
        const int pos = (int)(pos0 + row);                 // (meaningful where row < n_bank)
        float s = sS[(w * 16 + qi) * KN_SLD + h * 64 + lane];
        if (s != s) s = qnan_f32();
        const bool ok = row < n_bank && pos != ex && (c < k || knn_before(s, pos, ts, ti));
        unsigned long long mask = __ballot(ok);
        while (mask) {                                     // ascending positions; the k-th entry moves with every insert
          const int b = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          const float cs = __shfl(s, b, 64);
          const int cp = (int)((long long)pos0 + (long long)t * KN_TB + h * 64 + b);
          if (c < k || knn_before(cs, cp, ts, ti)) knn_insert(Ls, Li, k, lane, cs, cp, c, ts, ti);
        }
      }
      if (lane == qi) { cnt = c; ths = ts; thi = ti; }
    }
  }

  for (int qi = 0; qi < 16; ++qi) {                        // fewer than k candidates: idx -1, score NaN
    const int q = q0 + w * 16 + qi;
    if (q >= Q) break;
    const int c = __shfl(cnt, qi, 64);
    for (int i = c + lane; i < k; i += 64) {
      out_s[(size_t)q * k + i] = qnan_f32();
      out_i[(size_t)q * k + i] = -1;
    }
  }
}

// ---- merge.  One workgroup per query.  The n_lists sorted lists (the splits' rows of the workspace, then with_old: the output
// row itself) are copied to LDS; an entry's place in the result is its place in its own list plus, per other list, the number of
// entries that rank before it (a binary search: the positions are distinct, so the order is total and the places are too).
__global__ __launch_bounds__(KN_THREADS) void knn_merge_kernel(const float* __restrict__ ws_s, const int32_t* __restrict__ ws_i,
                                                               size_t split_stride, int splits, int with_old, int k, float* out_s,
                                                               int32_t* out_i) {
  extern __shared__ __align__(16) unsigned char kn_lds[];
  const int nl = splits + (with_old ? 1 : 0);
  float* ls = reinterpret_cast<float*>(kn_lds);            // [nl][k]
  int32_t* li = reinterpret_cast<int32_t*>(ls + nl * k);   // [nl][k]
  float* os = reinterpret_cast<float*>(li + nl * k);       // [k]
  int32_t* oi = reinterpret_cast<int32_t*>(os + k);        // [k]
  int32_t* ln = oi + k;                                    // [nl] valid entries per list
  const int tid = threadIdx.x;
  const size_t q = blockIdx.x;
  for (int e = tid; e < nl * k; e += KN_THREADS) {
    const int a = e / k, i = e - a * k;
    const bool old = a == splits;
    ls[e] = old ? out_s[q * k + i] : ws_s[a * split_stride + q * k + i];
    li[e] = old ? out_i[q * k + i] : ws_i[a * split_stride + q * k + i];
  }
  for (int i = tid; i < k; i += KN_THREADS) { os[i] = qnan_f32(); oi[i] = -1; }
  __syncthreads();
  for (int a = tid; a < nl; a += KN_THREADS) {
    int lo = 0, hi = k;                                    // the first idx < 0
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (li[a * k + mid] >= 0) lo = mid + 1; else hi = mid;
    }
    ln[a] = lo;
  }
  __syncthreads();
  for (int e = tid; e < nl * k; e += KN_THREADS) {
    const int a = e / k, i = e - a * k;
    if (i >= ln[a]) continue;
    const float s = ls[e];
    const int idx = li[e];
    int place = i;
    for (int b = 0; b < nl && place < k; ++b) {
      if (b == a) continue;
      int lo = 0, hi = ln[b];
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (knn_before(ls[b * k + mid], li[b * k + mid], s, idx)) lo = mid + 1; else hi = mid;
      }
      place += lo;
    }
    if (place < k) { os[place] = s; oi[place] = idx; }
  }
  __syncthreads();
  for (int i = tid; i < k; i += KN_THREADS) { out_s[q * k + i] = os[i]; out_i[q * k + i] = oi[i]; }
}

// ---- vote.  One wave per query.  Entry j of the list carries label lab[j] and weight exp(score / T) (no label: idx < 0 or
// idx >= n_label).  For ks[i]: lane j's entries (j, j + 64, ..) each walk the first ks[i] entries in order, add up the weights of
// their own label (the same sequence of additions for every entry of a class) and learn whether an earlier entry has it; the first
// entry of each class stands for it.  Five rounds of a wave-wide "best (vote, label)" pick the output.  Cost: O(ks^2 / 64) per
// query, whatever the number of identities.
__global__ __launch_bounds__(KN_VOTE_THREADS) void knn_vote_kernel(const float* __restrict__ top_s, const int32_t* __restrict__ top_i,
                                                                   int Q, int k, const int32_t* __restrict__ label, int64_t n_label,
                                                                   knn_ks ks, float temperature, int32_t* __restrict__ pred,
                                                                   float* __restrict__ vote) {
  __shared__ float s_w[KN_VOTE_THREADS / 64][KN_MAX_K];
  __shared__ int32_t s_l[KN_VOTE_THREADS / 64][KN_MAX_K];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = blockIdx.x * (KN_VOTE_THREADS / 64) + w;
  if (q >= Q) return;                                      // (no barrier below: the waves are independent)
  float* W = s_w[w];
  int32_t* L = s_l[w];
  for (int j = lane; j < k; j += 64) {
    const int idx = top_i[(size_t)q * k + j];
    const bool have = idx >= 0 && (int64_t)idx < n_label;
    L[j] = have ? label[idx] : -1;
    W[j] = have ? expf(top_s[(size_t)q * k + j] / temperature) : 0.0f;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  for (int n = 0; n < ks.n; ++n) {
    const int kn = ks.v[n];
    float cv[KN_PER_LANE];
    int cl[KN_PER_LANE];
#pragma unroll
    for (int m = 0; m < KN_PER_LANE; ++m) {
      const int j = lane + 64 * m;
      cv[m] = 0.0f; cl[m] = -1;
      if (j < kn && L[j] >= 0) {
        const int mine = L[j];
        bool first = true;
        float sum = 0.0f;
        for (int i = 0; i < kn; ++i)
          if (L[i] == mine) {
            if (i < j) first = false;
            sum += W[i];
          }
        if (first) { cv[m] = sum; cl[m] = mine; }
      }
    }
    for (int o = 0; o < KN_TOP; ++o) {
      // larger vote first, then smaller label; label -1: no class
      float bv = 0.0f;
      int bl = -1, bm = -1;
#pragma unroll
      for (int m = 0; m < KN_PER_LANE; ++m)
        if (cl[m] >= 0 && (bl < 0 || cv[m] > bv || (cv[m] == bv && cl[m] < bl))) { bv = cv[m]; bl = cl[m]; bm = m; }
      float rv = bv;
      int rl = bl;
#pragma unroll
      for (int x = 32; x >= 1; x >>= 1) {
        const float ov = __shfl_xor(rv, x, 64);
        const int ol = __shfl_xor(rl, x, 64);
        if (ol >= 0 && (rl < 0 || ov > rv || (ov == rv && ol < rl))) { rv = ov; rl = ol; }
      }
      if (rl >= 0 && rl == bl) {                           // a class has one standing entry: exactly one lane drops it
#pragma unroll
        for (int m = 0; m < KN_PER_LANE; ++m)
          if (m == bm) cl[m] = -1;
      }
      if (lane == 0) {
        const size_t at = ((size_t)n * Q + q) * KN_TOP + o;
        pred[at] = rl;
        vote[at] = rl >= 0 ? rv : 0.0f;
      }
    }
  }
}

int knn_cu_count() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      cus = n;
    else
      return 256;
  }
  return cus;
}

// the number of bank splits a call runs with: a function of the shape and the device alone
int knn_splits(int n_query, int64_t n_bank, int splits) {
  const int64_t tiles = (n_bank + KN_TB - 1) / KN_TB;
  const int64_t groups = ((int64_t)n_query + KN_TQ - 1) / KN_TQ;
  int64_t s = splits;
  if (s <= 0) {                                            // two workgroups per CU, or what the queries give on their own
    const int64_t want = 2 * (int64_t)knn_cu_count();
    s = groups >= want ? 1 : (want + groups - 1) / groups;
  }
  if (s > KN_MAX_SPLITS) s = KN_MAX_SPLITS;
  if (s > tiles) s = tiles;
  return s < 1 ? 1 : (int)s;
}

}  // namespace

extern "C" int64_t lafs_knn_workspace(int n_query, int64_t n_bank, int k, int splits) {
  if (n_query <= 0 || n_bank <= 0 || k <= 0) return 0;
  const int s = knn_splits(n_query, n_bank, splits);
  return s > 1 ? (int64_t)s * n_query * k * (int64_t)(sizeof(float) + sizeof(int32_t)) : 0;
}

extern "C" int lafs_knn_search(const float* bank, int ldb, int64_t n_bank, int64_t bank_pos0, const float* query, int ldq, int n_query,
                               int D, int k, const int32_t* exclude, int merge, int splits, float* top_score, int32_t* top_idx,
                               void* workspace, size_t workspace_bytes, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(bank && query && top_score && top_idx, "bad operand");
  LAFS_CHECK_ARG(n_bank > 0 && n_query > 0 && bank_pos0 >= 0 && bank_pos0 + n_bank < ((int64_t)1 << 31),
                 "n_bank and n_query must be positive, bank_pos0 >= 0 and bank_pos0 + n_bank < 2^31");
  LAFS_CHECK_ARG(D >= 1 && D <= KN_MAX_D, "D must be in [1, 1024]");
  LAFS_CHECK_ARG(k >= 1 && k <= KN_MAX_K, "k must be in [1, 256]");
  LAFS_CHECK_ARG(splits >= 0, "splits must be >= 0 (0: chosen by the library)");
  LAFS_CHECK_ARG(ldb >= D && ldq >= D && ldb % 4 == 0 && ldq % 4 == 0, "ldb and ldq must be >= D and multiples of 4");
  LAFS_CHECK_ARG(((uintptr_t)bank & 15) == 0 && ((uintptr_t)query & 15) == 0, "bank and query must be 16-byte aligned");
  const int s = knn_splits(n_query, n_bank, splits);
  const size_t need = (size_t)lafs_knn_workspace(n_query, n_bank, k, splits);
  LAFS_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace != nullptr), "workspace smaller than lafs_knn_workspace()");
  LAFS_CHECK_ARG(need == 0 || ((uintptr_t)workspace & 3) == 0, "workspace must be 4-byte aligned");
  const size_t stride = (size_t)n_query * k;
  const int64_t tiles = (n_bank + KN_TB - 1) / KN_TB;
  const int per = (int)((tiles + s - 1) / s);
  const unsigned groups = (unsigned)(((size_t)n_query + KN_TQ - 1) / KN_TQ);
  const size_t lds = (size_t)KN_LDS_FLOATS * sizeof(float);
  float* ws_s = reinterpret_cast<float*>(workspace);
  int32_t* ws_i = reinterpret_cast<int32_t*>(ws_s + (size_t)s * stride);
  size_t mlds = 0;
  if (s > 1) {
    const int nl = s + (merge ? 1 : 0);
    mlds = ((size_t)nl * k * 2 + (size_t)k * 2 + nl) * 4;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(knn_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mlds);
    if (e != hipSuccess) { lafs_set_error("lafs_knn_search: cannot reserve %zu bytes of LDS: %s", mlds, hipGetErrorString(e)); return (int)e; }
  }
  if (s == 1) {                                            // the lists are the output rows; merge: they start from what is there
    hipLaunchKernelGGL(knn_search_kernel, dim3(groups, 1), dim3(KN_THREADS), lds, stream, bank, ldb, (int)n_bank, (int)bank_pos0, query, ldq,
                       n_query, D, k, exclude, merge ? 1 : 0, per, top_score, top_idx, (size_t)0);
    LAFS_LAUNCH_CHECK();
    return LAFS_OK;
  }
  hipLaunchKernelGGL(knn_search_kernel, dim3(groups, (unsigned)s), dim3(KN_THREADS), lds, stream, bank, ldb, (int)n_bank, (int)bank_pos0, query,
                     ldq, n_query, D, k, exclude, 0, per, ws_s, ws_i, stride);
  LAFS_LAUNCH_CHECK();
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)n_query), dim3(KN_THREADS), mlds, stream, ws_s, ws_i, stride, s, merge ? 1 : 0, k,
                     top_score, top_idx);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_knn_vote(const float* top_score, const int32_t* top_idx, int n_query, int k, const int32_t* bank_label, int64_t n_label,
                             const int32_t* ks, int n_ks, float temperature, int32_t* pred, float* vote, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(top_score && top_idx && bank_label && ks && pred && vote, "bad operand");
  LAFS_CHECK_ARG(n_query > 0 && k >= 1 && k <= KN_MAX_K && n_label > 0, "n_query and n_label must be positive, k in [1, 256]");
  LAFS_CHECK_ARG(n_ks >= 1 && n_ks <= KN_MAX_KS, "n_ks must be in [1, 8]");
  LAFS_CHECK_ARG(temperature > 0.0f, "temperature must be positive");
  knn_ks a;
  a.n = n_ks;
  for (int i = 0; i < KN_MAX_KS; ++i) a.v[i] = 0;
  for (int i = 0; i < n_ks; ++i) {
    LAFS_CHECK_ARG(ks[i] >= 1 && ks[i] <= k && (i == 0 || ks[i] > ks[i - 1]), "ks must be ascending, each in [1, k]");
    a.v[i] = ks[i];
  }
  const unsigned blocks = (unsigned)(((size_t)n_query + KN_VOTE_THREADS / 64 - 1) / (KN_VOTE_THREADS / 64));
  hipLaunchKernelGGL(knn_vote_kernel, dim3(blocks), dim3(KN_VOTE_THREADS), 0, stream, top_score, top_idx, n_query, k, bank_label, n_label, a,
                     temperature, pred, vote);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}
