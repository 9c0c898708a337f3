// Softmax cross-entropy, rank of the target and bf16 gradient of plain logits: the loss of the linear probe on frozen features
// (lafs_cvpr2024_amd/linear_probe.py; DINO's eval_linear.py protocol, no counterpart in the reference).  Three launches, or two
// without a gradient, in the (row, chunk) shape of lafs_margin_softmax_ce_bf16:
//   lp_part_kernel      (row, chunk of LP_CHUNK columns) -> the chunk's (max, sum exp(z - max)) and how many of its columns rank
//                       before the target
//   lp_finalise_kernel  one wave per row folds the row's partials in chunk order -> lse, row_loss, row_rank
//   lp_grad_kernel      (row, chunk) -> bf16(grad_scale (exp(z - lse) - [k = y])), the last chunk also the zero pad columns
// Bytes per call (B rows, C classes; the partials, 12 B per (row, chunk) written and read once, left out):
//   without dlogits   4 B C            one read of the logits
//   with dlogits      8 B C + 2 B lddl the logits are read by both (row, chunk) kernels -- the gradient needs the row's lse, which
//                     needs the whole row first, and a row of 2 .. 300 000 floats has no place on chip to wait -- and written once as
//                     bf16.  Only a logits table that stays in the 256 MiB last-level cache makes the second read cheaper than HBM.
// Every sum has a fixed order (lane, 64-lane butterfly, waves 0..3, chunks in index order) and nothing is an atomic: two calls on
// equal inputs give equal bits.  The order does depend on the alignment of a row's start (scalar head below).
#include "common.hpp"
#include "lafs_hip.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_VEC = 4;                                   // float4 loads per thread
constexpr int LP_CHUNK = LP_THREADS * LP_VEC * 4;           // 4096 columns per workgroup

__device__ __forceinline__ float lp_qnan() { return __int_as_float(0x7fc00000); }

// Columns [k0, k0 + n) of one row as a scalar head (up to the first 16-byte boundary), nvec float4 and a scalar tail of < 4.
// n <= LP_CHUNK, so nvec <= LP_THREADS * LP_VEC: thread t owns head element t, vectors t + 256 i (i < LP_VEC) and tail element t.
struct LpSpan { int k0, n, head, nvec, tail0; };
__device__ __forceinline__ LpSpan lp_span(const float* row, int C, int ch) {
  LpSpan s;
  s.k0 = ch * LP_CHUNK;
  s.n = min(C - s.k0, LP_CHUNK);
  const int mis = (int)(((uintptr_t)(row + s.k0) >> 2) & 3);
  s.head = min(s.n, (4 - mis) & 3);
  s.nvec = (s.n - s.head) >> 2;
  s.tail0 = s.head + 4 * s.nvec;
  return s;
}

// What a thread holds of its chunk: all loads are issued before the first use
struct LpRegs { float4 v[LP_VEC]; float h, t; };
__device__ __forceinline__ LpRegs lp_load(const float* p, const LpSpan& s) {
  LpRegs r;
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < LP_VEC; ++i) {
    const int vi = t + LP_THREADS * i;
    r.v[i] = (vi < s.nvec) ? *reinterpret_cast<const float4*>(p + s.head + 4 * vi) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  r.h = (t < s.head) ? p[t] : 0.f;
  r.t = (s.tail0 + t < s.n) ? p[s.tail0 + t] : 0.f;
  return r;
}

// f(z, k) on every column the thread holds, in the order head, vectors, tail
template <class F>
__device__ __forceinline__ void lp_each(const LpRegs& r, const LpSpan& s, F f) {
  const int t = threadIdx.x;
  if (t < s.head) f(r.h, s.k0 + t);
#pragma unroll
  for (int i = 0; i < LP_VEC; ++i) {
    const int vi = t + LP_THREADS * i;
    if (vi < s.nvec) {
      const int k = s.k0 + s.head + 4 * vi;
      f(r.v[i].x, k); f(r.v[i].y, k + 1); f(r.v[i].z, k + 2); f(r.v[i].w, k + 3);
    }
  }
  if (s.tail0 + t < s.n) f(r.t, s.k0 + s.tail0 + t);
}
// sum rescaled from its own maximum to the common one (an empty stream: 0, never exp(-inf + inf))
__device__ __forceinline__ float lp_rescale(float sum, float mx, float common) { return (mx == -INFINITY) ? 0.f : sum * __expf(mx - common); }
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// columns that rank before the target: a larger logit, or an equal one at a smaller index
__device__ __forceinline__ int lp_before(float z, int k, float zy, int y) { return (z > zy || (z == zy && k < y)) ? 1 : 0; }

__global__ __launch_bounds__(LP_THREADS) void lp_part_kernel(const float* __restrict__ logits, int ld, int C, const int* __restrict__ y, int nch,
                                                            float* __restrict__ part, int* __restrict__ cnt) {
  __shared__ float sm[4], ss[4];
  __shared__ int sc[4];
  const int b = blockIdx.y, ch = blockIdx.x, t = threadIdx.x;
  const float* row = logits + (size_t)b * ld;
  const int yb = y[b];
  const bool has = yb >= 0 && yb < C;
  const float zy = has ? row[yb] : INFINITY;                 // (no target: nothing ranks before +inf at index -1; never read)
  const int yk = has ? yb : -1;
  const LpSpan s = lp_span(row, C, ch);
  const LpRegs r = lp_load(row + s.k0, s);
  float mx = -INFINITY, sum = 0.f;                        // the thread's columns: the maximum first, then sum exp(z - max)
  int before = 0;
  lp_each(r, s, [&](float z, int) { mx = fmaxf(mx, z); });
  lp_each(r, s, [&](float z, int k) {
    if (mx != -INFINITY) sum += __expf(z - mx);
    before += lp_before(z, k, zy, yk);
  });
  const float wmx = wave_max(mx);
  const float wsum = wave_sum(lp_rescale(sum, mx, wmx));
  before = wave_sum_i(before);
  if ((t & 63) == 0) { sm[t >> 6] = wmx; ss[t >> 6] = wsum; sc[t >> 6] = before; }
  __syncthreads();
  if (t == 0) {
    const float bmx = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    float bsum = 0.f;
    for (int w = 0; w < 4; ++w) bsum += lp_rescale(ss[w], sm[w], bmx);
    float* p = part + ((size_t)b * nch + ch) * 2;
    p[0] = bmx; p[1] = bsum;
    cnt[(size_t)b * nch + ch] = has ? (sc[0] + sc[1]) + (sc[2] + sc[3]) : 0;
  }
}

// One wave per row: lane l folds partials l, l + 64, ... in order, then the butterfly.
__global__ __launch_bounds__(64) void lp_finalise_kernel(const float* __restrict__ logits, int ld, int C, const int* __restrict__ y, int nch,
                                                        const float* __restrict__ part, const int* __restrict__ cnt,
                                                        float* __restrict__ row_lse, float* __restrict__ row_loss, int* __restrict__ row_rank) {
  const int b = blockIdx.x, l = threadIdx.x;
  const float* prow = part + (size_t)b * nch * 2;
  const int* crow = cnt + (size_t)b * nch;
  float mx = -INFINITY;
  for (int c = l; c < nch; c += 64) mx = fmaxf(mx, prow[2 * c]);
  const float rmx = wave_max(mx);
  float sum = 0.f;
  int before = 0;
  for (int c = l; c < nch; c += 64) { sum += lp_rescale(prow[2 * c + 1], prow[2 * c], rmx); before += crow[c]; }
  const float rsum = wave_sum(sum);
  before = wave_sum_i(before);
  if (l == 0) {
    const float lse = rmx + __logf(rsum);
    const int yb = y[b];
    row_lse[b] = lse;
    if (yb >= 0 && yb < C) { row_loss[b] = lse - logits[(size_t)b * ld + yb]; row_rank[b] = before; }
    else if (yb == -1) { row_loss[b] = 0.f; row_rank[b] = -1; }
    else { row_loss[b] = lp_qnan(); row_rank[b] = -2; }
  }
}

__global__ __launch_bounds__(LP_THREADS) void lp_grad_kernel(const float* __restrict__ logits, int ld, int C, const int* __restrict__ y, int nch,
                                                            const float* __restrict__ row_lse, float gscale, bf16_t* __restrict__ dl, int lddl) {
  const int b = blockIdx.y, ch = blockIdx.x, t = threadIdx.x;
  const float* row = logits + (size_t)b * ld;
  bf16_t* drow = dl + (size_t)b * lddl;
  const int yb = y[b];
  const LpSpan s = lp_span(row, C, ch);
  if (ch == nch - 1)
    for (int k = C + t; k < lddl; k += LP_THREADS) drow[k] = 0;
  if (yb < 0 || yb >= C) {                                    // no target, or a label that is none: a zero gradient row
    for (int k = s.k0 + t; k < s.k0 + s.n; k += LP_THREADS) drow[k] = 0;
    return;
  }
  const LpRegs r = lp_load(row + s.k0, s);
  const float lse = row_lse[b];
  auto grad = [&](float z, int k) { return gscale * (__expf(z - lse) - ((k == yb) ? 1.f : 0.f)); };
  if (t < s.head) drow[s.k0 + t] = f2bf(grad(r.h, s.k0 + t));
#pragma unroll
  for (int i = 0; i < LP_VEC; ++i) {
    const int vi = t + LP_THREADS * i;
    if (vi < s.nvec) {
      const int k = s.k0 + s.head + 4 * vi;
      const float g0 = grad(r.v[i].x, k), g1 = grad(r.v[i].y, k + 1), g2 = grad(r.v[i].z, k + 2), g3 = grad(r.v[i].w, k + 3);
      // head == 0: k is a multiple of 4 and the gradient row starts on 16 bytes (lddl % 8 == 0), so the 8-byte store is aligned
      if (s.head == 0) {
        *reinterpret_cast<uint2*>(drow + k) = make_uint2(pack_bf2(g0, g1), pack_bf2(g2, g3));
      } else {
        drow[k] = f2bf(g0); drow[k + 1] = f2bf(g1); drow[k + 2] = f2bf(g2); drow[k + 3] = f2bf(g3);
      }
    }
  }
  if (s.tail0 + t < s.n) drow[s.k0 + s.tail0 + t] = f2bf(grad(r.t, s.k0 + s.tail0 + t));
}

int lp_chunks(int C) { return ceil_div(C, LP_CHUNK); }

}  // namespace

extern "C" int64_t lafs_softmax_ce_rank_workspace_bytes(int B, int C) {
  if (B <= 0 || C <= 0) return -1;
  return (int64_t)B * (3 * (int64_t)lp_chunks(C) + 1) * 4;
}

extern "C" int lafs_softmax_ce_rank(const float* logits, int ld, int B, int C, const int32_t* y, float grad_scale, void* dlogits_bf16, int lddl,
                                    float* row_loss, int32_t* row_rank, float* ws, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(logits && y && row_loss && row_rank && ws, "null operand");
  LAFS_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && ld >= C, "bad shape (1 <= B <= 65535, 1 <= C <= ld)");
  LAFS_CHECK_ARG(((uintptr_t)logits & 3) == 0, "logits must be 4-byte aligned");
  LAFS_CHECK_ARG(dlogits_bf16 == nullptr || (lddl >= C && lddl % 8 == 0 && ((uintptr_t)dlogits_bf16 & 15) == 0),
                 "dlogits: lddl >= C, lddl % 8 == 0, 16-byte aligned");
  const int nch = lp_chunks(C);
  // workspace: part f32 [B, nch, 2] | cnt i32 [B, nch] | lse f32 [B]
  float* part = ws;
  int* cnt = reinterpret_cast<int*>(ws + (size_t)B * nch * 2);
  float* lse = ws + (size_t)B * nch * 3;
  const dim3 grid(nch, B);
  hipLaunchKernelGGL(lp_part_kernel, grid, dim3(LP_THREADS), 0, stream, logits, ld, C, y, nch, part, cnt);
  LAFS_LAUNCH_CHECK();
  hipLaunchKernelGGL(lp_finalise_kernel, dim3(B), dim3(64), 0, stream, logits, ld, C, y, nch, (const float*)part, (const int*)cnt, lse,
                     row_loss, row_rank);
  LAFS_LAUNCH_CHECK();
  if (dlogits_bf16 != nullptr) {
    hipLaunchKernelGGL(lp_grad_kernel, grid, dim3(LP_THREADS), 0, stream, logits, ld, C, y, nch, (const float*)lse, grad_scale,
                       (bf16_t*)dlogits_bf16, lddl);
    LAFS_LAUNCH_CHECK();
  }
  return LAFS_OK;
}
