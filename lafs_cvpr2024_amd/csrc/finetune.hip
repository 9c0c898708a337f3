// Fine-tune step kernels (train_largescale.py): fused margin-softmax + soft-target cross-entropy over the class
// axis, batch mixup with the u8 -> [-1,1] normalisation folded in, and the landmark patch gather.
//   CosFace                         face_pre_pro/ViT_face.py:49-89   s*(cos - m*y), y one-hot OR dense soft label
//   SoftTargetCrossEntropy (timm)   train_largescale.py:602,820
//   Mixup batch mode                util/mixup_my.py:189-200, 18-24  (target has <= 2 non-zeros per row, so it is
//                                   passed as (y1, y2, lam) and the dense [B,C] matrix is never materialised)
//   CutMix, pair / elem modes, label smoothing   util/mixup_my.py:27-81, 114-187 (a parameter row per sample; the smoothed
//                                   target is dense but has closed form: a constant plus two spikes)
//   extract_patches_pytorch_gridsample   face_pre_pro/ViT_face.py:1615-1656 (n sequential grid_sample launches -> 1)
#include "common.hpp"
#include "lafs_hip.h"

namespace {

__device__ __forceinline__ float margin_logit(float c, float y, float s, float m, int type) {
  if (type == 0) return s * (c - m * y);
  if (y > 0.f) {                                      // ArcFace, hard label
    const float cc = fminf(fmaxf(c, -1.f), 1.f);
    return s * __cosf(acosf(cc) + m);
  }
  return s * c;
}
__device__ __forceinline__ float margin_dlogit(float c, float y, float s, float m, int type) {
  if (type == 0 || y <= 0.f) return s;
  const float cc = fminf(fmaxf(c, -1.f + 1e-7f), 1.f - 1e-7f);
  const float th = acosf(cc);
  return s * __sinf(th + m) / __sinf(th);
}

// The margin of a launch, behind one pair of calls: logit(c, y) = z and dlogit(c, y) = dz/dcos of a class with cosine c and target
// weight y.  FixedMargin: CosFace / ArcFace, one (m, type) for the batch -- the two functions above.  AdaMargin: AdaFace (Kim, Jain,
// Liu, CVPR 2022; PARITY UNPINNED), a pair per ROW formed by lafs_adaface_margins from the embedding's norm:
//     c^ = clamp(c, -1 + eps, 1 - eps) on every class;   target (y > 0): z = s (cos(clip(acos c^ + g_ang, eps, pi - eps)) - g_add);
//     elsewhere z = s c^;   dz/dc = s sin(theta_m) / sin(theta) on a target, s elsewhere, and exactly 0 where c was clamped or theta_m
//     clipped.
// A row's pair is the same in every lane of its workgroup (blockIdx.y indexes it): it is loaded once, into scalar registers.  The
// target's acosf / cosf / sinf are the full-precision library functions: at most two classes per row take that branch.
struct FixedMargin {
  float s, m; int type;
  __device__ __forceinline__ float logit(float c, float y) const { return margin_logit(c, y, s, m, type); }
  __device__ __forceinline__ float dlogit(float c, float y) const { return margin_dlogit(c, y, s, m, type); }
  __device__ __forceinline__ const FixedMargin& row(int) const { return *this; }
};
constexpr float ADA_EPS = 1e-3f, ADA_LO = -1.f + 1e-3f, ADA_HI = 1.f - 1e-3f, ADA_PI_HI = 3.14159265358979323846f - 1e-3f;
struct AdaMargin {
  float s, g_ang, g_add;
  __device__ __forceinline__ float logit(float c, float y) const {
    const float cc = fminf(fmaxf(c, ADA_LO), ADA_HI);
    if (y > 0.f) return s * (cosf(fminf(fmaxf(acosf(cc) + g_ang, ADA_EPS), ADA_PI_HI)) - g_add);
    return s * cc;
  }
  __device__ __forceinline__ float dlogit(float c, float y) const {
    if (c < ADA_LO || c > ADA_HI) return 0.f;
    if (y <= 0.f) return s;
    const float th = acosf(c), tm = th + g_ang;
    return (tm < ADA_EPS || tm > ADA_PI_HI) ? 0.f : s * sinf(tm) / sinf(th);
  }
};
struct AdaMargins {
  float s; const float* row_margin;                   // f32 [B, 2] = (g_ang, g_add)
  __device__ __forceinline__ AdaMargin row(int b) const { return {s, row_margin[2 * (size_t)b], row_margin[2 * (size_t)b + 1]}; }
};

// ---- the dense head's loss: margin + softmax + soft-target CE, one implementation behind three entry points ----
// Target of row b, never materialised (util/mixup_my.py:18-24 label smoothing; :152-200 batch / pair / elem modes; :71-81 CutMix's
// area-corrected lambda):
//     y_k = off + (1 - eps) (lam_b [k = a1] + (1 - lam_b) [k = a2]),   off = eps / C.
// It enters the margin itself, z_k = s (cos_k - m y_k) (ViT_face.py:69-73), and
//     loss_b = lse(z) - sum_k y_k z_k = lse(z) - off sum_k z_k - (the two spikes),      d loss / d z_k = softmax_k - y_k.
// With eps = 0 the target is exactly lam_b [k = a1] + (1 - lam_b) [k = a2] (off = 0, 1 - eps = 1; equal classes: lam + (1 - lam)).
struct MixLabel {
  int a1, a2; float w1, w2, off;
  __device__ __forceinline__ float operator()(int k) const { return off + (((k == a1) ? w1 : 0.f) + ((k == a2) ? w2 : 0.f)); }
};
// y2 == nullptr: the mixup partner of row b is row B-1-b (Mixup batch mode, util/mixup_my.py:189-200)
__device__ __forceinline__ void mce_labels(const int* y1, const int* y2, int b, int B, int& a1, int& a2) {
  a1 = y1[b];
  a2 = (y2 != nullptr) ? y2[b] : y1[B - 1 - b];
}
// lambda of row b: lam_rows[b * lam_stride] when lam_rows != nullptr (device memory, read when the kernel runs: stride 0 = one lambda for
// the batch, 1 = a plain array, LAFS_MIX_WORDS = the parameter table of lafs_mix_normalize), else lam_scalar
__device__ __forceinline__ MixLabel mix_label(const int* y1, const int* y2, const float* lam_rows, int lam_stride, float lam_scalar, float eps,
                                              int b, int B, int C) {
  MixLabel L;
  mce_labels(y1, y2, b, B, L.a1, L.a2);
  const float lam = lam_rows ? lam_rows[(size_t)b * lam_stride] : lam_scalar, on = 1.f - eps;
  L.w1 = on * lam; L.w2 = on * (1.f - lam); L.off = eps / (float)C;
  return L;
}

// online (max, sum exp) of a stream of logits: per thread, then per workgroup of 4 waves
struct OnlineLse {
  float mx = -INFINITY, sum = 0.f;
  __device__ __forceinline__ void add(float z) {
    if (z > mx) { sum = sum * __expf(mx - z) + 1.f; mx = z; } else { sum += __expf(z - mx); }
  }
  // a*b + c*d with both products rounded (no fma)
  static __device__ __forceinline__ float dot2_unfused(float a, float b, float c, float d) {
#pragma clang fp contract(off)
    return a * b + c * d;
  }
  // The pair of the union of two disjoint streams (both empty: max stays -inf, sum 0).  Which product of sa*ea + sb*eb joins the add
  // in an fma is spelled out: left to -ffp-contract the compiler picks, and not the same way in every kernel (common.hpp, ln_sq4).
  static __device__ __forceinline__ void merge(float& ma, float& sa, float mb, float sb, bool fuse) {
    const float mn = fmaxf(ma, mb), ea = __expf(ma - mn), eb = __expf(mb - mn);
    sa = (mn == -INFINITY) ? 0.f : fuse ? __builtin_fmaf(sa, ea, sb * eb) : dot2_unfused(sa, ea, sb, eb);
    ma = mn;
  }
  // 64-lane butterfly, then the 4 waves through LDS (one barrier).  The workgroup's pair is valid in thread 0 only.  The butterfly's
  // last level adds two rounded products and the levels before it fuse the own one: the arithmetic every recorded result was made with.
  __device__ __forceinline__ void block_fold() {
    __shared__ float sm[4], ss[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) merge(mx, sum, __shfl_xor(mx, o, 64), __shfl_xor(sum, o, 64), o > 1);
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = mx; ss[threadIdx.x >> 6] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
      mx = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
      sum = 0.f;
      for (int w = 0; w < 4; ++w) if (sm[w] != -INFINITY) sum += ss[w] * __expf(sm[w] - mx);
    }
  }
  __device__ __forceinline__ float lse() const { return mx + __logf(sum); }
};

// gscale * (exp(z - shift) * pscale - y) * dz/dcos: the dense head has shift = lse, pscale = 1; the class-sharded head the global
// max and 1/Z
template <class MG>
__device__ __forceinline__ float margin_grad(float c, float y, float shift, float pscale, const MG& mg, float gscale) {
  return gscale * (__expf(mg.logit(c, y) - shift) * pscale - y) * mg.dlogit(c, y);
}
__device__ __forceinline__ float margin_grad(float c, float y, float shift, float pscale, float s, float m, int type, float gscale) {
  return margin_grad(c, y, shift, pscale, FixedMargin{s, m, type}, gscale);
}
// the spikes' share of sum_k y_k z_k: (y_k - off) z_k at a1 and a2 (a1 == a2: the summed weight, once)
template <class MG>
__device__ __forceinline__ float spike_dot(const float* row, const MixLabel& label, const MG& mg) {
  const int a1 = label.a1, a2 = label.a2;
  float dot = (label(a1) - label.off) * mg.logit(row[a1], label(a1));
  if (a2 != a1) dot += (label(a2) - label.off) * mg.logit(row[a2], label(a2));
  return dot;
}
__device__ __forceinline__ float spike_dot(const float* row, const MixLabel& label, float s, float m, int type) {
  return spike_dot(row, label, FixedMargin{s, m, type});
}

// One workgroup per sample row, in place, one launch: cos -> d loss / d cos (f32).  The row loss is formed before the barrier
// because the overwrite below destroys row[a1] and row[a2].
__global__ __launch_bounds__(256) void margin_ce_kernel(float* __restrict__ cosv, int ld, int C, const int* __restrict__ y1,
                                                       const int* __restrict__ y2, float lam, float s, float m, int type,
                                                       float gscale, float* __restrict__ row_loss) {
  __shared__ float bc;
  const int b = blockIdx.x;
  float* row = cosv + (size_t)b * ld;
  const MixLabel label = mix_label(y1, y2, nullptr, 0, lam, 0.f, b, gridDim.x, C);
  OnlineLse acc;
  for (int k = threadIdx.x; k < C; k += 256) acc.add(margin_logit(row[k], label(k), s, m, type));
  acc.block_fold();
  if (threadIdx.x == 0) {
    bc = acc.lse();
    row_loss[b] = acc.lse() - spike_dot(row, label, s, m, type);   // sum_k y_k = 1
  }
  __syncthreads();
  const float lse = bc;
  for (int k = threadIdx.x; k < C; k += 256) row[k] = margin_grad(row[k], label(k), lse, 1.f, s, m, type, gscale);
}

// The same loss over (row, chunk) workgroups: one workgroup per row streams 824 KB twice at C = 205 990 and 128 rows leave half
// the chip idle (556 us, latency-bound); NCH chunks per row fill it.  Pass 1: per-chunk (max, sum exp) of the margin logits; pass 2:
// every workgroup folds its row's NCH partials, writes d loss / d cos of its chunk as bf16 (the operand format of the two
// gradient GEMMs: no fp32 round trip, no separate cast) and chunk 0 the row loss.  cos is read-only.
// SMOOTH: label smoothing is on (off > 0), so pass 1 keeps a third per-chunk partial, sum_k z_k, and the row loss takes its
// off * sum_k z_k term: part f32 [B, NCH, 3] instead of [B, NCH, 2].  Without it off is exactly 0 and the term it drops is 0 * sum z.
constexpr int MCE_NCH = 16;
struct MceChunk { int k0, k1; };
__device__ __forceinline__ MceChunk mce_chunk(int C, int ch) {
  const int per = ((C + MCE_NCH - 1) / MCE_NCH + 3) & ~3, k0 = ch * per;
  return {k0, min(C, k0 + per)};
}
// lse of a row from its NCH (max, sum exp) partials, NP floats apart
template <int NP>
__device__ __forceinline__ float mce_fold_lse(const float* prow) {
  OnlineLse r;
#pragma unroll
  for (int c = 0; c < MCE_NCH; ++c) r.mx = fmaxf(r.mx, prow[c * NP]);
#pragma unroll
  for (int c = 0; c < MCE_NCH; ++c) {
    const float mc = prow[c * NP];
    if (mc != -INFINITY) r.sum += prow[c * NP + 1] * __expf(mc - r.mx);
  }
  return r.lse();
}
// bf16 gradient of classes [k0, k1) of one row (k0 a multiple of 4); `pads`: also zero the pad columns [C, lddc) of the gradient operand
template <class MG>
__device__ __forceinline__ void mce_write_chunk(const float* row, bf16_t* drow, MceChunk ck, const MixLabel& label, float lse, const MG& mg,
                                                float gscale, bool pads, int C, int lddc) {
  const int k1 = ck.k1;
  for (int k = ck.k0 + 4 * threadIdx.x; k < k1; k += 1024) {        // 4 consecutive classes per thread: 16-byte loads, 8-byte stores
    if (k + 3 < k1) {
      const float4 c4 = *reinterpret_cast<const float4*>(row + k);
      const float cv[4] = {c4.x, c4.y, c4.z, c4.w};
      float g[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = margin_grad(cv[e], label(k + e), lse, 1.f, mg, gscale);
      *reinterpret_cast<uint2*>(drow + k) = make_uint2(pack_bf2(g[0], g[1]), pack_bf2(g[2], g[3]));
    } else {
      for (int e = 0; e < 4 && k + e < k1; ++e) drow[k + e] = f2bf(margin_grad(row[k + e], label(k + e), lse, 1.f, mg, gscale));
    }
  }
  if (pads)
    for (int k = C + threadIdx.x; k < lddc; k += 256) drow[k] = 0;
}

// MGS: the launch's margins (FixedMargin itself, or AdaMargins: the table a row's AdaMargin is taken from)
template <bool SMOOTH, class MGS>
__global__ __launch_bounds__(256) void margin_ce_part_kernel(const float* __restrict__ cosv, int ld, int B, int C, const int* __restrict__ y1,
                                                            const int* __restrict__ y2, const float* __restrict__ lam_rows, int lam_stride,
                                                            float lam, float eps, MGS margins, float* __restrict__ part) {
  constexpr int NP = SMOOTH ? 3 : 2;
  __shared__ float sz[4];
  const int b = blockIdx.y, ch = blockIdx.x;
  const float* row = cosv + (size_t)b * ld;
  const auto mg = margins.row(b);
  const MixLabel label = mix_label(y1, y2, lam_rows, lam_stride, lam, eps, b, B, C);
  const MceChunk ck = mce_chunk(C, ch);
  OnlineLse acc;
  float zs = 0.f;
  for (int k = ck.k0 + threadIdx.x; k < ck.k1; k += 256) {
    const float z = mg.logit(row[k], label(k));
    if constexpr (SMOOTH) zs += z;
    acc.add(z);
  }
  if constexpr (SMOOTH) {
    zs = wave_sum(zs);
    if ((threadIdx.x & 63) == 0) sz[threadIdx.x >> 6] = zs;
  }
  acc.block_fold();
  if (threadIdx.x == 0) {
    float* p = part + ((size_t)b * MCE_NCH + ch) * NP;
    p[0] = acc.mx; p[1] = acc.sum;
    if constexpr (SMOOTH) p[2] = (sz[0] + sz[1]) + (sz[2] + sz[3]);
  }
}
template <bool SMOOTH, class MGS>
__global__ __launch_bounds__(256) void margin_ce_grad_kernel(const float* __restrict__ cosv, int ld, int B, int C, const int* __restrict__ y1,
                                                            const int* __restrict__ y2, const float* __restrict__ lam_rows, int lam_stride,
                                                            float lam, float eps, MGS margins, float gscale,
                                                            const float* __restrict__ part, bf16_t* __restrict__ dcos, int lddc,
                                                            float* __restrict__ row_loss) {
  constexpr int NP = SMOOTH ? 3 : 2;
  const int b = blockIdx.y, ch = blockIdx.x;
  const float* row = cosv + (size_t)b * ld;
  const auto mg = margins.row(b);
  const MixLabel label = mix_label(y1, y2, lam_rows, lam_stride, lam, eps, b, B, C);
  const float* prow = part + (size_t)b * MCE_NCH * NP;
  const float lse = mce_fold_lse<NP>(prow);
  if (ch == 0 && threadIdx.x == 0) {
    float loss = lse - spike_dot(row, label, mg);   // sum_k y_k = 1
    if constexpr (SMOOTH) {
      float Zs = 0.f;
      for (int c = 0; c < MCE_NCH; ++c) Zs += prow[c * NP + 2];
      loss -= label.off * Zs;
    }
    row_loss[b] = loss;
  }
  mce_write_chunk(row, dcos + (size_t)b * lddc, mce_chunk(C, ch), label, lse, mg, gscale, ch == MCE_NCH - 1, C, lddc);
}

__global__ __launch_bounds__(256) void cast_i64_i32_kernel(const long long* __restrict__ src, int* __restrict__ dst, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = (int)src[i];
}

// patch-vector gradient [B, r*r, 192] -> image gradient [B, 3, 8r, 8r]: the inverse re-indexing of lafs_patchify
// (order 0: '(c p1 p2)' vectors of the conv patch embedding, 1: '(p1 p2 c)' of Part-fViT's Rearrange)
__global__ __launch_bounds__(256) void unpatchify_kernel(const float* __restrict__ dp, int B, int r, int order, float* __restrict__ dimg) {
  const int S = 8 * r;
  const size_t total = (size_t)B * 3 * S * S;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int x = (int)(i % S), y = (int)((i / S) % S), c = (int)((i / ((size_t)S * S)) % 3), b = (int)(i / ((size_t)3 * S * S));
    const int pi = y >> 3, pj = x >> 3, u = y & 7, v = x & 7;
    const int e = order == 1 ? (u * 8 + v) * 3 + c : c * 64 + u * 8 + v;
    dimg[i] = dp[((size_t)b * r * r + pi * r + pj) * 192 + e];
  }
}

__global__ __launch_bounds__(256) void mean_kernel(const float* __restrict__ v, int n, float scale, float* __restrict__ out) {
  __shared__ float red[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += v[i];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (red[0] + red[1] + red[2] + red[3]) * scale;
}

// u8 -> [-1,1] (x/255*2-1) and the mixup blend of a pixel with its partner's, shared by the two kernels below.  At lambda 1 the pixel
// passes through and the partner is not loaded (hence the pointer).
__device__ __forceinline__ float u8_norm(uint8_t v) { return (float)v * (2.f / 255.f) - 1.f; }
__device__ __forceinline__ float mix_blend(float x, const uint8_t* partner, float lam) {
  return (lam == 1.f) ? x : x * lam + u8_norm(*partner) * (1.f - lam);
}

__global__ __launch_bounds__(256) void mixup_norm_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int B, size_t per,
                                                        float lam, const float* __restrict__ lam_dev) {
  if (lam_dev != nullptr) lam = *lam_dev;                // a captured step reads this micro-step's lambda from device memory
  const size_t total = (size_t)B * per;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / per, r = i % per;
    dst[i] = mix_blend(u8_norm(src[i]), src + (B - 1 - b) * per + r, lam);
  }
}

// u8 -> [-1,1] with this micro-step's mixing folded in, per ROW (util/mixup_my.py:152-200: batch, pair and elem modes all mix row b
// with row B-1-b of the unmixed batch).  tab: LAFS_MIX_WORDS 32-bit words per row -- lambda (f32), CutMix flag, box yl, yh, xl, xh --
// read when the kernel runs.  A CutMix row takes its partner inside the box ([yl, yh) x [xl, xh), every channel: :163, :180-181, :196)
// and itself outside; any other row is blended as mixup_norm_kernel blends (mix_blend).
__global__ __launch_bounds__(256) void mix_norm_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int B, int S,
                                                      const int* __restrict__ tab) {
  const size_t per = (size_t)3 * S * S, total = (size_t)B * per;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t b = i / per, r = i % per;
    const int* t = tab + b * LAFS_MIX_WORDS;
    const float lam = __int_as_float(t[0]);
    const uint8_t* partner = src + (B - 1 - b) * per + r;
    const float x = u8_norm(src[i]), xf = u8_norm(*partner);
    if (t[1] != 0) {
      const int px = (int)(r % S), py = (int)((r / S) % S);
      dst[i] = (py >= t[2] && py < t[3] && px >= t[4] && px < t[5]) ? xf : x;
    } else {
      dst[i] = mix_blend(x, partner, lam);
    }
  }
}

// ---- landmark patch gather: one wave (8x8 lanes = one patch) per (image, landmark) ----
__device__ __forceinline__ float tap(const float* im, int S, int x, int y) {
  return (x >= 0 && x < S && y >= 0 && y < S) ? im[y * S + x] : 0.f;
}

__global__ __launch_bounds__(64) void gather_fwd_kernel(const float* __restrict__ img, const float* __restrict__ theta, int S, int n,
                                                       int r, float* __restrict__ out) {
  const int b = blockIdx.y, k = blockIdx.x;
  const int i = threadIdx.x >> 3, j = threadIdx.x & 7;          // output row i walks along x (transposed patch)
  const float px = theta[((size_t)b * n + k) * 2 + 0] + (float)(i - 4) - 0.5f;
  const float py = theta[((size_t)b * n + k) * 2 + 1] + (float)(j - 4) - 0.5f;
  const float fx0 = floorf(px), fy0 = floorf(py);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const float fx = px - fx0, fy = py - fy0;
  const int R = r * 8;
  const int Y = (k / r) * 8 + i, X = (k % r) * 8 + j;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* im = img + ((size_t)b * 3 + c) * S * S;
    const float v = (1.f - fy) * ((1.f - fx) * tap(im, S, x0, y0) + fx * tap(im, S, x0 + 1, y0)) +
                    fy * ((1.f - fx) * tap(im, S, x0, y0 + 1) + fx * tap(im, S, x0 + 1, y0 + 1));
    out[(((size_t)b * 3 + c) * R + Y) * R + X] = v;
  }
}

__global__ __launch_bounds__(64) void gather_bwd_kernel(const float* __restrict__ img, const float* __restrict__ theta,
                                                       const float* __restrict__ dmos, int S, int n, int r,
                                                       float* __restrict__ dtheta, float* __restrict__ dimg) {
  const int b = blockIdx.y, k = blockIdx.x;
  const int i = threadIdx.x >> 3, j = threadIdx.x & 7;
  const float px = theta[((size_t)b * n + k) * 2 + 0] + (float)(i - 4) - 0.5f;
  const float py = theta[((size_t)b * n + k) * 2 + 1] + (float)(j - 4) - 0.5f;
  const float fx0 = floorf(px), fy0 = floorf(py);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const float fx = px - fx0, fy = py - fy0;
  const int R = r * 8;
  const int Y = (k / r) * 8 + i, X = (k % r) * 8 + j;
  float gx = 0.f, gy = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* im = img + ((size_t)b * 3 + c) * S * S;
    const float d = dmos[(((size_t)b * 3 + c) * R + Y) * R + X];
    const float v00 = tap(im, S, x0, y0), v01 = tap(im, S, x0 + 1, y0), v10 = tap(im, S, x0, y0 + 1), v11 = tap(im, S, x0 + 1, y0 + 1);
    gx += d * ((1.f - fy) * (v01 - v00) + fy * (v11 - v10));
    gy += d * ((1.f - fx) * (v10 - v00) + fx * (v11 - v01));
    if (dimg != nullptr) {
      float* di = dimg + ((size_t)b * 3 + c) * S * S;
      auto add = [&](int x, int y, float w) { if (x >= 0 && x < S && y >= 0 && y < S) atomicAdd(di + y * S + x, d * w); };
      add(x0, y0, (1.f - fx) * (1.f - fy)); add(x0 + 1, y0, fx * (1.f - fy));
      add(x0, y0 + 1, (1.f - fx) * fy); add(x0 + 1, y0 + 1, fx * fy);
    }
  }
  gx = wave_sum(gx); gy = wave_sum(gy);
  if (threadIdx.x == 0) {
    dtheta[((size_t)b * n + k) * 2 + 0] = gx;
    dtheta[((size_t)b * n + k) * 2 + 1] = gy;
  }
}

// ---- class-sharded margin softmax (PartialFC): three row passes with the cross-rank statistics exchanged in between ----
// y[b] = local index of the row's target class inside this shard, or -1 when another rank owns it.  Soft (mixup) targets as the
// reference feeds them to its margin head (dense lam e_y1 + (1 - lam) e_y2 entering the margin itself, ViT_face.py:69-73): y2[b] =
// local index of the partner's class (or -1), lam[b] = the row's lambda; y2 == nullptr: hard labels.
struct ShardLabel {
  int t1, t2; float w1, w2;
  __device__ __forceinline__ float operator()(int k) const { return (k == t1 ? w1 : 0.f) + (k == t2 ? w2 : 0.f); }
};
__device__ __forceinline__ ShardLabel shard_label(const int* y, const int* y2, const float* lam, int b) {
  ShardLabel L;
  L.t1 = y[b]; L.t2 = -1; L.w1 = 1.f; L.w2 = 0.f;
  if (y2 != nullptr) {
    const float l = lam != nullptr ? lam[b] : 1.f;
    L.w1 = l; L.w2 = 1.f - l; L.t2 = y2[b];
    if (L.t2 == L.t1) { L.w1 = (L.t1 >= 0) ? 1.f : 0.f; L.t2 = -1; L.w2 = 0.f; }      // both labels on the same class
  }
  return L;
}
__global__ __launch_bounds__(256) void shard_rowmax_kernel(const float* __restrict__ cosv, int ld, int S, const int* __restrict__ y,
                                                          const int* __restrict__ y2, const float* __restrict__ lam,
                                                          float s, float m, int type, float* __restrict__ rowmax) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const float* row = cosv + (size_t)b * ld;
  const ShardLabel L = shard_label(y, y2, lam, b);
  float mx = -INFINITY;
  for (int k = threadIdx.x; k < S; k += 256) mx = fmaxf(mx, margin_logit(row[k], L(k), s, m, type));
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) rowmax[b] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// rowsum[b] = sum_k exp(z_k - gmax[b]);  tgt[b] = sum_k y_k z_k over the targets this rank owns (0 when they live elsewhere)
__global__ __launch_bounds__(256) void shard_rowsum_kernel(const float* __restrict__ cosv, int ld, int S, const int* __restrict__ y,
                                                          const int* __restrict__ y2, const float* __restrict__ lam,
                                                          float s, float m, int type, const float* __restrict__ gmax,
                                                          float* __restrict__ rowsum, float* __restrict__ tgt) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const float* row = cosv + (size_t)b * ld;
  const ShardLabel L = shard_label(y, y2, lam, b);
  const float g = gmax[b];
  float acc = 0.f;
  for (int k = threadIdx.x; k < S; k += 256) acc += __expf(margin_logit(row[k], L(k), s, m, type) - g);
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    rowsum[b] = red[0] + red[1] + red[2] + red[3];
    float t = 0.f;
    if (L.t1 >= 0) t += L.w1 * margin_logit(row[L.t1], L(L.t1), s, m, type);
    if (L.t2 >= 0) t += L.w2 * margin_logit(row[L.t2], L(L.t2), s, m, type);
    tgt[b] = t;
  }
}

// in place: cos -> dL/dcos = gscale * (exp(z - gmax)/Z - y) * dz/dcos
__global__ __launch_bounds__(256) void shard_grad_kernel(float* __restrict__ cosv, int ld, int S, const int* __restrict__ y,
                                                        const int* __restrict__ y2, const float* __restrict__ lam, float s,
                                                        float m, int type, const float* __restrict__ gmax,
                                                        const float* __restrict__ Z, float gscale) {
  const int b = blockIdx.x;
  float* row = cosv + (size_t)b * ld;
  const ShardLabel L = shard_label(y, y2, lam, b);
  const float g = gmax[b], iz = 1.0f / Z[b];
  for (int k = threadIdx.x; k < S; k += 256) row[k] = margin_grad(row[k], L(k), g, iz, s, m, type, gscale);
}

// ---- landmark post-processing: raw regressor output -> pixel landmarks (face_pre_pro/ViT_face.py:1347-1378) ----
// one workgroup per image: per-sample min-max to [0,111], + noise_scale * noise, optional selection (with replacement)
__global__ __launch_bounds__(256) void landmark_theta_kernel(const float* __restrict__ t, int n_full, const float* __restrict__ noise,
                                                             float noise_scale, const int* __restrict__ sel, int n_out,
                                                             float* __restrict__ theta) {
  __shared__ float rmin[4], rmax[4];
  const int b = blockIdx.x, L = 2 * n_full;
  const float* row = t + (size_t)b * L;
  float mn = INFINITY, mx = -INFINITY;
  for (int k = threadIdx.x; k < L; k += 256) { const float v = row[k]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
  mx = wave_max(mx); mn = -wave_max(-mn);
  if ((threadIdx.x & 63) == 0) { rmin[threadIdx.x >> 6] = mn; rmax[threadIdx.x >> 6] = mx; }
  __syncthreads();
  mn = fminf(fminf(rmin[0], rmin[1]), fminf(rmin[2], rmin[3]));
  mx = fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3]));
  const float range = mx - mn;
  for (int k = threadIdx.x; k < 2 * n_out; k += 256) {
    const int lm = sel ? sel[(size_t)b * n_out + (k >> 1)] : (k >> 1);
    const int src = 2 * lm + (k & 1);
    float v = (row[src] - mn) / range * 111.0f;
    if (noise) v += noise_scale * noise[(size_t)b * L + src];
    theta[(size_t)b * 2 * n_out + k] = v;
  }
}

// ---- landmark supervision of the fine-tune step (train_largescale.py:825-843): MSE of the backbone's landmarks against the frozen
// stage-1 CNN's, both / 111, its weighted share of the loss and its gradient into theta.  At most 128 x 196 pairs: ONE workgroup, one
// (x, y) pair per thread and round.  Fixed order, no atomics: a thread adds its pairs' squares in index order (x, then y, one fma
// each), a 64-lane butterfly follows, thread 0 adds the 16 wave sums in wave order.  The gradient does not need the sum, so it is
// added in the same pass.  weight == 0 adds exact zeros: fma(0, d, g) == g.
#define LMSE_THREADS 1024
__global__ __launch_bounds__(LMSE_THREADS) void landmark_mse_kernel(const float2* __restrict__ pred, const float2* __restrict__ label,
                                                                    long long n_pairs, const float* __restrict__ weight, float grad_scale,
                                                                    float inv, float* __restrict__ loss_land, float* __restrict__ loss,
                                                                    float2* __restrict__ dtheta) {
  __shared__ float part[LMSE_THREADS / LAFS_WAVE];
  const float w = weight[0] * grad_scale;                // this epoch's land_loss_control, read when the kernel runs
  const float coef = w * (2.f * inv);                    // d/dpred of w * mean((pred - label)^2 / 111^2)
  float sq = 0.f;
  for (long long i = threadIdx.x; i < n_pairs; i += LMSE_THREADS) {
    const float2 p = pred[i], l = label[i];
    const float dx = p.x - l.x, dy = p.y - l.y;
    sq = __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, sq));
    if (dtheta != nullptr) {
      float2 g = dtheta[i];
      g.x = __builtin_fmaf(coef, dx, g.x);
      g.y = __builtin_fmaf(coef, dy, g.y);
      dtheta[i] = g;
    }
  }
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < LMSE_THREADS / LAFS_WAVE; ++k) s += part[k];
    const float mean = s * inv;
    loss_land[0] = mean;
    if (loss != nullptr) loss[0] = __builtin_fmaf(w, mean, loss[0]);
  }
}

// ---- AdaFace: the batch's norm statistics, the running state and every row's margin pair, ONE workgroup ----
// n_b = clip(1 / inv_norm[b], 1e-3, 100);  mean = sum n_b / B;  std = sqrt(sum (n_b - mean)^2 / (B - 1)), two passes (a sum of squares
// cancels at norms near 20 +- 0.2);  update: state <- t (mean, std) + (1 - t) state, FIRST;  k_b = clip((n_b - batch_mean) /
// (batch_std + 1e-3) h, -1, 1);  row_margin[b] = (-m k_b, m + m k_b).  Fixed order, no atomics: a thread adds its rows in index order,
// a 64-lane butterfly follows, every thread adds the four wave sums as (0 + 1) + (2 + 3).  The state lives in device memory and is
// read and written when the kernel runs: a replayed graph moves it once per replay.
__device__ __forceinline__ float ada_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                                     // (red may still be read from the sum before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float ada_norm(float inv) { return fminf(fmaxf(1.f / inv, 1e-3f), 100.f); }
__global__ __launch_bounds__(256) void adaface_margins_kernel(const float* __restrict__ inv_norm, int B, float* __restrict__ state, float t_alpha,
                                                             float h, float m, int update, float* __restrict__ row_margin) {
  __shared__ float red[4], st[2];
  float a = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) a += ada_norm(inv_norm[i]);
  const float mean = ada_block_sum(a, red) / (float)B;
  float q = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) { const float d = ada_norm(inv_norm[i]) - mean; q = __builtin_fmaf(d, d, q); }
  const float sd = sqrtf(ada_block_sum(q, red) / (float)(B - 1));
  if (threadIdx.x == 0) {
    float bm = state[0], bs = state[1];
    if (update) {
      bm = __builtin_fmaf(t_alpha, mean, (1.f - t_alpha) * bm);
      bs = __builtin_fmaf(t_alpha, sd, (1.f - t_alpha) * bs);
      state[0] = bm; state[1] = bs;
    }
    st[0] = bm; st[1] = bs;
  }
  __syncthreads();
  const float bm = st[0], den = st[1] + 1e-3f;
  for (int i = threadIdx.x; i < B; i += 256) {
    const float k = fminf(fmaxf((ada_norm(inv_norm[i]) - bm) / den * h, -1.f), 1.f), mk = m * k;
    *reinterpret_cast<float2*>(row_margin + 2 * (size_t)i) = make_float2(-mk, m + mk);
  }
}

// the chunked form's three launches: partials, gradient + row losses, mean loss
template <bool SMOOTH, class MGS>
int launch_margin_ce(const float* cos, int ld, int B, int C, const int32_t* y1, const int32_t* y2, const float* lam_rows, int lam_stride, float lam,
                     float eps, MGS margins, float loss_scale, void* dcos, int lddc, float* loss_out, float* row_ws, float* part_ws,
                     hipStream_t stream) {
  hipLaunchKernelGGL((margin_ce_part_kernel<SMOOTH, MGS>), dim3(MCE_NCH, B), dim3(256), 0, stream, cos, ld, B, C, y1, y2, lam_rows, lam_stride,
                     lam, eps, margins, part_ws);
  LAFS_LAUNCH_CHECK();
  hipLaunchKernelGGL((margin_ce_grad_kernel<SMOOTH, MGS>), dim3(MCE_NCH, B), dim3(256), 0, stream, cos, ld, B, C, y1, y2, lam_rows, lam_stride,
                     lam, eps, margins, loss_scale / (float)B, part_ws, (bf16_t*)dcos, lddc, row_ws);
  LAFS_LAUNCH_CHECK();
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, stream, row_ws, B, 1.0f / (float)B, loss_out);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

int isqrt_exact(int n) {
  int r = 0;
  while ((r + 1) * (r + 1) <= n) ++r;
  return (r * r == n) ? r : -1;
}

}  // namespace

extern "C" int lafs_margin_softmax_ce(float* cos, int ld, int B, int C, const int32_t* y1, const int32_t* y2, float lam,
                                      float s, float m, int margin_type, float loss_scale, float* loss_out, float* row_ws,
                                      hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(cos && y1 && y2 && loss_out && row_ws && B > 0 && C > 0 && ld >= C, "bad operand");
  LAFS_CHECK_ARG(margin_type == 0 || margin_type == 1, "margin_type must be 0 (CosFace) or 1 (ArcFace)");
  hipLaunchKernelGGL(margin_ce_kernel, dim3(B), dim3(256), 0, stream, cos, ld, C, y1, y2, lam, s, m, margin_type, loss_scale / (float)B,
                     row_ws);
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, stream, row_ws, B, 1.0f / (float)B, loss_out);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_margin_softmax_ce_bf16(const float* cos, int ld, int B, int C, const int32_t* y1, const int32_t* y2, float lam,
                                           const float* lam_dev, float s, float m, int margin_type, float loss_scale, void* dcos, int lddc,
                                           float* loss_out, float* row_ws, float* part_ws, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(cos && y1 && dcos && loss_out && row_ws && part_ws && B > 0 && C > 0 && ld >= C && lddc >= C, "bad operand");
  LAFS_CHECK_ARG(ld % 4 == 0 && lddc % 4 == 0, "row strides must be multiples of 4 elements");
  LAFS_CHECK_ARG(margin_type == 0 || margin_type == 1, "margin_type must be 0 (CosFace) or 1 (ArcFace)");
  return launch_margin_ce<false>(cos, ld, B, C, y1, y2, lam_dev, 0, lam, 0.f, FixedMargin{s, m, margin_type}, loss_scale, dcos, lddc, loss_out,
                                 row_ws, part_ws, stream);
}

extern "C" int lafs_margin_softmax_ce_mix_bf16(const float* cos, int ld, int B, int C, const int32_t* y1, const int32_t* y2,
                                               const float* lam_rows, int lam_stride, float eps, float s, float m, int margin_type,
                                               float loss_scale, void* dcos, int lddc, float* loss_out, float* row_ws, float* part_ws,
                                               hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(cos && y1 && lam_rows && dcos && loss_out && row_ws && part_ws && B > 0 && C > 0 && ld >= C && lddc >= C, "bad operand");
  LAFS_CHECK_ARG(ld % 4 == 0 && lddc % 4 == 0, "row strides must be multiples of 4 elements");
  LAFS_CHECK_ARG(lam_stride >= 1, "lam_stride counts 32-bit words between two rows' lambdas (>= 1)");
  LAFS_CHECK_ARG(margin_type == 0 || margin_type == 1, "margin_type must be 0 (CosFace) or 1 (ArcFace)");
  LAFS_CHECK_ARG(eps >= 0.f && eps < 1.f, "label smoothing must lie in [0, 1)");
  LAFS_CHECK_ARG(eps == 0.f || margin_type == 0, "label smoothing needs the CosFace margin (ArcFace has no margin for a dense target)");
  const auto launch = eps > 0.f ? launch_margin_ce<true, FixedMargin> : launch_margin_ce<false, FixedMargin>;        // eps == 0: off = 0, nothing to smooth
  return launch(cos, ld, B, C, y1, y2, lam_rows, lam_stride, 0.f, eps, FixedMargin{s, m, margin_type}, loss_scale, dcos, lddc, loss_out, row_ws,
                part_ws, stream);
}

extern "C" int lafs_adaface_margins(const float* inv_norm, int B, float* state, float t_alpha, float h, float m, int update, float* row_margin,
                                    hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(inv_norm && state && row_margin, "bad operand");
  LAFS_CHECK_ARG((uintptr_t)row_margin % 8 == 0, "row_margin pairs must be 8-byte aligned");
  LAFS_CHECK_ARG(B >= 2, "the unbiased standard deviation of the batch's norms needs at least two rows");
  LAFS_CHECK_ARG(t_alpha >= 0.f && t_alpha <= 1.f, "t_alpha must lie in [0, 1]");
  LAFS_CHECK_ARG(update == 0 || update == 1, "update must be 0 (read the state) or 1 (update it first)");
  hipLaunchKernelGGL(adaface_margins_kernel, dim3(1), dim3(256), 0, stream, inv_norm, B, state, t_alpha, h, m, update, row_margin);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_margin_softmax_ce_ada_bf16(const float* cos, int ld, int B, int C, const int32_t* y1, const int32_t* y2,
                                               const float* lam_rows, int lam_stride, const float* row_margin, float s, float loss_scale,
                                               void* dcos, int lddc, float* loss_out, float* row_ws, float* part_ws, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(cos && y1 && lam_rows && row_margin && dcos && loss_out && row_ws && part_ws && B > 0 && C > 0 && ld >= C && lddc >= C,
                 "bad operand");
  LAFS_CHECK_ARG(ld % 4 == 0 && lddc % 4 == 0, "row strides must be multiples of 4 elements");
  LAFS_CHECK_ARG(lam_stride >= 0, "lam_stride counts 32-bit words between two rows' lambdas (0: one lambda for the batch)");
  return launch_margin_ce<false>(cos, ld, B, C, y1, y2, lam_rows, lam_stride, 0.f, 0.f, AdaMargins{s, row_margin}, loss_scale, dcos, lddc, loss_out,
                                 row_ws, part_ws, stream);
}

extern "C" int lafs_cast_i64_i32(const int64_t* src, int32_t* dst, int n, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(src && dst && n > 0, "bad operand");
  hipLaunchKernelGGL(cast_i64_i32_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const long long*)src, dst, n);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_unpatchify_f32(const float* dpatch, int B, int S, int order, float* dimg, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(dpatch && dimg && B > 0 && S > 0 && S % 8 == 0 && (order == 0 || order == 1), "bad operand");
  size_t blocks = ((size_t)B * 3 * S * S + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(unpatchify_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, dpatch, B, S / 8, order, dimg);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_mixup_normalize(const uint8_t* src_u8, float* dst, int B, int S, float lam, const float* lam_dev, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(src_u8 && dst && B > 0 && S > 0, "bad operand");
  const size_t per = (size_t)3 * S * S;
  size_t blocks = ((size_t)B * per + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(mixup_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src_u8, dst, B, per, lam, lam_dev);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_mix_normalize(const uint8_t* src_u8, float* dst, int B, int S, const int32_t* table, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(src_u8 && dst && table && B > 0 && S > 0, "bad operand");
  size_t blocks = ((size_t)B * 3 * S * S + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(mix_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src_u8, dst, B, S, table);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_patch_gather_fwd(const float* img, const float* theta, int B, int S, int n, float* mosaic, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  const int r = isqrt_exact(n);
  LAFS_CHECK_ARG(img && theta && mosaic && B > 0 && S > 0 && r > 0, "n must be a perfect square");
  hipLaunchKernelGGL(gather_fwd_kernel, dim3(n, B), dim3(64), 0, stream, img, theta, S, n, r, mosaic);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_patch_gather_bwd(const float* img, const float* theta, const float* dmosaic, int B, int S, int n,
                                     float* dtheta, float* dimg, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  const int r = isqrt_exact(n);
  LAFS_CHECK_ARG(img && theta && dmosaic && dtheta && B > 0 && S > 0 && r > 0, "n must be a perfect square");
  hipLaunchKernelGGL(gather_bwd_kernel, dim3(n, B), dim3(64), 0, stream, img, theta, dmosaic, S, n, r, dtheta, dimg);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_landmark_mse(const float* pred, const float* label, int B, int n, const float* weight, float grad_scale,
                                 float* loss_land, float* loss, float* dtheta, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(pred && label && weight && loss_land, "bad operand");
  LAFS_CHECK_ARG(B > 0 && n > 0, "B and n must be positive");
  LAFS_CHECK_ARG(grad_scale > 0.f, "grad_scale is 1 / acc_step: positive");
  LAFS_CHECK_ARG(((uintptr_t)pred | (uintptr_t)label | (uintptr_t)dtheta) % 8 == 0, "landmark pairs must be 8-byte aligned");
  const long long n_pairs = (long long)B * n;
  const float inv = (float)(1.0 / (111.0 * 111.0 * 2.0 * (double)n_pairs));
  hipLaunchKernelGGL(landmark_mse_kernel, dim3(1), dim3(LMSE_THREADS), 0, stream, (const float2*)pred, (const float2*)label, n_pairs, weight,
                     grad_scale, inv, loss_land, loss, (float2*)dtheta);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_shard_margin_rowmax(const float* cos, int ld, int B, int S, const int32_t* y_local, const int32_t* y2_local,
                                        const float* lam, float s, float m, int margin_type, float* rowmax, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(cos && y_local && rowmax && B > 0 && S > 0 && ld >= S, "bad operand");
  LAFS_CHECK_ARG(margin_type == 0 || margin_type == 1, "margin_type must be 0 (CosFace) or 1 (ArcFace)");
  LAFS_CHECK_ARG(y2_local == nullptr || margin_type == 0, "soft (mixup) targets: CosFace margin only (ArcFace takes hard labels)");
  hipLaunchKernelGGL(shard_rowmax_kernel, dim3(B), dim3(256), 0, stream, cos, ld, S, y_local, y2_local, lam, s, m, margin_type, rowmax);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_shard_margin_rowsum(const float* cos, int ld, int B, int S, const int32_t* y_local, const int32_t* y2_local,
                                        const float* lam, float s, float m, int margin_type, const float* gmax, float* rowsum,
                                        float* target_logit, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(cos && y_local && gmax && rowsum && target_logit && B > 0 && S > 0 && ld >= S, "bad operand");
  LAFS_CHECK_ARG(margin_type == 0 || margin_type == 1, "margin_type must be 0 (CosFace) or 1 (ArcFace)");
  LAFS_CHECK_ARG(y2_local == nullptr || margin_type == 0, "soft (mixup) targets: CosFace margin only (ArcFace takes hard labels)");
  hipLaunchKernelGGL(shard_rowsum_kernel, dim3(B), dim3(256), 0, stream, cos, ld, S, y_local, y2_local, lam, s, m, margin_type, gmax,
                     rowsum, target_logit);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_shard_margin_grad(float* cos, int ld, int B, int S, const int32_t* y_local, const int32_t* y2_local,
                                      const float* lam, float s, float m, int margin_type, const float* gmax, const float* Z,
                                      float grad_scale, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(cos && y_local && gmax && Z && B > 0 && S > 0 && ld >= S, "bad operand");
  LAFS_CHECK_ARG(margin_type == 0 || margin_type == 1, "margin_type must be 0 (CosFace) or 1 (ArcFace)");
  LAFS_CHECK_ARG(y2_local == nullptr || margin_type == 0, "soft (mixup) targets: CosFace margin only (ArcFace takes hard labels)");
  hipLaunchKernelGGL(shard_grad_kernel, dim3(B), dim3(256), 0, stream, cos, ld, S, y_local, y2_local, lam, s, m, margin_type, gmax, Z,
                     grad_scale);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}

extern "C" int lafs_landmark_theta(const float* t, int B, int n_full, const float* noise, float noise_scale, const int32_t* sel,
                                   int n_out, float* theta, hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(t && theta && B > 0 && n_full > 0 && n_out > 0, "bad operand");
  LAFS_CHECK_ARG(sel != nullptr || n_out <= n_full, "n_out > n_full needs a selection");
  hipLaunchKernelGGL(landmark_theta_kernel, dim3(B), dim3(256), 0, stream, t, n_full, noise, noise_scale, sel, n_out, theta);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}
