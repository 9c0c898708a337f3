// FaceDataset's torchvision tensor chain on the device (reference image_iter.py:214-219, applied at :349-351):
//   Compose([RandomResizedCrop(112, scale=(0.9, 1.0)), ColorJitter(0.1, 0.1, 0.1, 0.1), RandomErasing(scale=(0.02, 0.1))])
// on the uint8 CHW tensor RandAugment leaves.  One workgroup per image with the source and the result resident in LDS;
// lafs_cvpr2024_amd/face_tensor_aug.py draws the decisions on the host with torchvision 0.9.1's own torch calls.  The pixel
// arithmetic follows torchvision 0.9.1 functional_tensor (PARITY UNPINNED: restated, torchvision is not installed) as the installed
// torch evaluates it on the CPU, so that the result is bit-identical to tests/facedataset_tv_oracle.py.
#include "common.hpp"
#include "lafs_hip.h"

// every float operation is rounded on its own unless an explicit __fmaf_rn says otherwise
#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int MAXPIX = 112 * 112;
constexpr int MAXBYTE = MAXPIX * 3;
constexpr int THREADS = 512;

// torch's CPU upsample_bilinear2d (align_corners=False) for one axis: area_pixel_compute_source_index, guard_index_and_lambda.
// The installed torch evaluates `scale * (d + 0.5) - 0.5` as one fused multiply-add; equal sizes are a plain copy.
__device__ __forceinline__ void bilinear_axis(int d, int n_in, int n_out, float scale, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  if (n_in == n_out) { i0 = i1 = d; l0 = 1.0f; l1 = 0.0f; return; }
  float s = __fmaf_rn(scale, (float)d + 0.5f, -0.5f);
  if (s < 0.0f) s = 0.0f;
  i0 = min((int)floorf(s), n_in - 1);
  l1 = fminf(fmaxf(s - (float)i0, 0.0f), 1.0f);
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l0 = 1.0f - l1;
}

// functional_tensor._blend: (r * a + (1 - r) * b).clamp(0, 255).to(uint8), r and 1 - r the float32 values of the doubles
__device__ __forceinline__ unsigned char blend(int a, float b, float r, float rc) {
#pragma clang fp contract(off)
  const float x = r * (float)a;
  const float y = rc * b;
  const float v = fminf(fmaxf(x + y, 0.0f), 255.0f);
  return (unsigned char)(int)v;
}

// rgb_to_grayscale: (0.2989 * r + 0.587 * g + 0.114 * b).to(uint8), the Python constants cast to float32
__device__ __forceinline__ int gray(int r, int g, int b) {
#pragma clang fp contract(off)
  const float v = ((float)0.2989 * (float)r + (float)0.587 * (float)g) + (float)0.114 * (float)b;
  return (int)v;
}

// adjust_hue: x / 255 -> _rgb2hsv -> h = (h + f) % 1.0 -> _hsv2rgb -> (x * 255).to(uint8)
__device__ __forceinline__ void hue_px(int R, int G, int B, float f, int& oR, int& oG, int& oB) {
#pragma clang fp contract(off)
  const float r = __fdiv_rn((float)R, 255.0f), g = __fdiv_rn((float)G, 255.0f), b = __fdiv_rn((float)B, 255.0f);
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = __fdiv_rn(cr, eqc ? 1.0f : maxc);
  const float crd = eqc ? 1.0f : cr;
  const float rc = __fdiv_rn(maxc - r, crd), gc = __fdiv_rn(maxc - g, crd), bc = __fdiv_rn(maxc - b, crd);
  float h;                                                     // exactly one of hr, hg, hb is selected; the others add zeros
  if (maxc == r) h = bc - gc;
  else if (maxc == g) h = (2.0f + rc) - bc;
  else h = (4.0f + gc) - rc;
  h = fmodf(__fdiv_rn(h, 6.0f) + 1.0f, 1.0f);
  h = h + f;                                                   // torch.remainder(h, 1.0)
  h = fmodf(h, 1.0f);
  if (h != 0.0f && h < 0.0f) h = h + 1.0f;
  const float h6 = h * 6.0f;
  const float fi = floorf(h6);
  const float fr = h6 - fi;
  int i = (int)fi % 6;
  const float v = maxc;
  const float p = fminf(fmaxf(v * (1.0f - s), 0.0f), 1.0f);
  const float q = fminf(fmaxf(v * (1.0f - s * fr), 0.0f), 1.0f);
  const float t = fminf(fmaxf(v * (1.0f - s * (1.0f - fr)), 0.0f), 1.0f);
  float xr, xg, xb;                                            // the one-hot einsum select of _hsv2rgb
  switch (i) {
    case 0: xr = v; xg = t; xb = p; break;
    case 1: xr = q; xg = v; xb = p; break;
    case 2: xr = p; xg = v; xb = t; break;
    case 3: xr = p; xg = q; xb = v; break;
    case 4: xr = t; xg = p; xb = v; break;
    default: xr = v; xg = p; xb = q; break;
  }
  oR = (int)(xr * 255.0f); oG = (int)(xg * 255.0f); oB = (int)(xb * 255.0f);
}

// global <-> LDS byte copy, 16 bytes at a time when both sides allow it
__device__ __forceinline__ void copy_bytes(unsigned char* dst, const unsigned char* src, int n, bool vec) {
  if (vec) {
    for (int e = threadIdx.x; e < n / 16; e += blockDim.x) reinterpret_cast<uint4*>(dst)[e] = reinterpret_cast<const uint4*>(src)[e];
  } else {
    for (int e = threadIdx.x; e < n; e += blockDim.x) dst[e] = src[e];
  }
}

// `out` may alias `images` (H = W = S): the whole source reaches LDS before the first store, so no __restrict__ on either
__global__ __launch_bounds__(THREADS) void face_tensor_aug_kernel(const unsigned char* in, unsigned char* out,
                                                                  const lafs_face_tensor_aug_rec* __restrict__ recs, int H, int W, int S,
                                                                  int vec_in, int vec_out) {
#pragma clang fp contract(off)
  extern __shared__ uint4 lds_raw[];
  unsigned char* const src = reinterpret_cast<unsigned char*>(lds_raw);   // [3][H][W]
  unsigned char* const dst = src + MAXBYTE;                                // [3][S][S]
  __shared__ int gray_sum;
  const int b = blockIdx.x, npix_in = H * W, npix = S * S;
  const lafs_face_tensor_aug_rec r = recs[b];
  copy_bytes(src, in + (size_t)b * npix_in * 3, npix_in * 3, vec_in != 0);
  if (threadIdx.x == 0) gray_sum = 0;
  __syncthreads();

  // -- RandomResizedCrop: crop (i, j, h, w) of the source, resampled to S x S (the record is clamped into the image: no fault)
  const int ci = min(max(r.crop_i, 0), H - 1), cj = min(max(r.crop_j, 0), W - 1);
  const int ch = min(max(r.crop_h, 1), H - ci), cw = min(max(r.crop_w, 1), W - cj);
  const float sy = __fdiv_rn((float)ch, (float)S), sx = __fdiv_rn((float)cw, (float)S);
  for (int p = threadIdx.x; p < npix; p += blockDim.x) {
    const int y = p / S, x = p - y * S;
    int y0, y1, x0, x1;
    float h0, h1, w0, w1;
    bilinear_axis(y, ch, S, sy, y0, y1, h0, h1);
    bilinear_axis(x, cw, S, sx, x0, x1, w0, w1);
    const int r0 = (ci + y0) * W + cj, r1 = (ci + y1) * W + cj;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned char* pl = src + c * npix_in;
      // torch's Interpolate<2>: t = a * w0 + b * w1 per row, then t0 * h0 + t1 * h1, each as fma(first, w, second * w)
      const float t0 = __fmaf_rn((float)pl[r0 + x0], w0, (float)pl[r0 + x1] * w1);
      const float t1 = __fmaf_rn((float)pl[r1 + x0], w0, (float)pl[r1 + x1] * w1);
      const float v = __fmaf_rn(t0, h0, t1 * h1);
      dst[c * npix + p] = (unsigned char)(int)rintf(v);       // torch.round (half to even), then the uint8 cast
    }
  }

  // -- ColorJitter: the four adjustments in the record's order; each thread owns the same pixels throughout, so only the
  //    contrast mean (a reduction over the whole image) needs barriers
  for (int k = 0; k < 4; ++k) {
    const int op = r.order[k] & 3;
    float mean = 0.0f;
    if (op == 1) {
      int part = 0;
      for (int p = threadIdx.x; p < npix; p += blockDim.x) part += gray(dst[p], dst[npix + p], dst[2 * npix + p]);
      atomicAdd(&gray_sum, part);
      __syncthreads();
      mean = __fdiv_rn((float)gray_sum, (float)npix);          // an integer below 2^24: exact in any order, then one division
    }
    for (int p = threadIdx.x; p < npix; p += blockDim.x) {
      const int R = dst[p], G = dst[npix + p], B = dst[2 * npix + p];
      int oR, oG, oB;
      if (op == 3) {
        hue_px(R, G, B, r.hue, oR, oG, oB);
      } else {
        float f, fc, d;
        if (op == 0) { f = r.brightness; fc = r.brightness_c; d = 0.0f; }
        else if (op == 1) { f = r.contrast; fc = r.contrast_c; d = mean; }
        else { f = r.saturation; fc = r.saturation_c; d = (float)gray(R, G, B); }
        oR = blend(R, d, f, fc); oG = blend(G, d, f, fc); oB = blend(B, d, f, fc);
      }
      dst[p] = (unsigned char)oR; dst[npix + p] = (unsigned char)oG; dst[2 * npix + p] = (unsigned char)oB;
    }
  }

  // -- RandomErasing: the box is set to 0
  if (r.erase) {
    const int ei = max(r.erase_i, 0), ej = max(r.erase_j, 0);
    const int ei1 = min(ei + max(r.erase_h, 0), S), ej1 = min(ej + max(r.erase_w, 0), S);
    for (int p = threadIdx.x; p < npix; p += blockDim.x) {
      const int y = p / S, x = p - y * S;
      if (y >= ei && y < ei1 && x >= ej && x < ej1) dst[p] = dst[npix + p] = dst[2 * npix + p] = 0;
    }
  }
  __syncthreads();
  copy_bytes(out + (size_t)b * npix * 3, dst, npix * 3, vec_out != 0);
}

}  // namespace

extern "C" int lafs_face_tensor_aug(const uint8_t* images, uint8_t* out, const lafs_face_tensor_aug_rec* recs, int B, int H, int W, int S,
                                    hipStream_t stream) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(images && out && recs && B > 0, "bad operand");
  LAFS_CHECK_ARG(H >= 3 && W >= 3 && H * W <= MAXPIX, "source images of 3x3 up to 112x112 pixels (the picture lives in LDS)");
  LAFS_CHECK_ARG(S >= 3 && S * S <= MAXPIX, "output side S from 3 to 112 (the result lives in LDS)");
  LAFS_CHECK_ARG(!(images == out && (H != S || W != S)), "out may alias images only when H = W = S");
  const size_t lds = 2 * (size_t)MAXBYTE;
  {                                                   // per call: the attribute is per device and the call is cheap
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(face_tensor_aug_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { lafs_set_error("lafs_face_tensor_aug: cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e)); return (int)e; }
  }
  const int vec_in = ((H * W * 3) % 16 == 0 && (reinterpret_cast<uintptr_t>(images) & 15) == 0) ? 1 : 0;
  const int vec_out = ((S * S * 3) % 16 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(face_tensor_aug_kernel, dim3(B), dim3(THREADS), lds, stream, images, out, recs, H, W, S, vec_in, vec_out);
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}
