// Device-side JPEG decode of the RecordIO loaders (lafs_cvpr2024_amd/jpeg.py): baseline / extended-sequential Huffman streams,
// gray or YCbCr 4:4:4 / 4:2:2 / 4:2:0, bit-identical to Pillow (libjpeg-turbo).  All arithmetic lives in jpeg_core.hpp, which also
// compiles into the CPU program of tests/test_jpeg_host.py; this file only spreads it over one workgroup per image:
//   1. the workgroup zeroes the image's coefficient store, stages the scan's bytes in LDS and derives the four Huffman tables;
//   2. one lane walks the bit stream (Huffman decoding is serial) and writes int16 coefficients;
//   3. one thread per 8x8 block: dequantise + IDCT into uint8 component planes;
//   4. one thread per output pixel: chroma upsampling + YCbCr -> RGB into out[b].
// All images of a batch run concurrently; no atomics, so the bits are the same run to run.  The host parser validates the
// streams, but the kernel trusts nothing it reads from device memory (see jpeg_core.hpp): an image it cannot decode gets a
// non-zero status and still writes only inside its own slot and workspace slice.
#include "common.hpp"
#include "lafs_hip.h"
#define JPEG_HD __host__ __device__
#include "jpeg_core.hpp"

namespace {

using namespace jpegcore;

static_assert(sizeof(lafs_jpeg_image) == sizeof(Image), "lafs_jpeg_image is jpegcore::Image");
static_assert(offsetof(lafs_jpeg_image, data_len) == offsetof(Image, data_len) && offsetof(lafs_jpeg_image, table_off) == offsetof(Image, table_off) &&
              offsetof(lafs_jpeg_image, width) == offsetof(Image, width) && offsetof(lafs_jpeg_image, restart_interval) == offsetof(Image, restart_interval) &&
              offsetof(lafs_jpeg_image, hs) == offsetof(Image, hs) && offsetof(lafs_jpeg_image, ta) == offsetof(Image, ta),
              "lafs_jpeg_image is jpegcore::Image");
static_assert(LAFS_JPEG_MAX_DIM == MAX_DIM && LAFS_JPEG_TABLE_BYTES == TABLE_BYTES, "header constants");

constexpr int THREADS = 256;
constexpr int STAGE_BYTES = 40960;                     // scans up to this size are walked from LDS, longer ones from global memory

__global__ __launch_bounds__(THREADS) void jpeg_decode_kernel(const uint8_t* __restrict__ stream, int64_t stream_bytes,
                                                              const Image* __restrict__ images, const uint8_t* __restrict__ tables,
                                                              int64_t table_bytes, int H, int W, uint8_t* __restrict__ out,
                                                              int32_t* __restrict__ status, uint8_t* __restrict__ workspace) {
  __shared__ Layout L;
  __shared__ Huff huff[4];
  __shared__ int st;
  __shared__ uint8_t zz[64];
  __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const Image im = images[b];
  if (tid == 0) st = make_layout(im, H, W, stream_bytes, table_bytes, L);
  __syncthreads();
  if (st != 0) {                                       // not a record of this decoder: nothing is read or written for it
    if (tid == 0) status[b] = st;
    return;
  }
  const uint8_t* tab = tables + im.table_off;
  const uint8_t* data = stream + im.data_off;
  int16_t* coef = reinterpret_cast<int16_t*>(workspace + (size_t)b * image_workspace_bytes(H, W));
  uint8_t* planes = reinterpret_cast<uint8_t*>(coef) + (size_t)max_blocks(H, W) * 128;
  const int n_blocks = L.total_blocks;

  {                                                    // 1. zero the coefficients (the slice is 64-byte aligned), stage, tables
    uint4* z = reinterpret_cast<uint4*>(coef);
    for (int i = tid; i < n_blocks * 8; i += THREADS) z[i] = make_uint4(0, 0, 0, 0);
    const bool staged = im.data_len <= STAGE_BYTES;
    if (staged)
      for (int i = tid; i < im.data_len; i += THREADS) stage[i] = data[i];
    if (tid < 4) build_huff(tab + QUANT_BYTES + tid * HUFF_BYTES, huff[tid]);
    if (tid >= 64 && tid < 128) zz[tid - 64] = (uint8_t)zigzag_natural(tid - 64);
    __syncthreads();
    if (tid == 0) {                                    // 2. the serial walk
      // two call sites, so that the staged walk reads LDS with DS instructions: through one generic pointer every byte would be a
      // FLAT load, whose wait also waits for the coefficient stores in flight (measured: 6.3 ms instead of 4.3 ms per batch of 128 112x112 4:2:0 images)
      if (staged) st = decode_scan(L, stage, im.data_len, im.restart_interval, huff, zz, coef);
      else st = decode_scan(L, data, im.data_len, im.restart_interval, huff, zz, coef);
    }
    __syncthreads();
  }
  for (int blk = tid; blk < n_blocks; blk += THREADS)  // 3.
    idct_into_plane(L, coef, tab, planes, blk);
  __syncthreads();
  uint8_t* o = out + (size_t)b * 3 * H * W;            // 4.
  for (int p = tid; p < H * W; p += THREADS) {
    const int y = p / W;
    write_pixel(L, planes, p - y * W, y, o);
  }
  if (tid == 0) status[b] = st;
}

}  // namespace

extern "C" int64_t lafs_jpeg_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || H > MAX_DIM || W > MAX_DIM) return -1;
  return (int64_t)B * image_workspace_bytes(H, W);
}

extern "C" int lafs_jpeg_decode(const uint8_t* stream, int64_t stream_bytes, const lafs_jpeg_image* images, const uint8_t* tables,
                                int64_t table_bytes, int B, int H, int W, uint8_t* out, int32_t* status, void* workspace,
                                hipStream_t stream_id) {
  LAFS_CLEAR_ERROR();
  LAFS_CHECK_ARG(stream && images && tables && out && status && workspace, "null operand");
  LAFS_CHECK_ARG(B > 0 && H > 0 && W > 0 && stream_bytes > 0 && table_bytes >= TABLE_BYTES, "non-positive size");
  LAFS_CHECK_ARG(H <= MAX_DIM && W <= MAX_DIM, "images of up to LAFS_JPEG_MAX_DIM x LAFS_JPEG_MAX_DIM pixels");
  LAFS_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(images) & 7) == 0, "workspace / records not aligned");
  hipLaunchKernelGGL(jpeg_decode_kernel, dim3(B), dim3(THREADS), 0, stream_id, stream, stream_bytes, reinterpret_cast<const Image*>(images), tables,
                     table_bytes, H, W, out, status, reinterpret_cast<uint8_t*>(workspace));
  LAFS_LAUNCH_CHECK();
  return LAFS_OK;
}
