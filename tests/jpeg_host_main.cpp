// CPU driver of csrc/jpeg_core.hpp for tests/test_jpeg_host.py: the same text the gfx950 kernel is compiled from, run as an
// ordinary program (built with -fsanitize=address,undefined by the test).
//
//   jpeg_host_main IN OUT
// IN is a sequence of batches, each: int64 B, H, W, stream_bytes, table_bytes | B x 64-byte image records | stream | tables
// OUT gets, per batch: int32 status[B] | uint8 pixels[B][3][H][W]
// Every buffer is a heap block of exactly the size the C ABI asks for, so that an out-of-bounds access is caught.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lafs_cvpr2024_amd/csrc/jpeg_core.hpp"

using namespace jpegcore;

static bool read_exact(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
  for (;;) {
    int64_t head[5];
    const size_t got = fread(head, 1, sizeof(head), in);
    if (got == 0) break;
    if (got != sizeof(head)) { fprintf(stderr, "truncated batch header\n"); return 2; }
    const int64_t B = head[0], H = head[1], W = head[2], stream_bytes = head[3], table_bytes = head[4];
    if (B <= 0 || B > (1 << 20) || H <= 0 || W <= 0 || H > MAX_DIM || W > MAX_DIM || stream_bytes < 0 || table_bytes < 0 ||
        stream_bytes > (1ll << 31) || table_bytes > (1ll << 31)) { fprintf(stderr, "bad batch header\n"); return 2; }
    std::vector<Image> images((size_t)B);
    std::vector<uint8_t> stream((size_t)stream_bytes), tables((size_t)table_bytes);
    if (!read_exact(in, images.data(), (size_t)B * sizeof(Image)) || !read_exact(in, stream.data(), stream.size()) ||
        !read_exact(in, tables.data(), tables.size())) { fprintf(stderr, "truncated batch\n"); return 2; }
    std::vector<int32_t> status((size_t)B, 0);
    std::vector<uint8_t> pixels((size_t)(B * 3 * H * W), 0);
    for (int64_t b = 0; b < B; ++b) {
      const Image& im = images[(size_t)b];
      Layout L;
      int st = make_layout(im, (int)H, (int)W, stream_bytes, table_bytes, L);
      if (st == 0) {
        // one image's workspace slice, as the kernel lays it out: coefficients, then planes
        std::vector<uint8_t> ws((size_t)image_workspace_bytes((int)H, (int)W), 0);
        int16_t* coef = reinterpret_cast<int16_t*>(ws.data());
        uint8_t* planes = ws.data() + (size_t)max_blocks((int)H, (int)W) * 128;
        const uint8_t* tab = tables.data() + im.table_off;
        std::vector<Huff> huff(4);
        for (int t = 0; t < 4; ++t) build_huff(tab + QUANT_BYTES + t * HUFF_BYTES, huff[(size_t)t]);
        std::vector<uint8_t> zz(64);
        for (int k = 0; k < 64; ++k) zz[(size_t)k] = (uint8_t)zigzag_natural(k);
        std::vector<uint8_t> scan(stream.begin() + im.data_off, stream.begin() + im.data_off + im.data_len);   // exact-size copy
        st = decode_scan(L, scan.data(), im.data_len, im.restart_interval, huff.data(), zz.data(), coef);
        for (int blk = 0; blk < L.total_blocks; ++blk) idct_into_plane(L, coef, tab, planes, blk);
        uint8_t* o = pixels.data() + (size_t)(b * 3 * H * W);
        for (int y = 0; y < (int)H; ++y)
          for (int x = 0; x < (int)W; ++x) write_pixel(L, planes, x, y, o);
      }
      status[(size_t)b] = st;
    }
    if (fwrite(status.data(), sizeof(int32_t), status.size(), out) != status.size() ||
        fwrite(pixels.data(), 1, pixels.size(), out) != pixels.size()) { fprintf(stderr, "write failed\n"); return 2; }
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  return 0;
}
