// Baseline / extended-sequential Huffman JPEG decoding, restated from libjpeg's integer pipeline (jdhuff.c, jidctint.c "islow",
// jdsample.c "fancy" upsampling, jdcolor.c) so that the pixels equal Pillow's (libjpeg-turbo) bit for bit.
//
// Plain C++ without any HIP type: csrc/jpeg.hip compiles this text for gfx950 (JPEG_HD = __host__ __device__) and
// tests/jpeg_host_main.cpp compiles the very same text into a CPU program that runs under the sanitizers.
//
// Nothing here trusts a value it reads: every loop is bounded by block counts, every stream read is clamped to the scan's length
// (past the end, or at a marker, the reader supplies zero bits and flags the image), every table index is masked, and all
// arithmetic that a corrupt stream could drive out of range is done in wrapping unsigned integers.
#pragma once
#include <stdint.h>

#ifndef JPEG_HD
#define JPEG_HD
#endif

namespace jpegcore {

enum { MAX_DIM = 1024 };                               // largest accepted width / height
enum { QUANT_BYTES = 4 * 64 * 2, HUFF_BYTES = 16 + 256, TABLE_BYTES = QUANT_BYTES + 4 * HUFF_BYTES };   // 1600
// status bits of one image (0 = decoded)
enum { ST_RECORD = 1, ST_OVERRUN = 2, ST_CODE = 4, ST_COEF = 8, ST_RESTART = 16 };

// One 64-byte record per image (lafs_jpeg_image of include/lafs_hip.h, same layout).
struct Image {
  int64_t data_off;                                    // the scan's entropy-coded bytes inside the stream blob
  int32_t data_len;
  int32_t table_off;                                   // byte offset of this image's TABLE_BYTES block
  int32_t width, height;
  int32_t ncomp;                                       // 1 or 3
  int32_t restart_interval;                            // MCUs between RSTn markers, 0 = none
  uint8_t hs[3], vs[3], tq[3], td[3], ta[3];
  uint8_t pad[17];
};
static_assert(sizeof(Image) == 64, "one 64-byte record per image");

// Upper bound of the 8x8 blocks of any accepted sampling of a W x H image (4:4:4 has 3 * ceil(W/8) * ceil(H/8)).
JPEG_HD inline int max_blocks(int H, int W) { return 12 * ((W + 15) / 16) * ((H + 15) / 16); }
// Workspace of one image: int16 coefficients (natural order) followed by the uint8 component planes.
JPEG_HD inline int64_t image_workspace_bytes(int H, int W) { return (int64_t)max_blocks(H, W) * (128 + 64); }

// Validated geometry of one image.
struct Layout {
  int ncomp, hmax, vmax, mcux, mcuy;
  int hs[3], vs[3], tq[3], td[3], ta[3];
  int bw[3], bh[3];                                    // block grid of each component (MCU-padded)
  int blk0[3];                                         // first block of each component in the coefficient store
  int pw[3], ph[3];                                    // cropped plane size: ceil(W * hs / hmax) x ceil(H * vs / vmax)
  int total_blocks;
  int width, height;
};

// 0 when the record describes a stream this decoder accepts at exactly W x H, ST_RECORD otherwise.
JPEG_HD inline int make_layout(const Image& im, int H, int W, int64_t stream_bytes, int64_t table_bytes, Layout& L) {
  if (im.width != W || im.height != H || W < 1 || H < 1 || W > MAX_DIM || H > MAX_DIM) return ST_RECORD;
  if (im.ncomp != 1 && im.ncomp != 3) return ST_RECORD;
  if (im.data_off < 0 || im.data_len < 0 || im.data_off > stream_bytes || (int64_t)im.data_len > stream_bytes - im.data_off) return ST_RECORD;
  if (im.table_off < 0 || (int64_t)im.table_off + TABLE_BYTES > table_bytes) return ST_RECORD;
  if (im.restart_interval < 0) return ST_RECORD;
  L.ncomp = im.ncomp; L.width = W; L.height = H;
  for (int c = 0; c < 3; ++c) {
    L.hs[c] = im.hs[c]; L.vs[c] = im.vs[c];
    L.tq[c] = im.tq[c] & 3; L.td[c] = im.td[c] & 1; L.ta[c] = im.ta[c] & 1;
  }
  if (L.ncomp == 1) {                                  // a one-component scan is never interleaved: one block per MCU
    if (L.hs[0] != 1 || L.vs[0] != 1) return ST_RECORD;
  } else {
    const bool luma_ok = (L.hs[0] == 1 && L.vs[0] == 1) || (L.hs[0] == 2 && L.vs[0] == 1) || (L.hs[0] == 2 && L.vs[0] == 2);
    if (!luma_ok || L.hs[1] != 1 || L.vs[1] != 1 || L.hs[2] != 1 || L.vs[2] != 1) return ST_RECORD;
  }
  L.hmax = L.hs[0]; L.vmax = L.vs[0];
  L.mcux = (W + 8 * L.hmax - 1) / (8 * L.hmax);
  L.mcuy = (H + 8 * L.vmax - 1) / (8 * L.vmax);
  int blocks = 0;
  for (int c = 0; c < 3; ++c) {
    if (c >= L.ncomp) { L.bw[c] = L.bh[c] = L.pw[c] = L.ph[c] = 0; L.blk0[c] = blocks; L.hs[c] = L.vs[c] = 1; continue; }
    L.bw[c] = L.mcux * L.hs[c]; L.bh[c] = L.mcuy * L.vs[c];
    L.pw[c] = (W * L.hs[c] + L.hmax - 1) / L.hmax;
    L.ph[c] = (H * L.vs[c] + L.vmax - 1) / L.vmax;
    L.blk0[c] = blocks;
    blocks += L.bw[c] * L.bh[c];
  }
  L.total_blocks = blocks;
  if (blocks > max_blocks(H, W)) return ST_RECORD;     // (cannot happen for the accepted samplings; the stores rely on it)
  return 0;
}

// ---- tables -----------------------------------------------------------------------------------------------------------------

// natural (row-major) index of the k-th coefficient of the zigzag sequence
JPEG_HD inline int zigzag_natural(int k) {
  const unsigned char t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return t[k & 63];
}

// Derived Huffman table: an 8-bit look-ahead (length << 8 | value, 0 = longer code) and, for longer codes, libjpeg's
// maxcode / valoffset per length.
struct Huff {
  int32_t maxcode[17];                                 // [l] largest code of length l, -1 when none
  int32_t valoff[17];                                  // [l] index of the first value of length l minus its first code
  uint16_t look[256];
  uint8_t vals[256];
};

// BITS (16 bytes) + HUFFVAL (256 bytes) -> Huff.  A malformed table (more than 256 codes, over-subscribed code space) is cut
// where it goes wrong; the host parser refuses such streams, so this only keeps the walk inside the arrays.
JPEG_HD inline void build_huff(const uint8_t* t, Huff& h) {
  for (int i = 0; i < 256; ++i) { h.look[i] = 0; h.vals[i] = t[16 + i]; }
  h.maxcode[0] = -1; h.valoff[0] = 0;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    int n = t[l - 1];
    if (k + n > 256) n = 256 - k;
    if (code + n > (1 << l)) n = (1 << l) - code > 0 ? (1 << l) - code : 0;
    h.valoff[l] = k - code;
    h.maxcode[l] = n ? code + n - 1 : -1;
    if (l <= 8) {
      for (int i = 0; i < n; ++i) {
        const int first = (code + i) << (8 - l);
        for (int j = 0; j < (1 << (8 - l)); ++j) h.look[(first + j) & 255] = (uint16_t)((l << 8) | h.vals[k + i]);
      }
    }
    k += n;
    code = (code + n) << 1;
  }
}

// ---- bit reader -------------------------------------------------------------------------------------------------------------

struct BitReader {
  const uint8_t* p;
  int len, pos;
  uint32_t acc;                                        // the low `nbits` bits are unread, oldest on top
  int nbits, fake;                                     // `fake` of them (the youngest) are zero bits supplied past the data
  bool stopped;                                        // at a marker or at the end: only zero bits from here on
  int status;
};

JPEG_HD inline void br_init(BitReader& br, const uint8_t* p, int len) {
  br.p = p; br.len = len; br.pos = 0; br.acc = 0; br.nbits = 0; br.fake = 0; br.stopped = false; br.status = 0;
}

// Top the accumulator up to at least 25 bits.  FF 00 is a stuffed FF; FF followed by anything else is a marker, which is left
// in place (the restart logic looks at it) and reads as zero bits.
JPEG_HD inline void br_fill(BitReader& br) {
  while (br.nbits <= 24) {
    uint32_t b = 0;
    if (!br.stopped && br.pos < br.len) {
      b = br.p[br.pos];
      if (b == 0xFF) {
        if (br.pos + 1 < br.len && br.p[br.pos + 1] == 0x00) br.pos += 2;
        else { br.stopped = true; b = 0; }
      } else {
        br.pos += 1;
      }
    } else {
      br.stopped = true;
    }
    if (br.stopped) br.fake += 8;
    br.acc = (br.acc << 8) | b;
    br.nbits += 8;
  }
}
JPEG_HD inline uint32_t br_peek(const BitReader& br, int n) {      // 1 <= n <= 16 <= nbits
  return (br.acc >> (br.nbits - n)) & ((1u << n) - 1u);
}
JPEG_HD inline void br_skip(BitReader& br, int n) {
  br.nbits -= n;
  if (br.nbits < br.fake) { br.status |= ST_OVERRUN; br.fake = br.nbits; }
}

JPEG_HD inline int decode_symbol(BitReader& br, const Huff& h) {
  br_fill(br);
  const uint32_t e = h.look[br_peek(br, 8)];
  if (e) { br_skip(br, (int)(e >> 8)); return (int)(e & 255u); }
  for (int l = 9; l <= 16; ++l) {
    const int code = (int)br_peek(br, l);
    if (code <= h.maxcode[l]) { br_skip(br, l); return h.vals[(code + h.valoff[l]) & 255]; }
  }
  br.status |= ST_CODE;
  br_skip(br, 16);
  return 0;
}

// `s` further bits as a signed value (jdhuff.c HUFF_EXTEND), 0 <= s <= 15
JPEG_HD inline int receive_extend(BitReader& br, int s) {
  if (s == 0) return 0;
  br_fill(br);
  const int v = (int)br_peek(br, s);
  br_skip(br, s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One 8x8 block into coef[64] (natural order, zeroed by the caller).  At most 1 + 63 symbols.  zz[64] = zigzag_natural(0..63), held by
// the caller where the serial walk reads it fastest (LDS on the device).
JPEG_HD inline void decode_block(BitReader& br, const Huff& dc, const Huff& ac, int& pred, int16_t* coef, const uint8_t* zz) {
  int s = decode_symbol(br, dc);
  if (s > 15) { br.status |= ST_CODE; s = 15; }
  pred += receive_extend(br, s);
  if (pred > 32767 || pred < -32768) { br.status |= ST_COEF; pred = 0; }
  coef[0] = (int16_t)pred;
  int k = 1;
  for (int step = 0; step < 63 && k < 64; ++step) {
    const int rs = decode_symbol(br, ac);
    const int r = rs >> 4;
    s = rs & 15;
    if (s) {
      k += r;
      if (k > 63) { br.status |= ST_COEF; return; }
      coef[zz[k]] = (int16_t)receive_extend(br, s);
      ++k;
    } else {
      if (r != 15) return;                             // EOB
      k += 16;                                         // ZRL
      if (k > 64) { br.status |= ST_COEF; return; }
    }
  }
}

// At a restart boundary: drop the padding bits, step over RSTn (n = count mod 8; FF fill bytes may precede it).
JPEG_HD inline void restart(BitReader& br, int count) {
  br.acc = 0; br.nbits = 0; br.fake = 0; br.stopped = false;
  while (br.pos + 2 < br.len && br.p[br.pos] == 0xFF && br.p[br.pos + 1] == 0xFF) br.pos += 1;
  if (br.pos + 1 < br.len && br.p[br.pos] == 0xFF && br.p[br.pos + 1] == (0xD0 | (count & 7))) br.pos += 2;
  else { br.status |= ST_RESTART; br.stopped = true; }
}

// The whole scan of one image: coef = total_blocks * 64 int16, zeroed by the caller; component c's block (by, bx) lives at
// (blk0[c] + by * bw[c] + bx) * 64.  Returns the status bits.  `data` may point at a staged copy of the scan's bytes.
JPEG_HD inline int decode_scan(const Layout& L, const uint8_t* data, int data_len, int restart_interval, const Huff* huff /* DC0 DC1 AC0 AC1 */,
                               const uint8_t* zz /* zigzag_natural(0..63) */, int16_t* coef) {
  BitReader br;
  br_init(br, data, data_len);
  int pred[3] = {0, 0, 0};
  const int n_mcu = L.mcux * L.mcuy;
  int since = 0, rst = 0;
  for (int m = 0; m < n_mcu; ++m) {
    if (restart_interval > 0 && since == restart_interval) {
      restart(br, rst);
      rst += 1; since = 0;
      pred[0] = pred[1] = pred[2] = 0;
    }
    const int my = m / L.mcux, mx = m - my * L.mcux;
    for (int c = 0; c < L.ncomp; ++c) {
      const Huff& dc = huff[L.td[c]];
      const Huff& ac = huff[2 + L.ta[c]];
      for (int v = 0; v < L.vs[c]; ++v)
        for (int h = 0; h < L.hs[c]; ++h) {
          const int by = my * L.vs[c] + v, bx = mx * L.hs[c] + h;
          decode_block(br, dc, ac, pred[c], coef + (int64_t)(L.blk0[c] + by * L.bw[c] + bx) * 64, zz);
        }
    }
    since += 1;
  }
  return br.status;
}

// ---- dequantise + IDCT (jidctint.c jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2) -------------------------------------------------
// In wrapping 32-bit arithmetic: the same bits as libjpeg's `int` code wherever that does not overflow, and defined behaviour where a
// corrupt stream would make it.

JPEG_HD inline uint32_t descale(uint32_t x, int n) { return (uint32_t)((int32_t)(x + (1u << (n - 1))) >> n); }

JPEG_HD inline void idct_1d(const uint32_t in[8], uint32_t out[8], int shift) {
  const uint32_t F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299,
                 F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;
  uint32_t z2 = in[2], z3 = in[6];
  uint32_t z1 = (z2 + z3) * F_0_541;
  uint32_t tmp2 = z1 - z3 * F_1_847;
  uint32_t tmp3 = z1 + z2 * F_0_765;
  z2 = in[0]; z3 = in[4];
  uint32_t tmp0 = (z2 + z3) * 8192u;
  uint32_t tmp1 = (z2 - z3) * 8192u;
  const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  uint32_t z4 = tmp1 + tmp3;
  const uint32_t z5 = (z3 + z4) * F_1_175;
  tmp0 *= F_0_298; tmp1 *= F_2_053; tmp2 *= F_3_072; tmp3 *= F_1_501;
  z1 *= (0u - F_0_899); z2 *= (0u - F_2_562); z3 *= (0u - F_1_961); z4 *= (0u - F_0_390);
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  out[0] = descale(tmp10 + tmp3, shift); out[7] = descale(tmp10 - tmp3, shift);
  out[1] = descale(tmp11 + tmp2, shift); out[6] = descale(tmp11 - tmp2, shift);
  out[2] = descale(tmp12 + tmp1, shift); out[5] = descale(tmp12 - tmp1, shift);
  out[3] = descale(tmp13 + tmp0, shift); out[4] = descale(tmp13 - tmp0, shift);
}

JPEG_HD inline uint16_t quant_entry(const uint8_t* tables, int tq, int k) {        // DQT (zigzag) order, little-endian uint16
  const uint8_t* q = tables + (tq & 3) * 128 + (k & 63) * 2;
  return (uint16_t)(q[0] | (q[1] << 8));
}

// One block: coef (natural order) x quantiser -> 8x8 samples at dst (row stride `stride`).
JPEG_HD inline void idct_block(const int16_t* coef, const uint8_t* tables, int tq, uint8_t* dst, int stride) {
  uint32_t ws[64];
  uint32_t nat_q[64];
  for (int k = 0; k < 64; ++k) nat_q[zigzag_natural(k)] = quant_entry(tables, tq, k);
  for (int c = 0; c < 8; ++c) {                        // pass 1: columns, descale by CONST_BITS - PASS1_BITS = 11
    uint32_t in[8], out[8];
    for (int r = 0; r < 8; ++r) in[r] = (uint32_t)(int32_t)coef[r * 8 + c] * nat_q[r * 8 + c];
    idct_1d(in, out, 11);
    for (int r = 0; r < 8; ++r) ws[r * 8 + c] = out[r];
  }
  for (int r = 0; r < 8; ++r) {                        // pass 2: rows, descale by CONST_BITS + PASS1_BITS + 3 = 18
    uint32_t out[8];
    idct_1d(ws + r * 8, out, 18);
    for (int c = 0; c < 8; ++c) {
      const int32_t v = (int32_t)out[c] + 128;
      dst[r * stride + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
  }
}

// ---- upsampling + colour ----------------------------------------------------------------------------------------------------------

// The sample of a chroma plane (pw x ph valid samples, row stride `stride`) that libjpeg's upsampler puts at output pixel (x, y),
// for horizontal / vertical factors hf, vf in {1, 2} (jdsample.c: fancy h2v1 / h2v2 when the plane is wider than 2, replication
// otherwise).
JPEG_HD inline int upsample_at(const uint8_t* plane, int stride, int pw, int ph, int hf, int vf, int x, int y) {
  if (hf == 1 && vf == 1) return plane[y * stride + x];
  const int cx = x >> 1;
  if (pw <= 2 || !(vf == 1 || vf == 2)) return plane[(vf == 2 ? y >> 1 : y) * stride + cx];
  if (vf == 1) {                                       // fancy h2v1
    const uint8_t* row = plane + y * stride;
    const int cur = row[cx];
    if (!(x & 1)) return cx == 0 ? cur : (3 * cur + row[cx - 1] + 1) >> 2;
    return cx == pw - 1 ? cur : (3 * cur + row[cx + 1] + 2) >> 2;
  }
  const int cy = y >> 1;                               // fancy h2v2
  int ny = (y & 1) ? cy + 1 : cy - 1;
  ny = ny < 0 ? 0 : (ny > ph - 1 ? ph - 1 : ny);
  const uint8_t* r0 = plane + cy * stride;
  const uint8_t* r1 = plane + ny * stride;
  const int cs = 3 * r0[cx] + r1[cx];
  if (!(x & 1)) return cx == 0 ? (4 * cs + 8) >> 4 : (3 * cs + (3 * r0[cx - 1] + r1[cx - 1]) + 8) >> 4;
  return cx == pw - 1 ? (4 * cs + 7) >> 4 : (3 * cs + (3 * r0[cx + 1] + r1[cx + 1]) + 7) >> 4;
}

JPEG_HD inline uint8_t clamp8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// jdcolor.c ycc_rgb_convert: FIX(v) = int(v * 65536 + 0.5), ONE_HALF = 32768, arithmetic right shift
JPEG_HD inline void ycc_to_rgb(int y, int cb, int cr, uint8_t& r, uint8_t& g, uint8_t& b) {
  const int xb = cb - 128, xr = cr - 128;
  r = clamp8(y + ((91881 * xr + 32768) >> 16));
  b = clamp8(y + ((116130 * xb + 32768) >> 16));
  g = clamp8(y + ((-22554 * xb + 32768 - 46802 * xr) >> 16));
}

// Plane of component c inside the plane store (after the coefficients): MCU-padded, row stride bw[c] * 8.
JPEG_HD inline int64_t plane_offset(const Layout& L, int c) { return (int64_t)L.blk0[c] * 64; }

// Output pixel (x, y) of image L from its planes into out[3][H][W].
JPEG_HD inline void write_pixel(const Layout& L, const uint8_t* planes, int x, int y, uint8_t* out) {
  const int64_t npix = (int64_t)L.width * L.height, o = (int64_t)y * L.width + x;
  const int yy = planes[plane_offset(L, 0) + (int64_t)y * (L.bw[0] * 8) + x];
  if (L.ncomp == 1) { out[o] = out[npix + o] = out[2 * npix + o] = (uint8_t)yy; return; }
  const int cb = upsample_at(planes + plane_offset(L, 1), L.bw[1] * 8, L.pw[1], L.ph[1], L.hmax, L.vmax, x, y);
  const int cr = upsample_at(planes + plane_offset(L, 2), L.bw[2] * 8, L.pw[2], L.ph[2], L.hmax, L.vmax, x, y);
  ycc_to_rgb(yy, cb, cr, out[o], out[npix + o], out[2 * npix + o]);
}

// The IDCT of block `blk` (0 <= blk < total_blocks) into its plane.
JPEG_HD inline void idct_into_plane(const Layout& L, const int16_t* coef, const uint8_t* tables, uint8_t* planes, int blk) {
  int c = 0;
  if (L.ncomp == 3) c = blk >= L.blk0[2] ? 2 : (blk >= L.blk0[1] ? 1 : 0);
  const int local = blk - L.blk0[c], by = local / L.bw[c], bx = local - by * L.bw[c];
  const int stride = L.bw[c] * 8;
  idct_block(coef + (int64_t)blk * 64, tables, L.tq[c], planes + plane_offset(L, c) + (int64_t)by * 8 * stride + bx * 8, stride);
}

}  // namespace jpegcore
