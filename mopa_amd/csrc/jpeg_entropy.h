// The host half of the JPEG decoder (csrc/jpegdec.hip holds the device half): marker parser and Huffman decoding of baseline
// sequential streams, down to the quantised coefficients.  Plain C++, no HIP header: it also compiles on its own
// (tests/jpeg_entropy_check.cpp builds it with the host compiler under the address and undefined-behaviour sanitizers).
//
// Supported: SOF0, 8-bit samples, 1 component or 3 components with chroma at 1 x 1 and luma at 1 x 1, 2 x 1 or 2 x 2, one interleaved
// scan, restart intervals, any Huffman tables, sides up to JPEG_MAX_SIDE.  Everything else is refused with MOPA_ERR_UNSUPPORTED
// before a coefficient is written (JpegHeader::reason says why); a malformed stream returns MOPA_ERR_DATA.
//
// The stream is untrusted: every read is checked against the end of the input (JpegBits never moves past `end`), every write against
// the end of the output (the block grid is sized from the validated frame header and the buffer size is checked before the scan), and
// every loop either consumes input or counts down a bound taken from the header.
//
// Output buffer of one image (int16 units, byte offsets in the header):
//   [0, 384)                    the quantisation tables of the three components, uint16[3][64], natural order (unused rows 0)
//   plane_off[c] ...            component c: int16 [blocks_y][blocks_x][64], natural (de-zigzagged) order, grid padded to whole MCUs
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef MOPA_OK
#define MOPA_OK 0
#define MOPA_ERR_ARG (-1)
#endif
#ifndef MOPA_ERR_UNSUPPORTED
#define MOPA_ERR_UNSUPPORTED (-4)   // a JPEG stream outside the supported subset (the caller falls back to another decoder)
#define MOPA_ERR_DATA (-5)          // a malformed JPEG stream
#endif

#define JPEG_MAX_SIDE 8192
#define JPEG_QUANT_BYTES 384        // uint16[3][64] in front of the planes

enum JpegReason {
  JPEG_SUPPORTED = 0,
  JPEG_R_PROGRESSIVE = 1,    // SOF2
  JPEG_R_CODING = 2,         // extended sequential, lossless, arithmetic, differential (SOF1, 3, 5..15)
  JPEG_R_PRECISION = 3,      // not 8-bit samples
  JPEG_R_COMPONENTS = 4,     // not 1 or 3 components
  JPEG_R_SAMPLING = 5,       // other sampling factors
  JPEG_R_COLORSPACE = 6,     // Adobe transform flag not YCbCr, or components named R, G, B
  JPEG_R_SCANS = 7,          // several scans / a scan that is not the whole interleaved frame
  JPEG_R_SIZE = 8,           // a side above JPEG_MAX_SIDE
};

// 64-bit fields first: the same layout for every compiler (mopa_amd/jpegdec.py::Header mirrors it).
struct JpegHeader {
  int64_t plane_off[3];      // byte offsets of the coefficient planes in the output buffer
  int64_t coeff_bytes;       // size of the output buffer
  int32_t width, height, ncomp;
  int32_t hs, vs;            // luma sampling factors (chroma is 1 x 1); 1, 1 for one component
  int32_t mcus_x, mcus_y;
  int32_t blocks_x[3], blocks_y[3];
  int32_t comp_w[3], comp_h[3];     // the components' real (not padded) sizes: ceil(width / hs), ceil(height / vs) for chroma
  int32_t restart_interval;
  int32_t supported;         // 1 / 0
  int32_t reason;            // JpegReason
  uint16_t quant[3][64];     // natural order
};

static const uint8_t JPEG_NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

#define JPEG_LOOK 9
struct JpegHuff {
  uint8_t present;
  uint8_t look_len[1 << JPEG_LOOK];   // code length of the code that starts these 9 bits, 0 = longer than 9 (or none)
  uint8_t look_sym[1 << JPEG_LOOK];
  int32_t maxcode[18];                // largest code of each length, -1 = none; [17] is a sentinel
  int32_t valoff[17];                 // index of the first value of the length minus its first code
  uint8_t vals[256];
};

struct JpegParsed {
  JpegHeader h;
  JpegHuff dc[4], ac[4];
  uint16_t qt[4][64];        // natural order
  uint8_t qt_present[4];
  uint8_t comp_id[3], comp_tq[3], comp_td[3], comp_ta[3];
  const uint8_t* scan;       // first entropy-coded byte
};

static inline int jpeg_build_huff(JpegHuff& t, const uint8_t* counts, const uint8_t* vals, bool is_dc) {
  memset(&t, 0, sizeof(t));
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    const int n = counts[len - 1];
    if (code + n > (1 << len)) return MOPA_ERR_DATA;      // over-subscribed
    t.valoff[len] = k - code;
    t.maxcode[len] = n ? code + n - 1 : -1;
    for (int i = 0; i < n; ++i, ++k, ++code) {
      const uint8_t v = vals[k];
      if (is_dc && v > 15) return MOPA_ERR_DATA;
      t.vals[k] = v;
      if (len <= JPEG_LOOK) {
        const int first = code << (JPEG_LOOK - len), span = 1 << (JPEG_LOOK - len);
        for (int j = 0; j < span; ++j) {
          t.look_len[first + j] = (uint8_t)len;
          t.look_sym[first + j] = v;
        }
      }
    }
    code <<= 1;
  }
  t.maxcode[17] = 0x7FFFFFFF;
  t.present = 1;
  return MOPA_OK;
}

// Walks the markers in front of the entropy-coded data.  MOPA_OK: h is complete and the stream is supported; MOPA_ERR_UNSUPPORTED:
// h.reason says why (the geometry is filled in if the frame header was reached); MOPA_ERR_DATA: malformed.
static inline int jpeg_parse(const uint8_t* d, int64_t n, JpegParsed& P) {
  memset(&P, 0, sizeof(P));
  JpegHeader& h = P.h;
  if (!d || n < 2 || d[0] != 0xFF || d[1] != 0xD8) return MOPA_ERR_DATA;
  int64_t p = 2;
  bool have_frame = false, jfif = false, adobe = false;
  int adobe_transform = 0;
  for (;;) {
    if (p >= n || d[p] != 0xFF) return MOPA_ERR_DATA;
    while (p < n && d[p] == 0xFF) ++p;                   // fill bytes
    if (p >= n) return MOPA_ERR_DATA;
    const int m = d[p++];
    if (m == 0x00 || m == 0x01 || m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7)) return MOPA_ERR_DATA;
    if (p + 2 > n) return MOPA_ERR_DATA;
    const int64_t len = (int64_t)d[p] << 8 | d[p + 1];
    if (len < 2 || p + len > n) return MOPA_ERR_DATA;
    const uint8_t* s = d + p + 2;
    const int sl = (int)len - 2;
    p += len;
    if (m >= 0xC0 && m <= 0xCF && m != 0xC0 && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      if (sl >= 6) {
        h.height = s[1] << 8 | s[2];
        h.width = s[3] << 8 | s[4];
        h.ncomp = s[5];
      }
      h.reason = m == 0xC2 ? JPEG_R_PROGRESSIVE : JPEG_R_CODING;
      return MOPA_ERR_UNSUPPORTED;
    }
    if (m == 0xCC) {
      h.reason = JPEG_R_CODING;                           // arithmetic conditioning
      return MOPA_ERR_UNSUPPORTED;
    }
    if (m == 0xC0) {
      if (have_frame || sl < 6) return MOPA_ERR_DATA;
      const int prec = s[0], nc = s[5];
      h.height = s[1] << 8 | s[2];
      h.width = s[3] << 8 | s[4];
      h.ncomp = nc;
      if (sl != 6 + 3 * nc) return MOPA_ERR_DATA;
      if (prec != 8) { h.reason = JPEG_R_PRECISION; return MOPA_ERR_UNSUPPORTED; }
      if (h.width == 0 || h.height == 0) return MOPA_ERR_DATA;
      if (nc != 1 && nc != 3) { h.reason = JPEG_R_COMPONENTS; return MOPA_ERR_UNSUPPORTED; }
      if (h.width > JPEG_MAX_SIDE || h.height > JPEG_MAX_SIDE) { h.reason = JPEG_R_SIZE; return MOPA_ERR_UNSUPPORTED; }
      int ch[3], cv[3];
      for (int i = 0; i < nc; ++i) {
        P.comp_id[i] = s[6 + 3 * i];
        ch[i] = s[7 + 3 * i] >> 4;
        cv[i] = s[7 + 3 * i] & 15;
        P.comp_tq[i] = s[8 + 3 * i];
      }
      if (nc == 1) {
        h.hs = h.vs = 1;                                  // the factors of a single component do not matter
      } else {
        const bool luma = (ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2);
        if (!luma || ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1) { h.reason = JPEG_R_SAMPLING; return MOPA_ERR_UNSUPPORTED; }
        h.hs = ch[0];
        h.vs = cv[0];
      }
      for (int i = 0; i < nc; ++i)
        if (P.comp_tq[i] > 3) return MOPA_ERR_DATA;
      have_frame = true;
    } else if (m == 0xDB) {
      int q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        if (pq > 1 || tq > 3) return MOPA_ERR_DATA;
        const int size = 64 * (pq + 1);
        if (q + 1 + size > sl) return MOPA_ERR_DATA;
        for (int k = 0; k < 64; ++k)
          P.qt[tq][JPEG_NATURAL[k]] = pq ? (uint16_t)(s[q + 1 + 2 * k] << 8 | s[q + 2 + 2 * k]) : s[q + 1 + k];
        P.qt_present[tq] = 1;
        q += 1 + size;
      }
    } else if (m == 0xC4) {
      int q = 0;
      while (q < sl) {
        if (q + 17 > sl) return MOPA_ERR_DATA;
        const int tc = s[q] >> 4, th = s[q] & 15;
        int total = 0;
        for (int k = 0; k < 16; ++k) total += s[q + 1 + k];
        if (tc > 1 || th > 3 || total > 256 || q + 17 + total > sl) return MOPA_ERR_DATA;
        const int rc = jpeg_build_huff(tc ? P.ac[th] : P.dc[th], s + q + 1, s + q + 17, tc == 0);
        if (rc != MOPA_OK) return rc;
        q += 17 + total;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return MOPA_ERR_DATA;
      h.restart_interval = s[0] << 8 | s[1];
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
    } else if (m == 0xDA) {
      if (!have_frame) return MOPA_ERR_DATA;
      const int nc = h.ncomp;
      if (sl < 1 || sl != 4 + 2 * s[0]) return MOPA_ERR_DATA;
      if (s[0] != nc) { h.reason = JPEG_R_SCANS; return MOPA_ERR_UNSUPPORTED; }
      for (int i = 0; i < nc; ++i) {
        if (s[1 + 2 * i] != P.comp_id[i]) { h.reason = JPEG_R_SCANS; return MOPA_ERR_UNSUPPORTED; }
        P.comp_td[i] = s[2 + 2 * i] >> 4;
        P.comp_ta[i] = s[2 + 2 * i] & 15;
      }
      if (s[1 + 2 * nc] != 0 || s[2 + 2 * nc] != 63 || s[3 + 2 * nc] != 0) { h.reason = JPEG_R_SCANS; return MOPA_ERR_UNSUPPORTED; }
      if (nc == 3 && !jfif) {
        const bool rgb_ids = P.comp_id[0] == 'R' && P.comp_id[1] == 'G' && P.comp_id[2] == 'B';
        if (adobe ? adobe_transform != 1 : rgb_ids) { h.reason = JPEG_R_COLORSPACE; return MOPA_ERR_UNSUPPORTED; }
      }
      for (int i = 0; i < nc; ++i) {
        if (P.comp_td[i] > 3 || P.comp_ta[i] > 3 || !P.dc[P.comp_td[i]].present || !P.ac[P.comp_ta[i]].present) return MOPA_ERR_DATA;
        if (!P.qt_present[P.comp_tq[i]]) return MOPA_ERR_DATA;
        memcpy(h.quant[i], P.qt[P.comp_tq[i]], 128);
      }
      h.mcus_x = (h.width + 8 * h.hs - 1) / (8 * h.hs);
      h.mcus_y = (h.height + 8 * h.vs - 1) / (8 * h.vs);
      int64_t off = JPEG_QUANT_BYTES;
      for (int i = 0; i < nc; ++i) {
        const int ch = i ? 1 : h.hs, cv = i ? 1 : h.vs;
        h.blocks_x[i] = h.mcus_x * ch;
        h.blocks_y[i] = h.mcus_y * cv;
        h.comp_w[i] = i ? (h.width + h.hs - 1) / h.hs : h.width;
        h.comp_h[i] = i ? (h.height + h.vs - 1) / h.vs : h.height;
        h.plane_off[i] = off;
        off += (int64_t)h.blocks_x[i] * h.blocks_y[i] * 128;
      }
      h.coeff_bytes = off;
      h.supported = 1;
      P.scan = d + p;
      return MOPA_OK;
    }
    // APPn, COM and every other marker with a length: skipped
  }
}

// Bit reader over the entropy-coded bytes: `acc` holds `n` real bits (right-aligned).  FF 00 is a stuffed FF; FF followed by anything
// else is a marker and stops the reader (`at_marker`), as does the end of the buffer: no bit is ever invented, a decoder that asks
// for more than is there gets `false`.
struct JpegBits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t acc;
  int n;
  bool stopped;

  inline void fill() {
    while (n <= 56 && !stopped) {
      if (p >= end) { stopped = true; break; }
      const uint8_t b = *p;
      if (b == 0xFF) {
        if (p + 1 >= end || p[1] != 0) { stopped = true; break; }
        p += 2;
      } else {
        ++p;
      }
      acc = acc << 8 | b;
      n += 8;
    }
  }
  // the next k <= 16 bits, zero-padded where the stream has fewer
  inline uint32_t peek(int k) {
    if (n < k) fill();
    return n >= k ? (uint32_t)(acc >> (n - k)) & ((1u << k) - 1) : (uint32_t)(acc << (k - n)) & ((1u << k) - 1);
  }
  inline bool skip(int k) {
    if (n < k) return false;
    n -= k;
    return true;
  }
  inline bool get(int k, uint32_t& v) {
    if (k == 0) { v = 0; return true; }
    if (n < k) { fill(); if (n < k) return false; }
    n -= k;
    v = (uint32_t)(acc >> n) & ((1u << k) - 1);
    return true;
  }
};

static inline bool jpeg_symbol(JpegBits& b, const JpegHuff& t, int& sym) {
  const uint32_t look = b.peek(16);
  const int l9 = t.look_len[look >> (16 - JPEG_LOOK)];
  if (l9) {
    sym = t.look_sym[look >> (16 - JPEG_LOOK)];
    return b.skip(l9);
  }
  for (int len = JPEG_LOOK + 1; len <= 16; ++len) {
    const int code = (int)(look >> (16 - len));
    if (code <= t.maxcode[len]) {
      sym = t.vals[(code + t.valoff[len]) & 255];
      return b.skip(len);
    }
  }
  return false;                                           // a code that is not in the table
}

static inline int jpeg_extend(uint32_t v, int s) { return s && v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// After the last MCU of an interval (or of the scan): drop the rest of the byte, skip fill bytes, take the marker.
static inline int jpeg_take_marker(JpegBits& b) {
  if (b.n >= 8) return -1;                                // whole unread bytes of entropy-coded data in front of the marker
  b.n = 0;
  b.acc = 0;
  const uint8_t* p = b.p;
  if (p >= b.end || *p != 0xFF) return -1;
  while (p < b.end && *p == 0xFF) ++p;
  if (p >= b.end) return -1;
  b.p = p + 1;
  b.stopped = false;
  return *p;
}

// coeff: the output buffer of `coeff_bytes` bytes (2-byte aligned).  The header is written too.
static inline int jpeg_entropy_decode(const uint8_t* d, int64_t n, JpegHeader* out_h, int16_t* coeff, int64_t coeff_bytes) {
  // ~12 KB of tables: on the stack, so that concurrent calls share nothing
  JpegParsed P;
  const int rc = jpeg_parse(d, n, P);
  if (out_h) *out_h = P.h;
  if (rc != MOPA_OK) return rc;
  const JpegHeader& h = P.h;
  if (!coeff || coeff_bytes < h.coeff_bytes || ((uintptr_t)coeff & 1)) return MOPA_ERR_ARG;
  memset(coeff, 0, JPEG_QUANT_BYTES);
  memcpy(coeff, h.quant, (size_t)h.ncomp * 128);
  JpegBits b = {P.scan, d + n, 0, 0, false};
  int pred[3] = {0, 0, 0};
  const int64_t total = (int64_t)h.mcus_x * h.mcus_y;
  int64_t to_restart = h.restart_interval ? h.restart_interval : total;
  int rst = 0, mx = 0, my = 0;
  for (int64_t mcu = 0; mcu < total; ++mcu) {
    if (to_restart == 0) {
      if (jpeg_take_marker(b) != 0xD0 + (rst & 7)) return MOPA_ERR_DATA;
      ++rst;
      pred[0] = pred[1] = pred[2] = 0;
      to_restart = h.restart_interval;
    }
    --to_restart;
    for (int c = 0; c < h.ncomp; ++c) {
      const JpegHuff& dc = P.dc[P.comp_td[c]];
      const JpegHuff& ac = P.ac[P.comp_ta[c]];
      const int ch = c ? 1 : h.hs, cv = c ? 1 : h.vs;
      int16_t* plane = (int16_t*)((char*)coeff + h.plane_off[c]);
      for (int v = 0; v < cv; ++v)
        for (int u = 0; u < ch; ++u) {
          // inside the plane: my * cv + v < blocks_y, mx * ch + u < blocks_x, and coeff_bytes >= the end of the last plane
          int16_t* blk = plane + ((int64_t)(my * cv + v) * h.blocks_x[c] + (mx * ch + u)) * 64;
          memset(blk, 0, 128);
          int s;
          uint32_t bits;
          if (!jpeg_symbol(b, dc, s) || !b.get(s, bits)) return MOPA_ERR_DATA;
          pred[c] += jpeg_extend(bits, s);
          blk[0] = (int16_t)(uint16_t)pred[c];
          pred[c] = (int16_t)(uint16_t)pred[c];           // kept in 16 bits: no input makes the sum overflow
          for (int k = 1; k < 64;) {
            int rs;
            if (!jpeg_symbol(b, ac, rs)) return MOPA_ERR_DATA;
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r != 15) break;
              k += 16;
              continue;
            }
            k += r;
            if (k > 63) return MOPA_ERR_DATA;             // a run past coefficient 63
            if (!b.get(s, bits)) return MOPA_ERR_DATA;
            blk[JPEG_NATURAL[k]] = (int16_t)jpeg_extend(bits, s);
            ++k;
          }
        }
    }
    if (++mx == h.mcus_x) { mx = 0; ++my; }
  }
  if (jpeg_take_marker(b) != 0xD9) return MOPA_ERR_DATA;   // no EOI behind the scan: truncated, or a further scan
  return MOPA_OK;
}
