// JPEG decoding, split at the quantised coefficients: the Huffman stage is a serial walk over untrusted bits and runs on the host
// (jpeg_entropy.h, plain C++), everything behind it is fixed-trip-count arithmetic over every pixel and runs here.  The result is the
// (H, W, 3) uint8 image that Pillow (libjpeg-turbo with its default settings) returns, bit for bit, in the layout
// imageprep.prepare_batch reads.  The chain is stated in DESIGN.md section 4; yardstick tests/_jpeg_reference.py, held against Pillow.
//
//   k_jd_decode  all images of a call in ONE launch, a workgroup per tile of 14 x 2 MCUs.  Phase 1, one 8 x 8 block per thread (64
//                coefficients in registers): dequantisation, libjpeg's accurate integer inverse DCT ("islow": 13-bit constants,
//                PASS1_BITS = 2, columns then rows, DESCALE rounding, int32), + 128, clamped to 8 bits, for the tile's luma blocks and
//                its chroma blocks plus the ring of chroma blocks the upsampling filter reaches into, into LDS (the component planes
//                never reach memory).  Phase 2, four adjacent pixels per thread: libjpeg-turbo's "fancy" chroma upsampling (triangle
//                filters; the far sample clamped into the component's REAL downsampled size, which is the library's edge rule;
//                planes of at most two real columns are replicated, as the library does), YCbCr -> RGB in 16-bit fixed point, and
//                12-byte stores into the destination where the row position is 4-byte aligned, bytes otherwise.
//                The two-kernel form with the planes in a workspace measured 5 % slower (profiles/r27_jpegdec.md) and is not here.
//
// No loop's trip count depends on image data: every bound comes from the header, which the host validated (jd_geometry recomputes
// the grid from width, height, component count and sampling and ignores the derived fields).  A corrupt coefficient changes pixel
// values and nothing else.  Per-image pointers and geometry travel as kernel arguments (JD_MAXB images).
#include "common.h"
#include "jpeg_entropy.h"

#define JD_MAXB 32             // images per call

struct JdImg {
  const int16_t* coeff;        // the image's coefficient buffer: quantisation tables, then the planes (jpeg_entropy.h)
  uint8_t* dst;                // (H, W, 3) uint8, rows `pitch` bytes apart
  int64_t pitch;
  int32_t W, H, mx, my;        // mx, my: MCUs per row / column
  int32_t hs, vs, nc;          // luma sampling, components
  int32_t wg0;                 // first workgroup (tile) of the image
};
struct JdArgs {
  JdImg im[JD_MAXB];
};

__device__ __forceinline__ int jd_clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// ------------------------------------------------------------------------------------------ inverse DCT
#define JD_DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))
// one 8-point pass (jidctint.c's even / odd decomposition)
__device__ __forceinline__ void jd_idct8(const int (&x)[8], int (&o)[8], const int shift) {
  int z2 = x[2], z3 = x[6];
  int z1 = (z2 + z3) * 4433;
  int tmp2 = z1 + z3 * (-15137), tmp3 = z1 + z2 * 6270;
  int tmp0 = (x[0] + x[4]) << 13, tmp1 = (x[0] - x[4]) << 13;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * 9633;
  tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  o[0] = JD_DESCALE(tmp10 + tmp3, shift); o[7] = JD_DESCALE(tmp10 - tmp3, shift);
  o[1] = JD_DESCALE(tmp11 + tmp2, shift); o[6] = JD_DESCALE(tmp11 - tmp2, shift);
  o[2] = JD_DESCALE(tmp12 + tmp1, shift); o[5] = JD_DESCALE(tmp12 - tmp1, shift);
  o[3] = JD_DESCALE(tmp13 + tmp0, shift); o[4] = JD_DESCALE(tmp13 - tmp0, shift);
}

__device__ __forceinline__ int jd_segment(const JdArgs& a, int B, int wg) {
  int s = 0;
  while (s + 1 < B && a.im[s + 1].wg0 <= wg) ++s;
  return s;
}

// ------------------------------------------------------------------------------------------ upsampling, colour, store
__device__ __forceinline__ uint32_t jd_rgb(int y, int cb, int cr) {
  cb -= 128;
  cr -= 128;
  const int r = jd_clamp8(y + ((91881 * cr + 32768) >> 16));
  const int g = jd_clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  const int b = jd_clamp8(y + ((116130 * cb + 32768) >> 16));
  return (uint32_t)r | (uint32_t)g << 8 | (uint32_t)b << 16;
}

// The four chroma samples of one component at pixels x0 .. x0 + 3 of row y (x0 a multiple of 4); hs == 2.  p: where sample (0, 0) of
// the component would lie (the kernel passes its LDS tile moved back by the tile's origin), rows cpitch apart.
__device__ __forceinline__ int4 jd_chroma4(const uint8_t* __restrict__ p, int cpitch, int dw, int dh, int vs, int x0, int y) {
  const int i0 = x0 >> 1;                                  // <= dw - 1: x0 <= W - 1
  const int n1 = i0 + 1 < dw ? i0 + 1 : dw - 1;
  const int cm = i0 > 0 ? i0 - 1 : 0, c2 = i0 + 2 < dw ? i0 + 2 : dw - 1;
  const int cy = vs == 2 ? y >> 1 : y;
  const uint8_t* __restrict__ near = p + (int64_t)cy * cpitch;
  int sm = near[cm], s0 = near[i0], s1 = near[n1], s2 = near[c2];
  if (dw <= 2) return make_int4(s0, s0, s1, s1);           // the library replicates planes of at most two columns
  int sh = 2, even = 1, odd = 2;
  if (vs == 2) {
    const int fy = (y & 1) ? (cy + 1 < dh ? cy + 1 : dh - 1) : (cy > 0 ? cy - 1 : 0);
    const uint8_t* __restrict__ far = p + (int64_t)fy * cpitch;
    sm = 3 * sm + far[cm]; s0 = 3 * s0 + far[i0]; s1 = 3 * s1 + far[n1]; s2 = 3 * s2 + far[c2];
    sh = 4; even = 8; odd = 7;
  }
  return make_int4((3 * s0 + sm + even) >> sh, (3 * s0 + s1 + odd) >> sh, (3 * s1 + s0 + even) >> sh, (3 * s1 + s2 + odd) >> sh);
}

// ------------------------------------------------------------------------------------------ the kernel
// A workgroup makes a tile of JF_TX x JF_TY MCUs.  Phase 1: one block per thread -- the tile's luma blocks and its chroma blocks with
// a halo of one block where the upsampling filter reaches over (left / right for hs == 2, above / below for vs == 2) -- into LDS.
// At most 14 * 2 * 4 + 2 * 16 * 4 = 240 blocks (4:2:0).  Phase 2: the tile's pixels from LDS.  Blocks outside the image's grid are
// not made and never read: the filter's far sample is clamped into the component's real size.
#define JF_TX 14
#define JF_TY 2
#define JF_LW (JF_TX * 2 * 8 + 16)          // LDS row pitch of the luma tile (bytes)
#define JF_CW ((JF_TX + 2) * 8 + 16)        // ... of a chroma tile
__global__ __launch_bounds__(256) void k_jd_decode(const JdArgs a, int B) {
  __shared__ uint16_t q[3 * 64];
  __shared__ __attribute__((aligned(16))) uint8_t ly[JF_TY * 2 * 8 * JF_LW];
  __shared__ __attribute__((aligned(16))) uint8_t lc[2][(JF_TY + 2) * 8 * JF_CW];
  const int s = jd_segment(a, B, blockIdx.x);
  const JdImg& im = a.im[s];
  if (threadIdx.x < 3 * 64) q[threadIdx.x] = ((const uint16_t*)im.coeff)[threadIdx.x];
  __syncthreads();
  const int hs = im.hs, vs = im.vs, nc = im.nc;
  const int tiles_x = (im.mx + JF_TX - 1) / JF_TX;
  const int tile = blockIdx.x - im.wg0;
  const int ty0 = tile / tiles_x * JF_TY, tx0 = (tile - tile / tiles_x * tiles_x) * JF_TX;      // first MCU of the tile
  const int hx = hs == 2, hy = vs == 2;
  const int lbw = JF_TX * hs, lbh = JF_TY * vs, nL = lbw * lbh;                                  // luma blocks of the tile
  const int cbw = JF_TX + 2 * hx, cbh = JF_TY + 2 * hy, nCt = nc == 3 ? cbw * cbh : 0;           // chroma blocks of the tile, per component
  const int nY = im.mx * hs * im.my * vs, nC = im.mx * im.my;
  {
    const int t = threadIdx.x;
    int c = -1, bx = 0, by = 0, lx = 0, lyy = 0;
    if (t < nL) {
      c = 0; lyy = t / lbw; lx = t - lyy * lbw; bx = tx0 * hs + lx; by = ty0 * vs + lyy;
      if (bx >= im.mx * hs || by >= im.my * vs) c = -1;
    } else if (t < nL + 2 * nCt) {
      const int u = t - nL;
      c = 1 + u / nCt;
      const int v = u - (c - 1) * nCt;
      lyy = v / cbw; lx = v - lyy * cbw; bx = tx0 - hx + lx; by = ty0 - hy + lyy;
      if (bx < 0 || by < 0 || bx >= im.mx || by >= im.my) c = -1;
    }
    if (c >= 0) {
      const int bxc = c ? im.mx : im.mx * hs;
      const int64_t i = (c == 0 ? 0 : c == 1 ? nY : nY + nC) + (int64_t)by * bxc + bx;
      const uint4* src = (const uint4*)(im.coeff + JPEG_QUANT_BYTES / 2 + i * 64);
      const uint16_t* qc = q + 64 * c;
      uint8_t* out = c == 0 ? ly + lyy * 8 * JF_LW + lx * 8 : lc[c - 1] + lyy * 8 * JF_CW + lx * 8;
      const int pitch = c == 0 ? JF_LW : JF_CW;
      int w[8][8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const uint4 v = src[r];
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) w[r][k] = (int)(int16_t)(u[k >> 1] >> (16 * (k & 1))) * (int)qc[8 * r + k];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        int x[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = w[r][k];
        jd_idct8(x, o, 13 - 2);
#pragma unroll
        for (int r = 0; r < 8; ++r) w[r][k] = o[r];
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        int o[8];
        jd_idct8(w[r], o, 13 + 2 + 3);
        uint2 v = make_uint2(0, 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v.x |= (uint32_t)jd_clamp8(o[k] + 128) << (8 * k);
          v.y |= (uint32_t)jd_clamp8(o[k + 4] + 128) << (8 * k);
        }
        *(uint2*)(out + r * pitch) = v;
      }
    }
  }
  __syncthreads();
  const int W = im.W, H = im.H;
  const int TW = lbw * 8, TH = lbh * 8, G = TW / 4;
  const int px0 = tx0 * hs * 8, py0 = ty0 * vs * 8;          // the tile's first pixel
  const int cx0 = (tx0 - hx) * 8, cy0 = (ty0 - hy) * 8;      // the chroma sample at LDS column / row 0
  const int dw = hs == 2 ? (W + 1) >> 1 : W, dh = vs == 2 ? (H + 1) >> 1 : H;
  for (int it = threadIdx.x; it < TH * G; it += 256) {       // trip count from the tile's geometry
    const int yl = it / G, xl = (it - yl * G) * 4;
    const int x0 = px0 + xl, y = py0 + yl;
    if (x0 >= W || y >= H) continue;
    const int npx = W - x0 < 4 ? W - x0 : 4;
    const uint32_t yw = *(const uint32_t*)(ly + yl * JF_LW + xl);
    uint32_t px[4];
    if (nc == 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) px[k] = (yw >> (8 * k) & 255) * 0x010101u;
    } else {
      int4 cb, cr;
      if (hs == 1) {
        const uint32_t bw = *(const uint32_t*)(lc[0] + (y - cy0) * JF_CW + (x0 - cx0)), rw = *(const uint32_t*)(lc[1] + (y - cy0) * JF_CW + (x0 - cx0));
        cb = make_int4(bw & 255, bw >> 8 & 255, bw >> 16 & 255, bw >> 24);
        cr = make_int4(rw & 255, rw >> 8 & 255, rw >> 16 & 255, rw >> 24);
      } else {
        // jd_chroma4 with the plane's origin moved to the LDS tile: p + cy * pitch + col  ==  tile + (cy - cy0) * pitch + (col - cx0)
        cb = jd_chroma4(lc[0] - (int64_t)cy0 * JF_CW - cx0, JF_CW, dw, dh, vs, x0, y);
        cr = jd_chroma4(lc[1] - (int64_t)cy0 * JF_CW - cx0, JF_CW, dw, dh, vs, x0, y);
      }
      px[0] = jd_rgb((int)(yw & 255), cb.x, cr.x);
      px[1] = jd_rgb((int)(yw >> 8 & 255), cb.y, cr.y);
      px[2] = jd_rgb((int)(yw >> 16 & 255), cb.z, cr.z);
      px[3] = jd_rgb((int)(yw >> 24), cb.w, cr.w);
    }
    uint8_t* __restrict__ out = im.dst + (int64_t)y * im.pitch + (int64_t)x0 * 3;
    if (npx == 4 && ((uintptr_t)out & 3) == 0) {
      uint32_t* o = (uint32_t*)out;
      o[0] = px[0] | px[1] << 24;
      o[1] = px[1] >> 8 | px[2] << 16;
      o[2] = px[2] >> 16 | px[3] << 8;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < npx) {
          out[3 * k] = (uint8_t)px[k];
          out[3 * k + 1] = (uint8_t)(px[k] >> 8);
          out[3 * k + 2] = (uint8_t)(px[k] >> 16);
        }
    }
  }
}

// ------------------------------------------------------------------------------------------ host side
struct JdGeom {
  int W, H, nc, hs, vs, mx, my;
  int64_t blocks, coeff_bytes;
};
// The grid of an image from the five numbers that define it; false if they are not a supported image.
static bool jd_geometry(const JpegHeader& h, JdGeom& g) {
  if (h.width < 1 || h.height < 1 || h.width > JPEG_MAX_SIDE || h.height > JPEG_MAX_SIDE) return false;
  if (h.ncomp != 1 && h.ncomp != 3) return false;
  if (!((h.hs == 1 && h.vs == 1) || (h.ncomp == 3 && h.hs == 2 && (h.vs == 1 || h.vs == 2)))) return false;
  g.W = h.width; g.H = h.height; g.nc = h.ncomp; g.hs = h.hs; g.vs = h.vs;
  g.mx = (g.W + 8 * g.hs - 1) / (8 * g.hs);
  g.my = (g.H + 8 * g.vs - 1) / (8 * g.vs);
  g.blocks = (int64_t)g.mx * g.my * (g.hs * g.vs + (g.nc == 3 ? 2 : 0));
  g.coeff_bytes = JPEG_QUANT_BYTES + g.blocks * 128;
  return true;
}

MOPA_API int mopa_jpeg_max_images(void) { return JD_MAXB; }
MOPA_API int mopa_jpeg_header_bytes(void) { return (int)sizeof(JpegHeader); }

// The geometry of a stream and whether it is supported, from its markers alone: fills *header_host (a JpegHeader, jpeg_entropy.h)
// and touches nothing else.  MOPA_OK: supported; MOPA_ERR_UNSUPPORTED: header.reason says why; MOPA_ERR_DATA: malformed.  No GPU.
MOPA_API int mopa_jpeg_info(const uint8_t* data_host, void* header_host, int64_t nbytes) {
  if (!data_host || !header_host || nbytes < 0) return MOPA_ERR_ARG;
  JpegParsed P;
  const int rc = jpeg_parse(data_host, nbytes, P);
  memcpy(header_host, &P.h, sizeof(JpegHeader));
  return rc;
}

// Bytes of the coefficient buffer of the image a header describes (0 if it describes none).  No GPU.
MOPA_API size_t mopa_jpeg_coeff_bytes(const void* header_host) {
  JdGeom g;
  JpegHeader h;
  if (!header_host) return 0;
  memcpy(&h, header_host, sizeof(h));
  return jd_geometry(h, g) ? (size_t)g.coeff_bytes : 0;
}

// The host half: the stream's quantised coefficients into coeff_host (coeff_bytes bytes, 2-byte aligned; pinned memory lets the
// upload run asynchronously), its header into *header_host.  MOPA_ERR_UNSUPPORTED before anything is written to coeff_host,
// MOPA_ERR_DATA for a malformed stream (coeff_host then holds a partial result), MOPA_ERR_ARG for a buffer that is too small.  No GPU.
MOPA_API int mopa_jpeg_entropy_decode(const uint8_t* data_host, void* header_host, void* coeff_host, int64_t nbytes, int64_t coeff_bytes) {
  if (!data_host || !header_host || nbytes < 0) return MOPA_ERR_ARG;
  JpegHeader h;
  const int rc = jpeg_entropy_decode(data_host, nbytes, &h, (int16_t*)coeff_host, coeff_bytes);
  memcpy(header_host, &h, sizeof(h));
  return rc;
}

// The device half for B <= mopa_jpeg_max_images() images in one launch, no workspace, no read-back.  coeff_ptrs_host[b]: DEVICE address
// of image b's coefficient buffer (16-byte aligned, coeff_bytes_host[b] bytes: what mopa_jpeg_entropy_decode wrote), headers_host: the B
// headers, dst_ptrs_host[b]: DEVICE address of the (H, W, 3) uint8 destination whose rows are pitch_host[b] >= 3 W bytes apart.
MOPA_API int mopa_jpeg_decode_batch(const void* const* coeff_ptrs_host, const int64_t* coeff_bytes_host, const void* headers_host, int32_t B,
                                    void* const* dst_ptrs_host, const int64_t* pitch_host, void* stream) {
  if (!coeff_ptrs_host || !coeff_bytes_host || !headers_host || !dst_ptrs_host || !pitch_host || B < 1 || B > JD_MAXB) return MOPA_ERR_ARG;
  JdArgs a = {};
  int64_t wg = 0;
  for (int b = 0; b < B; ++b) {
    JpegHeader h;
    JdGeom g;
    memcpy(&h, (const char*)headers_host + (size_t)b * sizeof(JpegHeader), sizeof(h));
    if (!jd_geometry(h, g)) return MOPA_ERR_ARG;
    if (!coeff_ptrs_host[b] || ((uintptr_t)coeff_ptrs_host[b] & 15) || coeff_bytes_host[b] < g.coeff_bytes) return MOPA_ERR_ARG;
    if (!dst_ptrs_host[b] || pitch_host[b] < (int64_t)3 * g.W) return MOPA_ERR_ARG;
    JdImg& im = a.im[b];
    im.coeff = (const int16_t*)coeff_ptrs_host[b];
    im.dst = (uint8_t*)dst_ptrs_host[b];
    im.pitch = pitch_host[b];
    im.W = g.W; im.H = g.H; im.mx = g.mx; im.my = g.my; im.hs = g.hs; im.vs = g.vs; im.nc = g.nc;
    im.wg0 = (int32_t)wg;
    wg += cdiv64(g.mx, JF_TX) * cdiv64(g.my, JF_TY);                   // <= 74 * 512 per image
  }
  k_jd_decode<<<(unsigned)wg, 256, 0, (hipStream_t)stream>>>(a, B);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
