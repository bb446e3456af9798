// PNG decoding, split at the filtered scanlines: inflate is a serial walk over untrusted bits and runs on the host (mopa_amd/pngdec.py,
// the standard library's zlib), undoing the per-row filters (None / Sub / Up / Average / Paeth) and the expansion to RGB are
// fixed-trip-count integer arithmetic over every byte and run here.  The result is the (H, W, 3) uint8 image that
// np.asarray(Image.open(...).convert("RGB")) returns, bit for bit, in the layout imageprep.prepare_batch reads.  The chain is stated in
// DESIGN.md section 4; yardstick tests/_png_reference.py, held against Pillow.
//
//   k_pn_decode  all images of a call in ONE launch, ONE workgroup per image (PN_WAVES waves), no workgroup ever waits for another.
//                Byte (y, i) needs (y, i - bpp), (y - 1, i) and (y - 1, i - bpp): the bpp bytes of a pixel are independent chains
//                (carried two to a register in its 16-bit halves, packed 16-bit arithmetic, the row's filter as lane constants: a step
//                has no branch), the rows form a wavefront with a skew of one pixel.  A pass covers
//                PN_ROWS rows, lane = row: at step t the lane of row r undoes pixel x = t - r.  Its left neighbour is its own last
//                result, the pixel above is the result of the lane above from the step before (one DPP move), the pixel above
//                left is what that move gave the step before.  Lane 0 of a wave has no lane above: wave w - 1 leaves the
//                results of its last row in a ring in LDS, and wave w runs PN_D phases (of PN_K steps, one workgroup barrier
//                pair each) behind it, so that what it reads was written before an earlier barrier.  The last row of a pass stays in
//                LDS (`carry`) for the first row of the next: unfiltered scanlines never reach memory.
//                Column blocks go through LDS so that the accesses to memory are row-contiguous: per phase and wave a tile of 64
//                rows x PN_K steps, the row of lane r moved by r pixels (what the lane needs in this phase).  Between two phases every
//                tile element is swapped by ONE lane, between LDS and its registers: the result it holds is taken out and the
//                filtered pixel of the coming phase, loaded a phase earlier, put in.  Then, before the steps of the phase and running
//                under them, the results are stored -- expanded to RGB in the store: grey replicated, alpha dropped, palette looked
//                up (a 256-entry table, zero past PLTE, so every index is inside) -- and the pixels of the phase after are loaded.
//                The steps themselves run in registers: a lane reads its PN_K pixels of the tile first and writes them back last.
//
// Every loop's trip count follows from W, H and bpp alone.  The filter byte only selects a predictor and is clamped to 0..4 (the
// host refused a stream with another one).  A corrupt scanline changes pixel values and nothing else.  Integer arithmetic, no
// atomics, no workspace.  Per-image pointers and geometry travel as kernel arguments (PN_MAXB images); the palettes are read from
// the device copy of the headers.
#include "common.h"
#include <string.h>

#define PN_MAXB 32                      // images per call
#define PN_MAX_SIDE 8192
#define PN_WAVES 8
#define PN_THREADS (64 * PN_WAVES)
#define PN_ROWS (64 * PN_WAVES)         // rows per pass
#define PN_K 32                         // steps per phase = columns per block
#define PN_D 3                          // phases a wave starts behind the wave above it; (PN_D - 1) * PN_K >= 63
#define PN_TP (PN_K + 1)                // tile row pitch in pixels: lanes of a wave on different banks
#define PN_RING 256                     // pixels of a wave's last row kept for the wave below; > (PN_D + 1) * PN_K - 64

static_assert((PN_D - 1) * PN_K >= 63, "a wave must read what the wave above wrote before an earlier barrier");
static_assert(PN_RING > (PN_D + 1) * PN_K - 64 && (PN_RING & (PN_RING - 1)) == 0, "ring too short");
static_assert(PN_WAVES >= 2, "the carry row is written behind where wave 0 reads it only with a wave in between");

// What a caller fills per image (mopa_amd/pngdec.py::Header).
struct PngHeader {
  int32_t width, height;
  int32_t color_type;                   // 0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGBA (8-bit samples)
  int32_t bpp;                          // bytes per pixel: 1, 3, 1, 2, 4
  uint32_t palette[256];                // R | G << 8 | B << 16; zero past the PLTE length
};

struct PnImg {
  const uint8_t* scan;                  // H rows of 1 + W * bpp bytes: the filter byte, then the filtered pixels
  uint8_t* dst;                         // (H, W, 3) uint8, rows `pitch` bytes apart
  int64_t pitch;
  int32_t W, H, ct, bpp;
};
struct PnArgs {
  PnImg im[PN_MAXB];
};

// A row's filter as lane constants, so that no step branches on it.  Bytes travel two to a register, in its 16-bit halves
// (PN_M picks them): the prediction is ((a & ma) + (b & mb)) >> sh for None / Sub / Up / Average and the Paeth choice under mp.
#define PN_M 0x00ff00ffu
struct PnFilter {
  uint32_t ma, mb, sh, mp;
};
__device__ __forceinline__ PnFilter pn_filter(int ft) {
  PnFilter f;
  f.ma = ft == 1 || ft == 3 ? PN_M : 0;
  f.mb = ft == 2 || ft == 3 ? PN_M : 0;
  f.sh = ft == 3;
  f.mp = ft == 4 ? 0xffffffffu : 0;
  return f;
}

typedef short pn_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pn_s2 pn_v(uint32_t x) { return __builtin_bit_cast(pn_s2, x); }
__device__ __forceinline__ uint32_t pn_u(pn_s2 x) { return __builtin_bit_cast(uint32_t, x); }

// Two bytes of a pixel at once: `raw` the filtered bytes, a / b / c the unfiltered bytes left / above / above left, each byte in a
// 16-bit half (values 0..255, so sums and differences stay inside the half).  Packed 16-bit arithmetic, no compare, no branch.
template <bool PAETH>
__device__ __forceinline__ uint32_t pn_unfilter2(uint32_t raw, uint32_t a, uint32_t b, uint32_t c, const PnFilter& f) {
  uint32_t pred = (((a & f.ma) + (b & f.mb)) >> f.sh) & PN_M;
  if (PAETH) {
    const pn_s2 p = pn_v(b) - pn_v(c), q = pn_v(a) - pn_v(c), s = p + q;  // pa = |b - c|, pb = |a - c|, pc = |a + b - 2 c|
    const pn_s2 pa = __builtin_elementwise_max(p, -p), pb = __builtin_elementwise_max(q, -q), pc = __builtin_elementwise_max(s, -s);
    const uint32_t not_a = pn_u(((pb - pa) | (pc - pa)) >> 15);            // all ones where pa > pb or pa > pc
    const uint32_t take_c = pn_u((pc - pb) >> 15);                         // all ones where pb > pc
    const uint32_t inner = (take_c & c) | (~take_c & b);
    const uint32_t pth = (not_a & inner) | (~not_a & a);                   // a if pa <= pb and pa <= pc, else b if pb <= pc, else c
    pred |= pth & f.mp;                                                    // ma = mb = 0 in a Paeth row
  }
  return (raw + pred) & PN_M;
}

__device__ __forceinline__ uint32_t pn_rgb(uint32_t v, int ct, const uint32_t* pal) {
  if (ct == 2 || ct == 6) return v & 0xffffffu;
  if (ct == 3) return pal[v & 255];
  return (v & 255) * 0x010101u;
}

// The lane above's value of `v` (lane 0: 0): one DPP move, no LDS.
__device__ __forceinline__ uint32_t pn_from_above(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// The filtered pixel at p (BPP bytes) as one register: one load of the pixel's width (3 bytes: the four from the byte in front, which
// is the filter byte or the pixel to the left and always inside the buffer).
template <int BPP>
__device__ __forceinline__ uint32_t pn_load(const uint8_t* __restrict__ p) {
  if (BPP == 1) return p[0];
  if (BPP == 2) {
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
  }
  uint32_t v;
  __builtin_memcpy(&v, BPP == 3 ? p - 1 : p, 4);
  return BPP == 3 ? v >> 8 : v;
}

// The PN_K steps of one phase of one wave, in registers: the lane's PN_K filtered pixels are read from its tile row first and its
// results written back last; lane l < PN_K fetches the pixel above lane 0 for step l beforehand and keeps lane 63's result of step l
// for the wave below, so that the steps themselves touch no memory.
template <int BPP, bool PAETH>
__device__ __forceinline__ void pn_steps(uint32_t* __restrict__ row, const uint32_t* __restrict__ above, bool above_is_carry,
                                         uint32_t* __restrict__ below, bool below_is_carry, int t0, int lane, int W, const PnFilter& f,
                                         uint32_t (&cur)[2], uint32_t (&up)[2]) {
  constexpr int NH = BPP == 1 ? 1 : 2;                                     // registers of a pixel: bytes 0 and 2, bytes 1 and 3
  uint32_t px[PN_K];
#pragma unroll
  for (int s = 0; s < PN_K; ++s) px[s] = row[s];
  const int xa = t0 + (lane & (PN_K - 1));                                 // lane 0's column at step lane
  const uint32_t abv = above_is_carry ? above[xa < W ? xa : W - 1] : above[xa & (PN_RING - 1)];
  uint32_t bel = 0;
#pragma unroll
  for (int s = 0; s < PN_K; ++s) {
    const int x = t0 + s - lane;
    const bool inside = x >= 0 && x < W;
    const uint32_t a0 = (uint32_t)__builtin_amdgcn_readlane((int)abv, s);
    uint32_t out = 0;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const uint32_t upleft = up[h];
      up[h] = pn_from_above(cur[h]);                                       // the lane above, one step ago: the same column
      up[h] = lane == 0 ? (a0 >> (8 * h)) & PN_M : up[h];
      const uint32_t v = pn_unfilter2<PAETH>((px[s] >> (8 * h)) & PN_M, cur[h], up[h], upleft, f);
      cur[h] = inside ? v : 0;                                             // left of the row: zeros
      out |= cur[h] << (8 * h);
    }
    px[s] = out;
    const uint32_t last = (uint32_t)__builtin_amdgcn_readlane((int)out, 63);
    bel = lane == s ? last : bel;
  }
#pragma unroll
  for (int s = 0; s < PN_K; ++s) row[s] = px[s];
  const int xb = t0 + lane - 63;                                           // lane 63's column at step lane
  if (lane < PN_K && xb >= 0 && xb < W) below[below_is_carry ? xb : xb & (PN_RING - 1)] = bel;
}

template <int BPP>
__device__ __forceinline__ void pn_image(const PnImg& im, uint32_t* __restrict__ tile, uint32_t* __restrict__ carry, uint32_t* __restrict__ ring,
                                         const uint32_t* __restrict__ pal) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int W = im.W, H = im.H, ct = im.ct;
  const int64_t rowb = 1 + (int64_t)W * BPP;
  const uint8_t* __restrict__ scan = im.scan;
  uint8_t* __restrict__ dst = im.dst;
  const int nq = (W + 63 + PN_K - 1) / PN_K;                // phases a wave needs for its 64 skewed rows
  uint32_t* __restrict__ mine = tile + w * 64 * PN_TP;      // this wave's tile
  const uint32_t* __restrict__ above = w == 0 ? carry : ring + (w - 1) * PN_RING;
  uint32_t* __restrict__ below = w == PN_WAVES - 1 ? carry : ring + w * PN_RING;
  // the tile elements this lane moves between memory and LDS: element i is step s0 of row 2 i + r0
  const int s0 = lane & (PN_K - 1), r0 = lane / PN_K;
  static_assert(PN_K == 32, "64 lanes cover two tile rows per element index");
  for (int i = threadIdx.x; i < W; i += PN_THREADS) carry[i] = 0;          // the row above the image
  for (int y0 = 0; y0 < H; y0 += PN_ROWS) {                                // a pass
    const int rows = H - y0 < PN_ROWS ? H - y0 : PN_ROWS;
    const int nwa = (rows + 63) >> 6;                                      // waves with rows in this pass
    const int Plast = nq + PN_D * (nwa - 1);
    const int yw = y0 + 64 * w;                                            // the wave's first row
    int ft = 0;
    if (yw + lane < H) {
      ft = scan[(int64_t)(yw + lane) * rowb];
      ft = ft > 4 ? 4 : ft;
    }
    const bool paeth = __any(ft == 4);
    const PnFilter f = pn_filter(ft);
    uint32_t cur[2] = {0, 0}, up[2] = {0, 0};
    uint32_t inv[PN_K], outv[PN_K];                                        // filtered pixels coming in, results going out
    for (int P = -1; P <= Plast; ++P) {
      const int q = P - PN_D * w;                                          // this wave's phase
      const bool mover = w < nwa && q >= -1 && q <= nq;
      __syncthreads();
      if (mover && q >= 0) {                                               // LDS only: the results of phase q - 1 out, the pixels of phase q in
#pragma unroll
        for (int i = 0; i < PN_K; ++i) {
          const int slot = (2 * i + r0) * PN_TP + s0;
          if (q >= 1) outv[i] = mine[slot];
          if (q < nq) mine[slot] = inv[i];
        }
      }
      __syncthreads();
      if (mover) {                                                         // memory only, under the steps below
        if (q >= 1) {
          uint8_t* o = dst + (int64_t)(yw + r0) * im.pitch + (int64_t)((q - 1) * PN_K + s0 - r0) * 3;   // element 0; 2 rows down, 2 pixels left each
#pragma unroll
          for (int i = 0; i < PN_K; ++i, o += 2 * im.pitch - 6) {
            const int r = 2 * i + r0, yy = yw + r, x = (q - 1) * PN_K + s0 - r;
            if (yy < H && x >= 0 && x < W) {
              const uint32_t v = pn_rgb(outv[i], ct, pal);
              o[0] = (uint8_t)v;
              o[1] = (uint8_t)(v >> 8);
              o[2] = (uint8_t)(v >> 16);
            }
          }
        }
        if (q + 1 < nq) {
          const uint8_t* p = scan + (int64_t)(yw + r0) * rowb + 1 + (int64_t)((q + 1) * PN_K + s0 - r0) * BPP;
#pragma unroll
          for (int i = 0; i < PN_K; ++i, p += 2 * rowb - 2 * BPP) {
            const int r = 2 * i + r0, yy = yw + r, x = (q + 1) * PN_K + s0 - r;
            inv[i] = yy < H && x >= 0 && x < W ? pn_load<BPP>(p) : 0;
          }
        }
      }
      if (w < nwa && q >= 0 && q < nq) {
        if (paeth) pn_steps<BPP, true>(mine + lane * PN_TP, above, w == 0, below, w == PN_WAVES - 1, q * PN_K, lane, W, f, cur, up);
        else pn_steps<BPP, false>(mine + lane * PN_TP, above, w == 0, below, w == PN_WAVES - 1, q * PN_K, lane, W, f, cur, up);
      }
    }
  }
}

__global__ __launch_bounds__(PN_THREADS) void k_pn_decode(const PnArgs a, const PngHeader* __restrict__ headers) {
  __shared__ uint32_t tile[PN_WAVES * 64 * PN_TP];
  __shared__ uint32_t carry[PN_MAX_SIDE];
  __shared__ uint32_t ring[PN_WAVES * PN_RING];
  __shared__ uint32_t pal[256];
  const PnImg& im = a.im[blockIdx.x];
  if (threadIdx.x < 256) pal[threadIdx.x] = im.ct == 3 ? headers[blockIdx.x].palette[threadIdx.x] : 0;
  for (int i = threadIdx.x; i < PN_WAVES * PN_RING; i += PN_THREADS) ring[i] = 0;
  __syncthreads();
  switch (im.bpp) {                                                        // uniform over the workgroup
    case 1: pn_image<1>(im, tile, carry, ring, pal); break;
    case 2: pn_image<2>(im, tile, carry, ring, pal); break;
    case 3: pn_image<3>(im, tile, carry, ring, pal); break;
    default: pn_image<4>(im, tile, carry, ring, pal); break;
  }
}

// ------------------------------------------------------------------------------------------ host side
static int pn_bpp(int ct) { return ct == 0 ? 1 : ct == 2 ? 3 : ct == 3 ? 1 : ct == 4 ? 2 : ct == 6 ? 4 : 0; }

MOPA_API int mopa_png_max_images(void) { return PN_MAXB; }
MOPA_API int mopa_png_header_bytes(void) { return (int)sizeof(PngHeader); }
// The kernel's tiling: rows of a pass (a wave takes 64 of them), columns of a block.
MOPA_API int mopa_png_rows_per_pass(void) { return PN_ROWS; }
MOPA_API int mopa_png_block_cols(void) { return PN_K; }

// The device half for B <= mopa_png_max_images() images in one launch, no workspace, no read-back.  scan_ptrs_host[b]: DEVICE address of
// image b's filtered scanlines, scan_bytes_host[b] == H * (1 + W * bpp) bytes; headers_host: the B headers (PngHeader); headers: a DEVICE
// copy of the same B headers (the kernel reads the palettes there and nothing else); out_ptrs_host[b]: DEVICE address of the (H, W, 3)
// uint8 destination whose rows are pitch_host[b] >= 3 W bytes apart.  What the kernel's indexing rests on is checked again here.
MOPA_API int mopa_png_decode_batch(const void* const* scan_ptrs_host, const int64_t* scan_bytes_host, const void* headers_host, const void* headers,
                                   int32_t B, void* const* out_ptrs_host, const int64_t* pitch_host, void* stream) {
  if (!scan_ptrs_host || !scan_bytes_host || !headers_host || !headers || !out_ptrs_host || !pitch_host || B < 1 || B > PN_MAXB) return MOPA_ERR_ARG;
  PnArgs a = {};
  for (int b = 0; b < B; ++b) {
    PngHeader h;
    memcpy(&h, (const char*)headers_host + (size_t)b * sizeof(PngHeader), sizeof(h));
    if (h.width < 1 || h.height < 1 || h.width > PN_MAX_SIDE || h.height > PN_MAX_SIDE) return MOPA_ERR_ARG;
    if (h.bpp < 1 || h.bpp > 4 || h.bpp != pn_bpp(h.color_type)) return MOPA_ERR_ARG;
    if (!scan_ptrs_host[b] || scan_bytes_host[b] != (int64_t)h.height * (1 + (int64_t)h.width * h.bpp)) return MOPA_ERR_ARG;
    if (!out_ptrs_host[b] || pitch_host[b] < (int64_t)3 * h.width) return MOPA_ERR_ARG;
    PnImg& im = a.im[b];
    im.scan = (const uint8_t*)scan_ptrs_host[b];
    im.dst = (uint8_t*)out_ptrs_host[b];
    im.pitch = pitch_host[b];
    im.W = h.width; im.H = h.height; im.ct = h.color_type; im.bpp = h.bpp;
  }
  k_pn_decode<<<(unsigned)B, PN_THREADS, 0, (hipStream_t)stream>>>(a, (const PngHeader*)headers);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
