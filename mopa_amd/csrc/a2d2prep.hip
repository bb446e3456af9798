// A2D2's offline preprocessing of a frame on the device (mopa/data/a2d2/preprocess.py:26-44,96-141): the undistortion of the
// camera image and of the colour-coded label image (cv2.undistort of a Telecam = an inverse map built once per camera, then a
// bilinear remap with a constant 0 border), the label image read at every lidar point's [row, col], the RGB code -> class index
// lookup of class_list.json, and the float32 casts of points, reflectance / 255 and points_img.
//
//   k_a2_map     one thread per destination pixel: the float64 chain of DESIGN.md section 4 -> OpenCV's fixed-point map layout,
//                xy (H, W, 2) int16 [sx, sy] (CV_16SC2) and frac (H, W) uint16 = fy5 * 32 + fx5 (CV_16UC1, INTER_BITS = 5).
//                Depends on the camera only: the binding builds it once and keeps it.
//   k_a2_remap   all planes of a call (the B images and, on request, the B label images) in one launch: grid over plane groups x (rows x
//                column groups), the map entries of a thread serve up to four planes; a thread makes PW adjacent destination pixels and stores whole dwords where its 3 PW bytes are
//                4-byte aligned (every group of a 1920-pixel row is), bytes otherwise (any width, any alignment, 1-pixel rows).
//                No LDS: the map is smooth, so the 2 x 2 gathers of neighbouring threads fall into the same lines.
//   k_a2_points  one thread per lidar point, all frames in one launch (a frame is cut into blocks of A2_ROWS points; per-frame
//                pointers and the block table of segbatch.h travel as kernel arguments).  The label pixel is the
//                remapped label image at (r, c) computed on the spot by the same a2_pixel as k_a2_remap -- the same bytes, and
//                only N ~ 1e4 of 2.3 M label pixels are ever made.
//
// Arithmetic: the map is float64 with every operation rounded once: plain operators under `#pragma clang fp contract(off)` (this
// toolchain's __dmul_rn / __dadd_rn / __dsub_rn are plain operators inside a header that allows contraction, so spelling the chain with
// them lets the compiler fuse it; the only fmas left in k_a2_map are inside the expansion of the three divisions, which are
// correctly rounded), rint rounds half to even; the remap is integer: ((32-fx)(32-fy) p00 + fx (32-fy) p01 + (32-fx) fy p10 +
// fx fy p11 + 512) >> 10, which is cv2.remap(INTER_LINEAR)'s 15-bit table form divided through by 32.  No float atomics; the one
// counter (points outside the label image, per frame) is an integer; results are deterministic.
#include "common.h"
#include "segbatch.h"
#include <limits.h>

#pragma clang fp contract(off)

#define A2_MAXB 32             // frames per point-kernel call
#define A2_MAXP 64             // planes per remap call
#define A2_ROWS 256            // lidar points per block
#define A2_PW 4                // destination pixels per thread of the remap (profiles/r26_a2d2prep.md: measured against 8)
#define A2_PLANES 4            // planes a remap thread walks with one read of its map entries
#define A2_MAXK 256            // rows of the colour table (LDS)
#define A2_MAXSIDE 32767       // image sides: a saturated int16 source coordinate must lie outside the source

struct A2Cam {
  double fx, fy, cx, cy;       // CamMatrixOriginal: the distorted source
  double nfx, nfy, ncx, ncy;   // CamMatrix: the undistorted destination
  double k1, k2, p1, p2, k3, k4, k5, k6;
};
struct A2Planes {
  const uint8_t* src[A2_MAXP]; // (H, W, 3) uint8
  uint8_t* dst[A2_MAXP];
};
struct A2Frames {
  const void* points[A2_MAXB];      // (n, 3) float64 / float32
  const double* row[A2_MAXB];       // (n,)
  const double* col[A2_MAXB];
  const void* refl[A2_MAXB];        // (n,) uint8 / float32 / float64, or unused
  const uint8_t* label[A2_MAXB];    // (H, W, 3) uint8: the raw label image
  SegTable<A2_MAXB> seg;            // points and blocks of the call's flat numbering
};

// ------------------------------------------------------------------------------------------ the map
__device__ __forceinline__ int a2_fix(double u) {
  const double s = u * 32.0;
  if (!(fabs(s) < (double)INFINITY)) return INT_MIN;
  const double r = rint(s);
  return r >= 2147483647.0 ? INT_MAX : r <= -2147483648.0 ? INT_MIN : (int)r;
}
__device__ __forceinline__ int a2_sat16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

__global__ __launch_bounds__(256) void k_a2_map(const A2Cam c, int W, int64_t total, short2* __restrict__ xy, uint16_t* __restrict__ frac) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const int i = (int)(p / W), j = (int)(p - (int64_t)i * W);
  const double x = ((double)j - c.ncx) / c.nfx, y = ((double)i - c.ncy) / c.nfy;
  const double x2 = x * x, y2 = y * y, r2 = x2 + y2, t = (2.0 * x) * y;
  const double kr = (1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2) / (1.0 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2);
  const double xd = (x * kr + c.p1 * t) + c.p2 * (r2 + 2.0 * x2);
  const double yd = (y * kr + c.p1 * (r2 + 2.0 * y2)) + c.p2 * t;
  const int iu = a2_fix(c.fx * xd + c.cx), iv = a2_fix(c.fy * yd + c.cy);
  xy[p] = make_short2((short)a2_sat16(iu >> 5), (short)a2_sat16(iv >> 5));
  frac[p] = (uint16_t)(((iv & 31) << 5) | (iu & 31));
}

// ------------------------------------------------------------------------------------------ one remapped pixel
// A destination pixel whose map entry is (sx, sy, fr) -> r | g << 8 | b << 16; a tap outside the source counts as 0.
// Interior pixels (all four taps inside and 8 readable bytes from the lower-left tap on; lim = bytes of the plane - 8) take the 6 bytes
// of a tap pair as one unaligned 8-byte load: 2 loads per pixel for 12.  The border and the last pixels of the plane take the byte path.
__device__ __forceinline__ bool a2_interior(int W, int H, int64_t lim, int sx, int sy, int64_t& o) {
  o = ((int64_t)sy * W + sx) * 3;
  return (unsigned)sx < (unsigned)(W - 1) && (unsigned)sy < (unsigned)(H - 1) && o + (int64_t)W * 3 <= lim;
}
__device__ __forceinline__ void a2_load(const uint8_t* __restrict__ src, int W, int64_t o, uint2& t, uint2& b) {
  __builtin_memcpy(&t, src + o, 8);
  __builtin_memcpy(&b, src + o + (int64_t)W * 3, 8);
}
__device__ __forceinline__ uint32_t a2_blend(uint2 t, uint2 b, int fr) {
  const int fx = fr & 31, fy = (fr >> 5) & 31;
  const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
  const uint32_t t1 = t.x >> 24 | t.y << 8, b1 = b.x >> 24 | b.y << 8;            // the right taps' three bytes
  uint32_t out = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    out |= (uint32_t)((w00 * (int)(t.x >> (8 * ch) & 255) + w01 * (int)(t1 >> (8 * ch) & 255) + w10 * (int)(b.x >> (8 * ch) & 255) +
                       w11 * (int)(b1 >> (8 * ch) & 255) + 512) >> 10) << (8 * ch);
  return out;
}
__device__ __forceinline__ uint32_t a2_border(const uint8_t* __restrict__ src, int W, int H, int sx, int sy, int fr) {
  const int fx = fr & 31, fy = (fr >> 5) & 31;
  const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
  const bool x0 = (unsigned)sx < (unsigned)W, x1 = (unsigned)(sx + 1) < (unsigned)W;
  const bool y0 = (unsigned)sy < (unsigned)H, y1 = (unsigned)(sy + 1) < (unsigned)H;
  if (!((x0 || x1) && (y0 || y1))) return 0;
  const int64_t o = ((int64_t)sy * W + sx) * 3, o1 = o + (int64_t)W * 3;
  uint32_t out = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int p00 = x0 && y0 ? src[o + ch] : 0, p01 = x1 && y0 ? src[o + 3 + ch] : 0;
    const int p10 = x0 && y1 ? src[o1 + ch] : 0, p11 = x1 && y1 ? src[o1 + 3 + ch] : 0;
    out |= (uint32_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10) << (8 * ch);
  }
  return out;
}
__device__ __forceinline__ uint32_t a2_pixel(const uint8_t* __restrict__ src, int W, int H, int64_t lim, int sx, int sy, int fr) {
  int64_t o;
  if (!a2_interior(W, H, lim, sx, sy, o)) return a2_border(src, W, H, sx, sy, fr);
  uint2 t, b;
  a2_load(src, W, o, t, b);
  return a2_blend(t, b, fr);
}

// ------------------------------------------------------------------------------------------ the remap
// item = row * G + group (G = groups of PW = A2_PW pixels per row), blockIdx.y = group of A2_PLANES planes
__global__ __launch_bounds__(256) void k_a2_remap(const A2Planes a, int P, int H, int W, int G, const short2* __restrict__ xy,
                                                  const uint16_t* __restrict__ frac) {
  constexpr int PW = A2_PW;
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= H * G) return;
  const int row = item / G, c0 = (item - row * G) * PW;
  const int npx = W - c0 < PW ? W - c0 : PW;
  const int64_t m = (int64_t)row * W + c0, lim = (int64_t)H * W * 3 - 8;
  short2 s[PW];
  uint16_t f[PW];
  if (npx == PW && (m & 3) == 0) {                         // 16 bytes of xy and 8 of frac per four pixels, aligned
#pragma unroll
    for (int q = 0; q < PW / 4; ++q) {
      const uint4 v = *(const uint4*)(xy + m + 4 * q);
      const uint2 g = *(const uint2*)(frac + m + 4 * q);
      const uint32_t vs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        s[4 * q + k] = make_short2((short)(vs[k] & 0xFFFF), (short)(vs[k] >> 16));
        f[4 * q + k] = (uint16_t)((k < 2 ? g.x : g.y) >> (16 * (k & 1)));
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < PW; ++k) {
      s[k] = k < npx ? xy[m + k] : make_short2(-2, -2);
      f[k] = k < npx ? frac[m + k] : (uint16_t)0;
    }
  }
  bool in[PW];
  int64_t o[PW];
#pragma unroll
  for (int k = 0; k < PW; ++k) in[k] = a2_interior(W, H, lim, s[k].x, s[k].y, o[k]);      // a padding entry (-2, -2) is not
  // the map entries serve A2_PLANES planes: the map is read once for them
  const int p1 = (blockIdx.y + 1) * A2_PLANES < P ? (blockIdx.y + 1) * A2_PLANES : P;
  for (int p = blockIdx.y * A2_PLANES; p < p1; ++p) {
    const uint8_t* __restrict__ src = a.src[p];
    uint8_t* __restrict__ out = a.dst[p] + m * 3;
    // every interior load of the plane is issued before the first blend waits for one
    uint2 t[PW], b[PW];
#pragma unroll
    for (int k = 0; k < PW; ++k) {
      t[k] = b[k] = make_uint2(0, 0);
      if (in[k]) a2_load(src, W, o[k], t[k], b[k]);
    }
    uint32_t words[PW * 3 / 4] = {};
#pragma unroll
    for (int k = 0; k < PW; ++k) {
      const uint32_t v = in[k] ? a2_blend(t[k], b[k], f[k]) : k < npx ? a2_border(src, W, H, s[k].x, s[k].y, f[k]) : 0u;
      const int bit = 24 * k, wi = bit >> 5, sh = bit & 31;
      words[wi] |= v << sh;
      if (sh > 8) words[wi + 1] |= v >> (32 - sh);
    }
    if (npx == PW && ((uintptr_t)out & 3) == 0) {
#pragma unroll
      for (int q = 0; q < PW * 3 / 4; ++q) ((uint32_t*)out)[q] = words[q];
    } else {
#pragma unroll
      for (int e = 0; e < PW * 3; ++e)
        if (e < npx * 3) out[e] = (uint8_t)(words[e >> 2] >> (8 * (e & 3)));
    }
  }
}

// ------------------------------------------------------------------------------------------ the points
// astype(np.int32) of a float64: truncation; what does not fit (or is not a number) lies outside every image
__device__ __forceinline__ int a2_trunc(double v) { return v > -2147483649.0 && v < 2147483648.0 ? (int)v : INT_MIN; }

// refl_kind: 0 = none (feats = 1), 1 = uint8, 2 = float32, 3 = float64.  xy == null: the pass-through camera (no undistortion).
__global__ __launch_bounds__(A2_ROWS) void k_a2_points(const A2Frames a, int S, int points_f64, int refl_kind, const short2* __restrict__ xy,
                                                       const uint16_t* __restrict__ frac, int W, int H, const uint8_t* __restrict__ table,
                                                       int K, float* __restrict__ points, float* __restrict__ feats,
                                                       uint8_t* __restrict__ seg, float2* __restrict__ img, int* __restrict__ bad) {
  __shared__ uint32_t tab[A2_MAXK];
  for (int k = threadIdx.x; k < K; k += A2_ROWS) tab[k] = table[3 * k] | table[3 * k + 1] << 8 | table[3 * k + 2] << 16;
  __syncthreads();
  const int s = seg_of_block(a.seg.blk0, S, blockIdx.x);
  const int i = (blockIdx.x - a.seg.blk0[s]) * A2_ROWS + threadIdx.x;
  if (i >= a.seg.n[s]) return;
  const int64_t o = (int64_t)a.seg.row0[s] + i;
  const double rowd = a.row[s][i], cold = a.col[s][i];
  img[o] = make_float2((float)rowd, (float)cold);
  if (points_f64) {
    const double* p = (const double*)a.points[s] + 3 * (int64_t)i;
    points[3 * o] = (float)p[0]; points[3 * o + 1] = (float)p[1]; points[3 * o + 2] = (float)p[2];
  } else {
    const float* p = (const float*)a.points[s] + 3 * (int64_t)i;
    points[3 * o] = p[0]; points[3 * o + 1] = p[1]; points[3 * o + 2] = p[2];
  }
  float ft = 1.f;
  if (refl_kind == 1) ft = (float)__ddiv_rn((double)((const uint8_t*)a.refl[s])[i], 255.0);
  else if (refl_kind == 2) ft = __fdiv_rn(((const float*)a.refl[s])[i], 255.f);       // numpy keeps a float32 array in float32
  else if (refl_kind == 3) ft = (float)__ddiv_rn(((const double*)a.refl[s])[i], 255.0);
  feats[o] = ft;
  const int r = a2_trunc(rowd), c = a2_trunc(cold);
  int cls = K;
  if ((unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W) {
    const int64_t m = (int64_t)r * W + c;
    int sx = c, sy = r, fr = 0;
    if (xy) { const short2 e = xy[m]; sx = e.x; sy = e.y; fr = frac[m]; }
    const uint32_t px = a2_pixel(a.label[s], W, H, (int64_t)H * W * 3 - 8, sx, sy, fr);
    for (int k = 0; k < K; ++k) cls = tab[k] == px ? k : cls;          // ascending, overwriting: the last equal row wins
  } else {
    atomicAdd(bad + s, 1);
  }
  seg[o] = (uint8_t)cls;
}

// ------------------------------------------------------------------------------------------ entry points
MOPA_API int mopa_a2d2prep_max_frames(void) { return A2_MAXB; }
MOPA_API int mopa_a2d2prep_max_planes(void) { return A2_MAXP; }

// The undistortion map of one camera.  cam_host: 16 doubles, [fx, fy, cx, cy] of CamMatrixOriginal, the same of CamMatrix, then
// k1, k2, p1, p2, k3, k4, k5, k6 (absent coefficients 0).  xy (H, W, 2) int16 [sx, sy], frac (H, W) uint16 = fy5 * 32 + fx5.
MOPA_API int mopa_a2d2prep_map(const double* cam_host, int32_t W, int32_t H, int16_t* xy, uint16_t* frac, void* stream) {
  if (!cam_host || W < 1 || H < 1 || W > A2_MAXSIDE || H > A2_MAXSIDE || !xy || !frac || ((uintptr_t)xy & 3) || ((uintptr_t)frac & 1)) return MOPA_ERR_ARG;
  A2Cam c;
  c.fx = cam_host[0]; c.fy = cam_host[1]; c.cx = cam_host[2]; c.cy = cam_host[3];
  c.nfx = cam_host[4]; c.nfy = cam_host[5]; c.ncx = cam_host[6]; c.ncy = cam_host[7];
  c.k1 = cam_host[8]; c.k2 = cam_host[9]; c.p1 = cam_host[10]; c.p2 = cam_host[11];
  c.k3 = cam_host[12]; c.k4 = cam_host[13]; c.k5 = cam_host[14]; c.k6 = cam_host[15];
  const int64_t total = (int64_t)W * H;
  k_a2_map<<<(unsigned)cdiv64(total, 256), 256, 0, (hipStream_t)stream>>>(c, W, total, (short2*)xy, frac);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// dst_host[p] = the (H, W, 3) uint8 plane src_host[p] seen through the map, for P <= mopa_a2d2prep_max_planes() planes in one
// launch.  A destination must not overlap any source.
MOPA_API int mopa_a2d2prep_remap(const void* const* src_host, void* const* dst_host, int32_t P, int32_t H, int32_t W, const int16_t* xy,
                                 const uint16_t* frac, void* stream) {
  if (!src_host || !dst_host || P < 1 || P > A2_MAXP || W < 1 || H < 1 || W > A2_MAXSIDE || H > A2_MAXSIDE || !xy || !frac) return MOPA_ERR_ARG;
  if (((uintptr_t)xy & 15) || ((uintptr_t)frac & 7)) return MOPA_ERR_ARG;
  A2Planes a = {};
  for (int p = 0; p < P; ++p) {
    if (!src_host[p] || !dst_host[p]) return MOPA_ERR_ARG;
    a.src[p] = (const uint8_t*)src_host[p];
    a.dst[p] = (uint8_t*)dst_host[p];
  }
  const int G = (int)cdiv64(W, A2_PW);
  const dim3 grid((unsigned)cdiv64((int64_t)H * G, 256), (unsigned)cdiv64(P, A2_PLANES));      // H * G <= 32767 * 8192 < 2^31
  k_a2_remap<<<grid, 256, 0, (hipStream_t)stream>>>(a, P, H, W, G, (const short2*)xy, frac);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// The per-point arrays of B frames, the frames' points one after the other: points (sum n, 3) float32, feats (sum n,) float32
// (reflectance / 255, or 1 with refl_kind 0), seg_labels (sum n,) uint8 (the index of the last row of table (K, 3) uint8 equal to
// the undistorted label pixel at [int32(row), int32(col)], else K), points_img (sum n, 2) float32 [row, col]; bad (B,) int32 is
// cleared, then counts per frame the points outside the image (they get K).  points_host: (n, 3) float64 (points_f64 = 1) or
// float32; row_host / col_host: (n,) float64; refl_host: (n,) uint8 / float32 / float64 for refl_kind 1 / 2 / 3; label_host: the raw
// (H, W, 3) uint8 label images.  xy / frac: the camera's map, both null for a camera that is not undistorted.
MOPA_API int mopa_a2d2prep_points(const void* const* points_host, const void* const* row_host, const void* const* col_host,
                                  const void* const* refl_host, const void* const* label_host, const int32_t* n_host, int32_t B,
                                  int32_t points_f64, int32_t refl_kind, const int16_t* xy, const uint16_t* frac, int32_t W, int32_t H,
                                  const uint8_t* table, int32_t K, float* points, float* feats, uint8_t* seg_labels, float* points_img,
                                  int32_t* bad, void* stream) {
  A2Frames a = {};
  const int blk = seg_table_fill(a.seg, n_host, B, A2_ROWS);
  if (blk < 0 || !points_host || !row_host || !col_host || !label_host) return MOPA_ERR_ARG;
  if (refl_kind < 0 || refl_kind > 3 || (refl_kind && !refl_host) || (xy != nullptr) != (frac != nullptr)) return MOPA_ERR_ARG;
  if (W < 1 || H < 1 || W > A2_MAXSIDE || H > A2_MAXSIDE || K < 0 || K > A2_MAXK || (K > 0 && !table) || !bad) return MOPA_ERR_ARG;
  if (((uintptr_t)xy & 3) || ((uintptr_t)frac & 1) || ((uintptr_t)points_img & 7) || ((uintptr_t)points & 3) || ((uintptr_t)feats & 3)) return MOPA_ERR_ARG;
  const uintptr_t pmask = points_f64 ? 7 : 3, rmask = refl_kind == 3 ? 7 : refl_kind == 2 ? 3 : 0;
  for (int s = 0; s < B; ++s) {
    const int n = n_host[s];
    if (!label_host[s]) return MOPA_ERR_ARG;
    if (n > 0) {
      if (!points_host[s] || !row_host[s] || !col_host[s] || (refl_kind && !refl_host[s])) return MOPA_ERR_ARG;
      if (((uintptr_t)points_host[s] & pmask) || ((uintptr_t)row_host[s] & 7) || ((uintptr_t)col_host[s] & 7)) return MOPA_ERR_ARG;
      if (refl_kind && ((uintptr_t)refl_host[s] & rmask)) return MOPA_ERR_ARG;
    }
    a.points[s] = points_host[s];
    a.row[s] = (const double*)row_host[s];
    a.col[s] = (const double*)col_host[s];
    a.refl[s] = refl_kind ? refl_host[s] : nullptr;
    a.label[s] = (const uint8_t*)label_host[s];
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(bad, 0, (size_t)B * sizeof(int32_t), st) != hipSuccess) return MOPA_ERR_LAUNCH;
  if (blk == 0) return MOPA_OK;
  if (!points || !feats || !seg_labels || !points_img) return MOPA_ERR_ARG;
  k_a2_points<<<(unsigned)blk, A2_ROWS, 0, st>>>(a, B, points_f64, refl_kind, (const short2*)xy, frac, W, H, table, K, points, feats,
                                                seg_labels, (float2*)points_img, bad);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
