// The 2D half of the input pipeline on the device: raw uint8 camera image + SAM mask + float image points of a sample ->
// the normalised CHW float image, the int32 mask with -100 for ignored pixels and the int64 image indices the step consumes.
//
// Reference: the per-sample work of Dataset.__getitem__ (mopa/data/nuscenes/nuscenes_dataloader.py:347-408,
// mopa/data/a2d2/a2d2_dataloader.py:237-263, mopa/data/semantic_kitti/semantic_kitti_dataloader.py:563-630) and refine_sam_mask
// (mopa/data/utils/refine_pseudo_labels.py:72-102): Pillow's BILINEAR resize of 8-bit images, ImageEnhance's three blends and the
// HSV round trip of adjust_hue behind torchvision's ColorJitter, scipy.ndimage.zoom(order=0), np.fliplr, /255. and the
// normalisation.  Fixtures: G10, G14 (hue).
//
// Everything is exact: the resize is integer multiply-adds on host-built 22-bit coefficient tables (the horizontal pass rounds to
// uint8 before the vertical one, as Pillow's two passes do), the blends are float32 with every product and sum rounded on its
// own (no contraction), the hue step keeps Pillow's mix of float32 and double (ip_hue), the contrast mean and the mask's per-id
// areas are integer sums.  No float atomics.
//
// B images of one size go through a stage in ONE launch (blockIdx.z = image); the per-image pointers and draws are small host
// arrays copied into the kernel arguments, so nothing is uploaded and nothing synchronises.  3-byte pixels are read as aligned
// dwords into LDS (an aligned dword that holds one valid byte never leaves the allocation) and written back as dwords with at most
// three single bytes at either end of a row segment.
#pragma clang fp contract(off)
#include "common.h"

#define IP_MAXB 32            // images per launch (the binding splits larger batches)
#define IP_BLOCK 256
#define IP_RS_TW 128          // resize: output columns per block
#define IP_RS_LDS 16384       // resize: bytes of staged source rows per block (a 4:1 nuScenes tile needs 14 KB: 9 rows x 1.6 KB)
#define IP_RS_MAXR 256        // resize: staged rows per chunk
#define IP_RS_KREG 12         // resize: horizontal weights held in registers (9 at 4:1); wider filters read the table
#define IP_MASK_MAXW 16384    // mask: bytes of one staged source row
#define IP_IGNORE (-100)

struct IpSrc { const uint8_t* p[IP_MAXB]; };
struct IpJitter {
  int8_t order[IP_MAXB][4];   // 0 brightness, 1 contrast, 2 saturation, 3 hue, -1 = end of list
  float factor[IP_MAXB][4];   // factor of order[j] (unused for hue)
  uint8_t shift[IP_MAXB];     // hue: what is added to H modulo 256
  uint8_t flip[IP_MAXB];
};

// ------------------------------------------------------------------------------------------------ staging helpers
// Bytes [0, n) at `src` -> LDS as dwords read from the aligned address at or below `src`; byte i is ((uint8_t*)lds)[shift + i].
__device__ __forceinline__ int ip_stage(const uint8_t* __restrict__ src, int n, uint32_t* __restrict__ lds) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(src);
  const int s = (int)(a & 3);
  if (n <= 0) return s;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a - s);
  const int nd = (s + n + 3) >> 2;
  for (int i = threadIdx.x; i < nd; i += blockDim.x) lds[i] = p[i];
  return s;
}

// LDS bytes [0, n) -> dst: single bytes up to the first aligned address and after the last, dwords in between.
__device__ __forceinline__ void ip_store(uint8_t* __restrict__ dst, int n, const uint8_t* __restrict__ lds) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
  int head = (int)((4 - (a & 3)) & 3);
  if (head > n) head = n;
  const int body = (n - head) >> 2, tail = n - head - 4 * body;
  if ((int)threadIdx.x < head) dst[threadIdx.x] = lds[threadIdx.x];
  uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + head);
  for (int i = threadIdx.x; i < body; i += blockDim.x) {
    const uint8_t* q = lds + head + 4 * i;
    d32[i] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
  }
  if ((int)threadIdx.x < tail) dst[head + 4 * body + threadIdx.x] = lds[head + 4 * body + threadIdx.x];
}

__device__ __forceinline__ int ip_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ------------------------------------------------------------------------------------------------ 1. resize
// Tables: row j of xtab = {xmin, n, weight[0..kx)} (int32, pitch 2 + kx), likewise ytab.  One block = IP_RS_TW output pixels of
// one output row; the source rows under it are staged in chunks, each thread runs the horizontal pass of its pixel on a staged
// row, rounds it to uint8 and feeds it to its vertical sum.
__global__ __launch_bounds__(IP_RS_TW) void k_resize_u8(IpSrc src, int H, int W, const int32_t* __restrict__ xtab, int kx,
                                                        const int32_t* __restrict__ ytab, int ky, int h, int w,
                                                        uint8_t* __restrict__ dst) {
  __shared__ __align__(16) uint32_t rows[IP_RS_LDS / 4];
  __shared__ __align__(16) uint8_t outb[IP_RS_TW * 3 + 8];
  __shared__ int shift[IP_RS_MAXR];
  const int b = blockIdx.z, y = blockIdx.y, x0 = blockIdx.x * IP_RS_TW;
  const int x1 = min(x0 + IP_RS_TW, w), x = x0 + threadIdx.x;
  const int32_t* ty = ytab + (int64_t)y * (2 + ky);
  const int ymin = ty[0];
  int ny = ty[1];
  if (ymin < 0 || ny < 0 || ny > ky || ymin + ny > H) ny = 0;              // a malformed table reads nothing
  // source columns under this block (the tables are monotone: first pixel's left edge, last pixel's right edge)
  int sxa = xtab[(int64_t)x0 * (2 + kx)], sxb = xtab[(int64_t)(x1 - 1) * (2 + kx)] + xtab[(int64_t)(x1 - 1) * (2 + kx) + 1];
  sxa = max(0, min(sxa, W));
  sxb = max(sxa, min(sxb, W));
  const int seg = (sxb - sxa) * 3, pitch = ((seg + 3 + 3) >> 2) + 1;        // dwords per staged row
  const int R = min(IP_RS_LDS / 4 / pitch, IP_RS_MAXR);                     // rows per chunk (the entry point checked R >= 1)
  if (R < 1) ny = 0;
  const int32_t* tx = xtab + (int64_t)min(x, w - 1) * (2 + kx);
  const int xmin = tx[0];
  int nx = tx[1];
  if (x >= x1 || xmin < sxa || nx < 0 || nx > kx || xmin + nx > sxb) nx = 0;
  int acc0 = 0, acc1 = 0, acc2 = 0;
  const bool in_regs = nx <= IP_RS_KREG;
  int wx[IP_RS_KREG];
#pragma unroll
  for (int k = 0; k < IP_RS_KREG; ++k) wx[k] = (in_regs && k < nx) ? tx[2 + k] : 0;
  const uint8_t* img = src.p[b];
  for (int r0 = 0; r0 < ny; r0 += R) {
    const int nr = min(R, ny - r0);
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const int s = ip_stage(img + ((int64_t)(ymin + r0 + r) * W + sxa) * 3, seg, rows + r * pitch);
      if (threadIdx.x == 0) shift[r] = s;
    }
    __syncthreads();
    if (nx > 0) {
      for (int r = 0; r < nr; ++r) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(rows + r * pitch) + shift[r] + (xmin - sxa) * 3;
        int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
        if (in_regs) {
#pragma unroll
          for (int k = 0; k < IP_RS_KREG; ++k) {
            if (k < nx) {
              s0 += wx[k] * p[3 * k];
              s1 += wx[k] * p[3 * k + 1];
              s2 += wx[k] * p[3 * k + 2];
            }
          }
        } else {
          for (int k = 0; k < nx; ++k) {
            const int c = tx[2 + k];
            s0 += c * p[3 * k];
            s1 += c * p[3 * k + 1];
            s2 += c * p[3 * k + 2];
          }
        }
        const int wy = ty[2 + r0 + r];
        acc0 += wy * ip_clip8(s0 >> 22);
        acc1 += wy * ip_clip8(s1 >> 22);
        acc2 += wy * ip_clip8(s2 >> 22);
      }
    }
  }
  if (x < x1) {
    outb[3 * threadIdx.x] = (uint8_t)ip_clip8((acc0 + (1 << 21)) >> 22);
    outb[3 * threadIdx.x + 1] = (uint8_t)ip_clip8((acc1 + (1 << 21)) >> 22);
    outb[3 * threadIdx.x + 2] = (uint8_t)ip_clip8((acc2 + (1 << 21)) >> 22);
  }
  __syncthreads();
  ip_store(dst + (((int64_t)b * h + y) * w + x0) * 3, (x1 - x0) * 3, outb);
}

// src_host[b]: (H, W, 3) uint8; xtab (w, 2 + kx) / ytab (h, 2 + ky) int32 device tables {first source index, count, weights};
// max_span: the widest run of source columns under 128 consecutive output columns (from the host's table); dst (B, h, w, 3).
MOPA_API int mopa_imageprep_resize_u8(const void* const* src_host, int B, int H, int W, const int32_t* xtab, int kx,
                                      const int32_t* ytab, int ky, int h, int w, int max_span, uint8_t* dst, void* stream) {
  if (!src_host || B < 1 || B > IP_MAXB || H < 1 || W < 1 || h < 1 || w < 1 || h > 65535 || kx < 1 || ky < 1 || !xtab || !ytab || !dst)
    return MOPA_ERR_ARG;
  if (max_span < 1 || max_span > W || (((max_span * 3 + 6) >> 2) + 1) * 4 > IP_RS_LDS) return MOPA_ERR_ARG;
  IpSrc s;
  for (int b = 0; b < B; ++b) {
    if (!src_host[b]) return MOPA_ERR_ARG;
    s.p[b] = (const uint8_t*)src_host[b];
  }
  dim3 grid((w + IP_RS_TW - 1) / IP_RS_TW, h, B);
  hipLaunchKernelGGL(k_resize_u8, grid, dim3(IP_RS_TW), 0, (hipStream_t)stream, s, H, W, xtab, kx, ytab, ky, h, w, dst);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// ------------------------------------------------------------------------------------------------ 2. colour jitter
// Pillow's ImagingBlend(degenerate, image, f) on one channel value: float32, the product rounded before the sum; truncation for
// 0 <= f <= 1, clipping first otherwise.
__device__ __forceinline__ int ip_blend(int deg, int v, float f, bool inside) {
  const float p = f * (float)(v - deg);                 // rounded on its own: this file is compiled without contraction, and the
  const float t = (float)deg + p;                        // __fmul_rn / __fadd_rn of the headers are not (they may fuse)
  if (inside) return (int)t;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}
__device__ __forceinline__ int ip_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// torchvision's adjust_hue on a PIL image: Pillow's rgb2hsv, H = (H + shift) & 255, Pillow's hsv2rgb (Convert.c).  The round trip
// is lossy and is made for shift 0 too.  Pillow's widths are kept: rgb2hsv takes its quotients in float32, evaluates the three-way
// hue expression in double and stores it to float32; hsv2rgb stores f and fs to float32, takes fs * f as a float32 product and
// everything else in double.  fmod(x, 1.0) of an x in (0, 2) is x - floor(x), exactly; C's round() of these non-negative
// values is floor(x + 0.5).
__device__ __forceinline__ void ip_hue(int shift, int& r, int& g, int& b) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  const int V = maxc;
  int H = 0, S = 0;
  if (maxc != minc) {
    const float cr = (float)(maxc - minc);
    const float s = __fdiv_rn(cr, (float)maxc);
    S = ip_clip8((int)((double)s * 255.0));
    const double rc = (double)__fdiv_rn((float)(maxc - r), cr), gc = (double)__fdiv_rn((float)(maxc - g), cr),
                 bc = (double)__fdiv_rn((float)(maxc - b), cr);
    float h;
    if (r == maxc) h = (float)(bc - gc);
    else if (g == maxc) h = (float)(2.0 + rc - bc);
    else h = (float)(4.0 + gc - rc);
    const double x = (double)h / 6.0 + 1.0;
    h = (float)(x - floor(x));
    H = ip_clip8((int)((double)h * 255.0));
  }
  H = (H + shift) & 255;
  if (S == 0) {
    r = g = b = V;
    return;
  }
  const double h6 = (double)H * 6.0 / 255.0, fi = floor(h6);
  const float f = (float)(h6 - fi);
  const float fs = (float)((double)S / 255.0);
  const float fsf = fs * f;
  const double v = (double)V;
  const int p = ip_clip8((int)floor(v * (1.0 - (double)fs) + 0.5));
  const int q = ip_clip8((int)floor(v * (1.0 - (double)fsf) + 0.5));
  const int t = ip_clip8((int)floor(v * (1.0 - (double)fs * (1.0 - (double)f)) + 0.5));
  switch ((int)fi % 6) {                                   // H = 255 gives fi = 6
    case 0: r = V, g = t, b = p; break;
    case 1: r = q, g = V, b = p; break;
    case 2: r = p, g = V, b = t; break;
    case 3: r = p, g = q, b = V; break;
    case 4: r = t, g = p, b = V; break;
    default: r = V, g = p, b = q; break;
  }
}

// Applies order[] to (r, g, b); `until_contrast` stops in front of the contrast step and reports whether there is one.
__device__ __forceinline__ bool ip_jitter(const int8_t* order, const float* factor, int shift, int mean, bool until_contrast, int& r,
                                          int& g, int& b) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int op = order[j];
    if (op < 0) break;
    if (op == 1 && until_contrast) return true;
    if (op == 3) {
      ip_hue(shift, r, g, b);
      continue;
    }
    const float f = factor[j];
    const bool inside = f >= 0.f && f <= 1.f;
    const int l = ip_luma(r, g, b);
    const int d = op == 0 ? 0 : (op == 1 ? mean : l);
    r = ip_blend(d, r, f, inside);
    g = ip_blend(d, g, f, inside);
    b = ip_blend(d, b, f, inside);
  }
  return false;
}

__device__ __forceinline__ bool ip_has_contrast(const int8_t* order) {
  return order[0] == 1 || (order[0] >= 0 && (order[1] == 1 || (order[1] >= 0 && (order[2] == 1 || (order[2] >= 0 && order[3] == 1)))));
}

// sums[b] += sum of L over the image as it stands in front of its contrast step, a hue step before it included (integer: exact
// in any order)
__global__ __launch_bounds__(IP_BLOCK) void k_contrast_sums(IpSrc src, int64_t pitch, int h, int w, IpJitter jit,
                                                            unsigned long long* __restrict__ sums) {
  __shared__ __align__(16) uint32_t row[(IP_BLOCK * 3 + 8) / 4 + 1];
  __shared__ int part[IP_BLOCK / WAVE];
  const int b = blockIdx.z;
  if (!ip_has_contrast(jit.order[b])) return;
  const int x0 = blockIdx.x * IP_BLOCK, nxs = min(IP_BLOCK, w - x0);
  int acc = 0;
  for (int y = blockIdx.y; y < h; y += gridDim.y) {
    __syncthreads();
    const int s = ip_stage(src.p[b] + (int64_t)y * pitch + (int64_t)x0 * 3, nxs * 3, row);
    __syncthreads();
    if ((int)threadIdx.x < nxs) {
      const uint8_t* p = reinterpret_cast<const uint8_t*>(row) + s + 3 * threadIdx.x;
      int r = p[0], g = p[1], bl = p[2];
      ip_jitter(jit.order[b], jit.factor[b], jit.shift[b], 0, true, r, g, bl);
      acc += ip_luma(r, g, bl);                                            // <= 255 per row: no overflow below 2^23 rows
    }
  }
  acc = wave_sum_i(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int k = 0; k < IP_BLOCK / WAVE; ++k) t += (unsigned long long)part[k];
    atomicAdd(&sums[b], t);
  }
}

// jitter (+ flip) (+ /255., normalisation, CHW) of one row segment per block
__global__ __launch_bounds__(IP_BLOCK) void k_pixels(IpSrc src, int64_t pitch, int h, int w, IpJitter jit,
                                                     const unsigned long long* __restrict__ sums, uint8_t* __restrict__ dst_u8,
                                                     float* __restrict__ dst_f32, int normalise, float m0, float m1, float m2,
                                                     float d0, float d1, float d2, float* __restrict__ ori) {
  __shared__ __align__(16) uint32_t row[(IP_BLOCK * 3 + 8) / 4 + 1];
  __shared__ __align__(16) uint8_t outb[IP_BLOCK * 3 + 8];
  const int b = blockIdx.z, y = blockIdx.y, x0 = blockIdx.x * IP_BLOCK, nxs = min(IP_BLOCK, w - x0);
  const int s = ip_stage(src.p[b] + (int64_t)y * pitch + (int64_t)x0 * 3, nxs * 3, row);
  int mean = 0;
  if (ip_has_contrast(jit.order[b])) mean = (int)((double)sums[b] / (double)((int64_t)h * w) + 0.5);
  __syncthreads();
  const bool flip = jit.flip[b] != 0;
  const int x = x0 + threadIdx.x;
  if ((int)threadIdx.x < nxs) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(row) + s + 3 * threadIdx.x;
    int r = p[0], g = p[1], bl = p[2];
    const int64_t plane = (int64_t)h * w;
    if (ori) {
      float* o = ori + (int64_t)b * 3 * plane + (int64_t)y * w + x;
      o[0] = __fdiv_rn((float)r, 255.f);
      o[plane] = __fdiv_rn((float)g, 255.f);
      o[2 * plane] = __fdiv_rn((float)bl, 255.f);
    }
    ip_jitter(jit.order[b], jit.factor[b], jit.shift[b], mean, false, r, g, bl);
    if (dst_f32) {
      float f0 = __fdiv_rn((float)r, 255.f), f1 = __fdiv_rn((float)g, 255.f), f2 = __fdiv_rn((float)bl, 255.f);
      if (normalise) {
        f0 = __fdiv_rn(f0 - m0, d0);
        f1 = __fdiv_rn(f1 - m1, d1);
        f2 = __fdiv_rn(f2 - m2, d2);
      }
      float* o = dst_f32 + (int64_t)b * 3 * plane + (int64_t)y * w + (flip ? w - 1 - x : x);
      o[0] = f0;
      o[plane] = f1;
      o[2 * plane] = f2;
    }
    if (dst_u8) {
      const int t = flip ? nxs - 1 - (int)threadIdx.x : (int)threadIdx.x;   // position inside the (mirrored) segment
      outb[3 * t] = (uint8_t)r;
      outb[3 * t + 1] = (uint8_t)g;
      outb[3 * t + 2] = (uint8_t)bl;
    }
  }
  if (dst_u8) {
    __syncthreads();
    const int ox0 = flip ? w - x0 - nxs : x0;
    ip_store(dst_u8 + (((int64_t)b * h + y) * w + ox0) * 3, nxs * 3, outb);
  }
}

// `slots` operations per image in order_host / factor_host: 3 (brightness, contrast, saturation only) or 4 (hue too, with its
// shift in shift_host[b]); the slots a three-slot caller does not have are filled with -1.
static int ip_fill(const void* const* src_host, int B, int slots, const int32_t* order_host, const float* factor_host,
                   const int32_t* shift_host, const int32_t* flip_host, IpSrc& s, IpJitter& j) {
  if (!src_host || B < 1 || B > IP_MAXB) return MOPA_ERR_ARG;
  for (int b = 0; b < B; ++b) {
    if (!src_host[b]) return MOPA_ERR_ARG;
    s.p[b] = (const uint8_t*)src_host[b];
    unsigned seen = 0;
    bool ended = false;
    const int shift = shift_host ? shift_host[b] : 0;
    if (shift < 0 || shift > 255) return MOPA_ERR_ARG;
    j.shift[b] = (uint8_t)shift;
    for (int k = 0; k < 4; ++k) {
      const int op = (order_host && k < slots) ? order_host[slots * b + k] : -1;
      if (op < -1 || op >= slots) return MOPA_ERR_ARG;
      if (op < 0) ended = true;
      else if (ended || (seen & (1u << op))) return MOPA_ERR_ARG;         // each operation at most once, no gaps
      else seen |= 1u << op;
      if (op == 3 && !shift_host) return MOPA_ERR_ARG;
      const bool blend = op >= 0 && op <= 2;
      if (blend && !factor_host) return MOPA_ERR_ARG;
      j.order[b][k] = (int8_t)op;
      j.factor[b][k] = blend ? factor_host[slots * b + k] : 1.f;
      if (blend && !(j.factor[b][k] == j.factor[b][k])) return MOPA_ERR_ARG;
    }
    j.flip[b] = (flip_host && flip_host[b]) ? 1 : 0;
  }
  return MOPA_OK;
}

static int ip_contrast_sums(const void* const* src_host, int B, int64_t pitch, int h, int w, int slots, const int32_t* order_host,
                            const float* factor_host, const int32_t* shift_host, void* sums, void* stream) {
  IpSrc s;
  IpJitter j;
  if (ip_fill(src_host, B, slots, order_host, factor_host, shift_host, nullptr, s, j) != MOPA_OK) return MOPA_ERR_ARG;
  if (h < 1 || w < 1 || pitch < (int64_t)w * 3 || !sums || (int64_t)h * w > ((int64_t)1 << 31)) return MOPA_ERR_ARG;
  if (hipMemsetAsync(sums, 0, 8 * (size_t)B, (hipStream_t)stream) != hipSuccess) return MOPA_ERR_LAUNCH;
  dim3 grid((w + IP_BLOCK - 1) / IP_BLOCK, min(h, 64), B);
  hipLaunchKernelGGL(k_contrast_sums, grid, dim3(IP_BLOCK), 0, (hipStream_t)stream, s, pitch, h, w, j, (unsigned long long*)sums);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

static int ip_pixels(const void* const* src_host, int B, int64_t pitch, int h, int w, int slots, const int32_t* order_host,
                     const float* factor_host, const int32_t* shift_host, const void* sums, const int32_t* flip_host,
                     uint8_t* dst_u8, float* dst_f32, const float* norm_host, float* ori, void* stream) {
  IpSrc s;
  IpJitter j;
  if (ip_fill(src_host, B, slots, order_host, factor_host, shift_host, flip_host, s, j) != MOPA_OK) return MOPA_ERR_ARG;
  if (h < 1 || w < 1 || h > 65535 || pitch < (int64_t)w * 3 || (!dst_u8 && !dst_f32)) return MOPA_ERR_ARG;
  for (int b = 0; b < B; ++b) {
    bool contrast = false;
    for (int k = 0; k < 4; ++k) contrast |= j.order[b][k] == 1;
    if (contrast && !sums) return MOPA_ERR_ARG;
  }
  float n[6] = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f};
  if (norm_host)
    for (int k = 0; k < 6; ++k) n[k] = norm_host[k];
  dim3 grid((w + IP_BLOCK - 1) / IP_BLOCK, h, B);
  hipLaunchKernelGGL(k_pixels, grid, dim3(IP_BLOCK), 0, (hipStream_t)stream, s, pitch, h, w, j, (const unsigned long long*)sums,
                     dst_u8, dst_f32, norm_host ? 1 : 0, n[0], n[1], n[2], n[3], n[4], n[5], ori);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// sums: B x uint64, zeroed here.  pitch: bytes between rows of the (possibly cropped) h x w window src_host[b] points at.
// order_host: B x 3 operations in the order they are applied (0 brightness, 1 contrast, 2 saturation, -1 = none left), each at
// most once; factor_host: B x 3, the factor of order_host[b][j].
MOPA_API int mopa_imageprep_contrast_sums(const void* const* src_host, int B, int64_t pitch, int h, int w,
                                          const int32_t* order_host, const float* factor_host, void* sums, void* stream) {
  return ip_contrast_sums(src_host, B, pitch, h, w, 3, order_host, factor_host, nullptr, sums, stream);
}

// dst_u8 (B, h, w, 3) and / or dst_f32 (B, 3, h, w); norm_host = {mean[3], std[3]} or null; ori (B, 3, h, w) or null: the
// unjittered, unflipped /255. copy.  sums: what mopa_imageprep_contrast_sums wrote (null when no image has a contrast step).
MOPA_API int mopa_imageprep_pixels(const void* const* src_host, int B, int64_t pitch, int h, int w, const int32_t* order_host,
                                   const float* factor_host, const void* sums, const int32_t* flip_host, uint8_t* dst_u8,
                                   float* dst_f32, const float* norm_host, float* ori, void* stream) {
  return ip_pixels(src_host, B, pitch, h, w, 3, order_host, factor_host, nullptr, sums, flip_host, dst_u8, dst_f32, norm_host, ori,
                   stream);
}

// The same two with the fourth operation: order_host and factor_host are B x 4, operation 3 = hue (torchvision's adjust_hue on a
// PIL image); its factor slot is not read, shift_host[b] = int(hue_factor * 255) mod 256, in 0..255, is what is added to H.  The
// sums are taken of the image in front of its contrast step, a hue step before it applied.
MOPA_API int mopa_imageprep_contrast_sums4(const void* const* src_host, int B, int64_t pitch, int h, int w,
                                           const int32_t* order_host, const float* factor_host, const int32_t* shift_host,
                                           void* sums, void* stream) {
  return ip_contrast_sums(src_host, B, pitch, h, w, 4, order_host, factor_host, shift_host, sums, stream);
}

MOPA_API int mopa_imageprep_pixels4(const void* const* src_host, int B, int64_t pitch, int h, int w, const int32_t* order_host,
                                    const float* factor_host, const int32_t* shift_host, const void* sums,
                                    const int32_t* flip_host, uint8_t* dst_u8, float* dst_f32, const float* norm_host, float* ori,
                                    void* stream) {
  return ip_pixels(src_host, B, pitch, h, w, 4, order_host, factor_host, shift_host, sums, flip_host, dst_u8, dst_f32, norm_host,
                   ori, stream);
}

// ------------------------------------------------------------------------------------------------ 4. SAM mask
// ytab (h) / xtab (w): source row / column of a zoomed pixel, -1 = outside the file's mask (reads the constant 0); null = the
// mask is used as it is (h == H, w == W).
__device__ __forceinline__ int ip_mask_at(const uint8_t* row, int sx) { return sx < 0 ? 0 : row[sx]; }

__global__ __launch_bounds__(IP_BLOCK) void k_mask_hist(IpSrc src, int H, int W, const int32_t* __restrict__ ytab,
                                                        const int32_t* __restrict__ xtab, int h, int w, int32_t* __restrict__ counts) {
  __shared__ __align__(16) uint32_t row[IP_MASK_MAXW / 4 + 2];
  __shared__ int hist[256];
  const int b = blockIdx.z;
  hist[threadIdx.x] = 0;                                                   // IP_BLOCK == 256
  for (int y = blockIdx.x; y < h; y += gridDim.x) {
    int sy = ytab ? ytab[y] : y;
    if (sy >= H) sy = -1;
    __syncthreads();
    if (sy < 0) {
      if (threadIdx.x == 0) atomicAdd(&hist[0], w);
      continue;
    }
    const int s = ip_stage(src.p[b] + (int64_t)sy * W, W, row);
    __syncthreads();
    const uint8_t* r8 = reinterpret_cast<const uint8_t*>(row) + s;
    for (int x = threadIdx.x; x < w; x += blockDim.x) {
      int sx = xtab ? xtab[x] : x;
      if (sx >= W) sx = -1;
      atomicAdd(&hist[ip_mask_at(r8, sx)], 1);
    }
  }
  __syncthreads();
  if (hist[threadIdx.x]) atomicAdd(&counts[b * 256 + threadIdx.x], hist[threadIdx.x]);
}

struct IpMaskArgs {
  int32_t row_limit[IP_MAXB];   // refine_sam_mask's h - max_h when it is known on the host
  int32_t top[IP_MAXB], left[IP_MAXB];
  uint8_t flip[IP_MAXB];
};

__global__ __launch_bounds__(IP_BLOCK) void k_mask_out(IpSrc src, int H, int W, const int32_t* __restrict__ ytab,
                                                       const int32_t* __restrict__ xtab, int h, int w,
                                                       const int32_t* __restrict__ counts, int min_count, IpMaskArgs a,
                                                       int limit_mode, const int32_t* __restrict__ row_limit_dev, int oh, int ow,
                                                       int32_t* __restrict__ dst) {
  __shared__ __align__(16) uint32_t row[IP_MASK_MAXW / 4 + 2];
  __shared__ int big[256];
  const int b = blockIdx.z, oy = blockIdx.y;
  big[threadIdx.x] = counts[b * 256 + threadIdx.x] >= min_count;
  const int zy = oy + a.top[b];
  int sy = ytab ? ytab[zy] : zy;
  if (sy >= H) sy = -1;
  int s = 0;
  if (sy >= 0) s = ip_stage(src.p[b] + (int64_t)sy * W, W, row);
  __syncthreads();
  // sam_mask[:h_limit] = -100 with Python's slice rule: a negative limit counts from the end
  bool cut = false;
  if (limit_mode) {
    const int64_t hl = limit_mode == 2 ? row_limit_dev[b] : a.row_limit[b];
    const int64_t lim = hl >= 0 ? (hl < h ? hl : h) : (h + hl > 0 ? h + hl : 0);
    cut = zy < lim;
  }
  const uint8_t* r8 = reinterpret_cast<const uint8_t*>(row) + s;
  int32_t* o = dst + ((int64_t)b * oh + oy) * ow;
  for (int ox = threadIdx.x; ox < ow; ox += blockDim.x) {
    const int zx = a.left[b] + (a.flip[b] ? ow - 1 - ox : ox);
    int sx = xtab ? xtab[zx] : zx;
    if (sx >= W) sx = -1;
    const int v = sy < 0 ? 0 : ip_mask_at(r8, sx);
    o[ox] = (cut || big[v]) ? IP_IGNORE : v;
  }
}

MOPA_API size_t mopa_imageprep_mask_workspace_bytes(int B) { return B > 0 ? (size_t)B * 256 * 4 : 0; }

// Mask (H, W) uint8 -> nearest zoom to (h, w) -> ids with >= min_count pixels and rows [: row limit] become -100 -> crop window
// (top, left, oh, ow) -> flip -> dst (B, oh, ow) int32.  limit_mode 0: no row limit; 1: row_limit_host[b]; 2: row_limit_dev[b]
// (what mopa_imageprep_indices reduced from the points).  crop_host: B x {top, left} or null.
MOPA_API int mopa_imageprep_mask(const void* const* mask_host, int B, int H, int W, const int32_t* ytab, const int32_t* xtab, int h,
                                 int w, int min_count, int limit_mode, const int32_t* row_limit_host, const int32_t* row_limit_dev,
                                 const int32_t* crop_host, int oh, int ow, const int32_t* flip_host, int32_t* dst, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (!mask_host || B < 1 || B > IP_MAXB || H < 1 || W < 1 || W > IP_MASK_MAXW || h < 1 || w < 1 || oh < 1 || ow < 1 || oh > 65535 ||
      !dst || limit_mode < 0 || limit_mode > 2)
    return MOPA_ERR_ARG;
  if ((!ytab && h != H) || (!xtab && w != W)) return MOPA_ERR_ARG;
  if ((limit_mode == 1 && !row_limit_host) || (limit_mode == 2 && !row_limit_dev)) return MOPA_ERR_ARG;
  if (!ws || ws_bytes < mopa_imageprep_mask_workspace_bytes(B)) return MOPA_ERR_WORKSPACE;
  IpSrc s;
  IpMaskArgs a;
  for (int b = 0; b < B; ++b) {
    if (!mask_host[b]) return MOPA_ERR_ARG;
    s.p[b] = (const uint8_t*)mask_host[b];
    a.top[b] = crop_host ? crop_host[2 * b] : 0;
    a.left[b] = crop_host ? crop_host[2 * b + 1] : 0;
    if (a.top[b] < 0 || a.left[b] < 0 || (int64_t)a.top[b] + oh > h || (int64_t)a.left[b] + ow > w) return MOPA_ERR_ARG;
    a.row_limit[b] = limit_mode == 1 ? row_limit_host[b] : 0;
    a.flip[b] = (flip_host && flip_host[b]) ? 1 : 0;
  }
  int32_t* counts = (int32_t*)ws;
  if (hipMemsetAsync(counts, 0, (size_t)B * 256 * 4, (hipStream_t)stream) != hipSuccess) return MOPA_ERR_LAUNCH;
  hipLaunchKernelGGL(k_mask_hist, dim3(min(h, 128), 1, B), dim3(IP_BLOCK), 0, (hipStream_t)stream, s, H, W, ytab, xtab, h, w, counts);
  MOPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_mask_out, dim3(1, oh, B), dim3(IP_BLOCK), 0, (hipStream_t)stream, s, H, W, ytab, xtab, h, w, counts,
                     min_count, a, limit_mode, row_limit_dev, oh, ow, dst);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// ------------------------------------------------------------------------------------------------ 5. image indices
struct IpPts {
  const void* pts[IP_MAXB];     // (n, 2) float32 or float64, [row, col]
  int64_t* idx[IP_MAXB];        // (n, 2) int64
  int64_t* ori[IP_MAXB];        // (n, 2) int64 or null
  uint8_t* keep[IP_MAXB];       // (n,) or null
  int32_t n[IP_MAXB];
  int32_t win[IP_MAXB][4];      // left, top, right, bottom
  uint8_t flip[IP_MAXB];
};

// float -> int64 as numpy's astype does for values in range (truncation); out of range and NaN give INT64_MIN, as on x86
template <typename T>
__device__ __forceinline__ int64_t ip_trunc(T v) {
  if (!(v >= (T)-9223372036854775808.0 && v < (T)9223372036854775808.0)) return INT64_MIN;
  return (int64_t)v;
}

// mode 0: resize form  p = s * floor(p) in T (s rounded to T first, as numpy does with a Python float against an array);
// mode 1: crop form    keep = inside the window, p -= (top, left) in T.
template <typename T>
__global__ __launch_bounds__(IP_BLOCK) void k_indices(IpPts a, int mode, double sy, double sx, int w_out,
                                                      int32_t* __restrict__ row_min) {
  __shared__ int part[IP_BLOCK / WAVE];
  const int b = blockIdx.y, n = a.n[b];
  const T* pts = reinterpret_cast<const T*>(a.pts[b]);
  const T ty = (T)sy, tx = (T)sx;
  int mn = INT32_MAX;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    T r = pts[2 * i], c = pts[2 * i + 1];
    if (mode == 0) {
      r = ty * floor(r);
      c = tx * floor(c);
    }
    if (row_min) {                                                          // int(np.min(points_img[:, 0])): trunc is monotone
      const T cl = r < (T)-1073741824.0 ? (T)-1073741824.0 : (r > (T)1073741824.0 ? (T)1073741824.0 : r);
      mn = min(mn, (int)cl);
    }
    if (a.ori[b]) {
      a.ori[b][2 * i] = ip_trunc<T>(r);
      a.ori[b][2 * i + 1] = ip_trunc<T>(c);
    }
    if (mode == 1) {
      const T l = (T)a.win[b][0], t = (T)a.win[b][1], rr = (T)a.win[b][2], bb = (T)a.win[b][3];
      if (a.keep[b]) a.keep[b][i] = (r >= t && r < bb && c >= l && c < rr) ? 1 : 0;
      r = r - t;
      c = c - l;
    }
    const int64_t ir = ip_trunc<T>(r);
    int64_t ic = ip_trunc<T>(c);
    if (a.flip[b]) ic = (int64_t)w_out - 1 - ic;
    a.idx[b][2 * i] = ir;
    a.idx[b][2 * i + 1] = ic;
  }
  if (row_min) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = min(mn, __shfl_xor(mn, o, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mn;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < IP_BLOCK / WAVE; ++k) mn = min(mn, part[k]);
      if (mn != INT32_MAX) atomicMin(&row_min[b], mn);
    }
  }
}

// pts_host[b]: (n_host[b], 2) points [row, col], dtype 0 = float32, 1 = float64.  mode 0 (resize): p = (sy, sx) * floor(p);
// mode 1 (crop): win_host = B x {left, top, right, bottom}, keep_host[b] (n,) uint8 says which points lie inside, p -= origin.
// idx_host[b] (n, 2) int64 = trunc(p), column mirrored to w_out - 1 - col where flip_host[b]; ori_host[b] (optional) = trunc of
// the points before crop and flip.  row_min (B x int32, optional): trunc(min over the points' rows in front of the crop), the
// row limit of the mask stage; a sample without points leaves 0x7f7f7f7f.
MOPA_API int mopa_imageprep_indices(const void* const* pts_host, const int32_t* n_host, int B, int dtype, int mode, double sy,
                                    double sx, const int32_t* win_host, int w_out, const int32_t* flip_host,
                                    void* const* idx_host, void* const* ori_host, void* const* keep_host, int32_t* row_min,
                                    void* stream) {
  if (!pts_host || !n_host || !idx_host || B < 1 || B > IP_MAXB || dtype < 0 || dtype > 1 || mode < 0 || mode > 1) return MOPA_ERR_ARG;
  if (mode == 1 && !win_host) return MOPA_ERR_ARG;
  IpPts a;
  int nmax = 0;
  for (int b = 0; b < B; ++b) {
    a.n[b] = n_host[b];
    if (a.n[b] < 0 || a.n[b] > (1 << 30) || (a.n[b] > 0 && (!pts_host[b] || !idx_host[b]))) return MOPA_ERR_ARG;
    a.pts[b] = pts_host[b];
    a.idx[b] = (int64_t*)idx_host[b];
    a.ori[b] = ori_host ? (int64_t*)ori_host[b] : nullptr;
    a.keep[b] = keep_host ? (uint8_t*)keep_host[b] : nullptr;
    for (int k = 0; k < 4; ++k) a.win[b][k] = win_host ? win_host[4 * b + k] : 0;
    a.flip[b] = (flip_host && flip_host[b]) ? 1 : 0;
    nmax = max(nmax, a.n[b]);
  }
  if (row_min && hipMemsetAsync(row_min, 0x7f, 4 * (size_t)B, (hipStream_t)stream) != hipSuccess) return MOPA_ERR_LAUNCH;
  if (nmax == 0) return MOPA_OK;
  dim3 grid(stream_grid(nmax, IP_BLOCK), B);
  if (dtype == 0)
    hipLaunchKernelGGL(k_indices<float>, grid, dim3(IP_BLOCK), 0, (hipStream_t)stream, a, mode, sy, sx, w_out, row_min);
  else
    hipLaunchKernelGGL(k_indices<double>, grid, dim3(IP_BLOCK), 0, (hipStream_t)stream, a, mode, sy, sx, w_out, row_min);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
