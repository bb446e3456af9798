// Dense 2D pseudo labels from SAM masks on the device: per sample the per-point maximum probabilities, raw 2D pseudo labels and
// image points plus the unrefined SAM mask -> the (H, W) int32 label map full_2d_pslabels (-100 = ignore), cropped and flipped.
//
// Reference: refine_sam_2Dlabels (mopa/data/utils/refine_pseudo_labels.py:25-69) behind the row expansion of
// SemanticKITTISCN.preprocess (mopa/data/semantic_kitti/semantic_kitti_dataloader.py:443-451) and the crop + flip of __getitem__
// (:587-590, :611-613).  Fixture: G17.
//
// The (N, C) probability rows are never built.  A row is `off = (1 - p) / (C - 1)` everywhere and `p` at the raw label, so its
// maximum `conf` and first arg-max `label'` follow from p, off and the raw label alone; the per-class median refinement of
// (conf, label') is mopa_refine_pseudo_labels_segmented (scanprep.hip), one segment per image.  The last point in array order wins
// a pixel (atomicMax of the point index), which is what index_put_ does with one thread.
//
// The per-id class sums are the one place where the reference is not reproducible (torch's float32 reduction order).  Here every
// row value x is added as the integer llrint(x * 2^40) with 64-bit integer atomics: exact to 2^-41 per term whatever the order,
// so the result is the same bits on every run.  Only the arg-max of the sums is needed, and the sum of class c is
//     S + D[c],   S = sum of q(off) over the id's reliable winners,   D[c] = sum of q(p) - q(off) over those with raw label c
// exactly (integer adds are associative), so only D is accumulated: one atomic per reliable winner instead of C.  The maximal
// sum of an id with k >= 1 reliable winners is at least k / C (a row sums to 1), so k * 2^-41 is far inside the k * 2^-24 * s
// that decides an id.  No float atomics.
//
// B images of one size go through every pass in ONE launch (blockIdx.z or .y = image); pointers, sizes and draws are small host
// arrays copied into the kernel arguments.  The launch count does not depend on B; nothing is read back.
#pragma clang fp contract(off)
#include "common.h"

#define DL_MAXB 32            // images per call (imageprep.hip IP_MAXB)
#define DL_MAXC 32            // classes (scanprep.hip SP_MAXC)
#define DL_BLOCK 256
#define DL_IGNORE (-100)
#define DL_SKIP INT32_MIN     // lookup value of an id that is left alone (too large, or absent)
#ifndef DL_STAT_BLOCKS
#define DL_STAT_BLOCKS 32     // blocks per image of the statistics pass (8 and 128 per image measured slower at B = 8: profiles/r29_denselabels.md)
#endif
#define DL_FIX 1099511627776.0  // 2^40

extern "C" size_t mopa_refine_pseudo_labels_segmented_workspace_bytes(int32_t S, int32_t C);
extern "C" int mopa_refine_pseudo_labels_segmented(const void* const* prob_host, const void* const* label_host, int32_t label_dtype,
                                                   const int32_t* n_host, void* const* out_host, int32_t S, int32_t C, int64_t ignore_label,
                                                   void* ws, size_t ws_bytes, void* stream);

struct DlArgs {
  const float* prob[DL_MAXB];     // (n,) float32: the maximum probability per point
  const uint8_t* label[DL_MAXB];  // (n,) uint8: the raw label
  const void* pts[DL_MAXB];       // (n, 2) float32 / float64 [row, col]
  const uint8_t* mask[DL_MAXB];   // (H, W) uint8
  int32_t n[DL_MAXB];
  int32_t row0[DL_MAXB];          // first point of the image in the call's flat point arrays
  int32_t top[DL_MAXB], left[DL_MAXB];
  uint8_t flip[DL_MAXB];
};

// Workspace layout (every part 256-byte aligned); the first four parts are zeroed by one memset per call.
struct DlWs {
  size_t win, area, sums, bad, zero_bytes;   // winner map u32 [B][H*W] (point index + 1, 0 = none), i32 [B][256], i64 [B][256][C], i32 [B]
  size_t lut, conf, lab, pix, refined, refine_ws, refine_bytes, total;
};
static DlWs dl_layout(int B, int64_t HW, int64_t n_total, int C) {
  DlWs w;
  size_t o = 0;
  w.win = o;      o += align_up((size_t)B * HW * 4, 256);
  w.area = o;     o += align_up((size_t)B * 256 * 4, 256);
  w.sums = o;     o += align_up((size_t)B * 256 * C * 8, 256);
  w.bad = o;      o += align_up((size_t)B * 4, 256);
  w.zero_bytes = o;
  w.lut = o;      o += align_up((size_t)B * 256 * 4, 256);
  w.conf = o;     o += align_up((size_t)n_total * 4, 256);
  w.lab = o;      o += align_up((size_t)n_total * 4, 256);
  w.pix = o;      o += align_up((size_t)n_total * 4, 256);
  w.refined = o;  o += align_up((size_t)n_total * 8, 256);
  w.refine_ws = o;
  w.refine_bytes = mopa_refine_pseudo_labels_segmented_workspace_bytes(B, C);
  o += w.refine_bytes;
  w.total = o;
  return w;
}

__device__ __forceinline__ float dl_off(float p, int C) { return __fdiv_rn(1.0f - p, (float)(C - 1)); }

// ------------------------------------------------------------------------------------------------ 1 + 3. points, winners
// conf = max of the row, lab = its first arg-max, pix = row-major pixel of (int(row), int(col)); a point outside the image, with
// a raw label >= C or with a probability outside [0, 1] gets lab = pix = -1 and is counted.  The winner map keeps the highest
// point index + 1 per pixel.
__global__ __launch_bounds__(DL_BLOCK) void k_dl_points(const DlArgs a, int pts_f64, int H, int W, int C, float* __restrict__ conf,
                                                        int32_t* __restrict__ lab, int32_t* __restrict__ pix,
                                                        uint32_t* __restrict__ win, int32_t* __restrict__ bad) {
  const int b = blockIdx.y, n = a.n[b];
  const float* __restrict__ prob = a.prob[b];
  const uint8_t* __restrict__ label = a.label[b];
  const int64_t r0 = a.row0[b];
  uint32_t* wb = win + (int64_t)b * H * W;
  for (int i = blockIdx.x * DL_BLOCK + threadIdx.x; i < n; i += gridDim.x * DL_BLOCK) {
    const float p = prob[i];
    const int raw = label[i];
    double r, c;
    if (pts_f64) {
      const double* q = (const double*)a.pts[b] + 2 * (int64_t)i;
      r = q[0]; c = q[1];
    } else {
      const float* q = (const float*)a.pts[b] + 2 * (int64_t)i;
      r = q[0]; c = q[1];
    }
    // truncation toward zero: (-1, 0) lands on 0.  NaN fails every comparison.
    const bool ok = r > -1.0 && r < (double)H && c > -1.0 && c < (double)W && raw < C && p >= 0.0f && p <= 1.0f;
    float cf = 0.0f;
    int l = -1, px = -1;
    if (ok) {
      const float off = dl_off(p, C);
      cf = p > off ? p : off;
      l = p > off ? raw : (p < off ? (raw != 0 ? 0 : 1) : 0);
      px = (int)r * W + (int)c;
      atomicMax(&wb[px], (uint32_t)i + 1u);
    } else {
      atomicAdd(&bad[b], 1);
    }
    conf[r0 + i] = cf;
    lab[r0 + i] = l;
    pix[r0 + i] = px;
  }
}

// ------------------------------------------------------------------------------------------------ 4. per-id statistics
// Area histogram over the image's pixels, then class sums over its reliable winners, both in LDS with integer atomics and one
// flush of the non-zero bins per block each.  The two tables share the LDS (int hist[256], then int64 D[256][C]: 64 KB at C = 32).
__global__ __launch_bounds__(DL_BLOCK) void k_dl_stats(const DlArgs a, int H, int W, int C, const int32_t* __restrict__ pix,
                                                       const int64_t* __restrict__ refined, const uint32_t* __restrict__ win,
                                                       int32_t* __restrict__ area, unsigned long long* __restrict__ sums) {
  extern __shared__ __align__(16) unsigned long long dl_lds[];
  unsigned long long* D = dl_lds;
  int* hist = reinterpret_cast<int*>(dl_lds);
  const int b = blockIdx.y;
  hist[threadIdx.x] = 0;                                                   // DL_BLOCK == 256
  __syncthreads();
  const uint8_t* __restrict__ m = a.mask[b];
  const int64_t HW = (int64_t)H * W;
  // pixels: single bytes up to the first aligned address and after the last aligned dword, dwords in between
  const int64_t head = min((int64_t)((4 - (reinterpret_cast<uintptr_t>(m) & 3)) & 3), HW);
  const int64_t body = (HW - head) >> 2, tail0 = head + 4 * body;
  const int tid = blockIdx.x * DL_BLOCK + threadIdx.x, nthr = gridDim.x * DL_BLOCK;
  if (tid < head) atomicAdd(&hist[m[tid]], 1);
  if (tid < HW - tail0) atomicAdd(&hist[m[tail0 + tid]], 1);
  const uint32_t* __restrict__ m32 = reinterpret_cast<const uint32_t*>(m + head);
  for (int64_t i = tid; i < body; i += nthr) {
    const uint32_t v = m32[i];
    if (v == (v & 255u) * 0x01010101u) {                                   // four pixels of one id, the common case: one add
      atomicAdd(&hist[v & 255u], 4);
    } else {
      atomicAdd(&hist[v & 255u], 1);
      atomicAdd(&hist[(v >> 8) & 255u], 1);
      atomicAdd(&hist[(v >> 16) & 255u], 1);
      atomicAdd(&hist[v >> 24], 1);
    }
  }
  __syncthreads();
  if (hist[threadIdx.x]) atomicAdd(&area[b * 256 + threadIdx.x], hist[threadIdx.x]);
  __syncthreads();
  // points: a reliable winner adds q(p) - q(off) to its id's sum of its raw class
  for (int i = threadIdx.x; i < 256 * C; i += DL_BLOCK) D[i] = 0ull;
  __syncthreads();
  const int n = a.n[b];
  const int64_t r0 = a.row0[b];
  const uint32_t* wb = win + (int64_t)b * HW;
  for (int i = tid; i < n; i += nthr) {
    const int px = pix[r0 + i];
    if (px < 0 || wb[px] != (uint32_t)i + 1u || refined[r0 + i] < 0) continue;
    const float p = a.prob[b][i];
    const long long q = llrint((double)p * DL_FIX) - llrint((double)dl_off(p, C) * DL_FIX);
    atomicAdd(&D[(int)m[px] * C + a.label[b][i]], (unsigned long long)q);
  }
  __syncthreads();
  unsigned long long* g = sums + (size_t)b * 256 * C;
  for (int i = threadIdx.x; i < 256 * C; i += DL_BLOCK)
    if (D[i]) atomicAdd(&g[i], D[i]);
}

// ------------------------------------------------------------------------------------------------ 5. lookup
// One thread per id: DL_SKIP for an id of min_count pixels or more (or of none), else the first arg-max of its class sums --
// class 0 when no reliable point lies in it.  Thread 0 hands out the image's count of skipped points.
__global__ __launch_bounds__(256) void k_dl_lookup(int C, int min_count, const int32_t* __restrict__ area,
                                                   const long long* __restrict__ sums, const int32_t* __restrict__ bad,
                                                   int32_t* __restrict__ lut, int32_t* __restrict__ counts) {
  const int b = blockIdx.x, id = threadIdx.x;
  const int ar = area[b * 256 + id];
  int v = DL_SKIP;
  if (ar > 0 && ar < min_count) {
    const long long* s = sums + ((size_t)b * 256 + id) * C;
    long long best = s[0];
    v = 0;
    for (int c = 1; c < C; ++c)
      if (s[c] > best) { best = s[c]; v = c; }
  }
  lut[b * 256 + id] = v;
  if (counts && id == 0) counts[b] = bad[b];
}

// ------------------------------------------------------------------------------------------------ 6. fill
__device__ __forceinline__ int dl_pixel(const uint8_t* __restrict__ m, const uint32_t* __restrict__ wb, const int64_t* __restrict__ refined,
                                        const int* lut, int64_t px) {
  const int v = lut[m[px]];
  if (v != DL_SKIP) return v;
  const uint32_t w = wb[px];
  return w ? (int)refined[w - 1u] : DL_IGNORE;
}

// One block = up to 4 * (DL_BLOCK - 1) pixels of one output row.  Thread 0 of the row's first block writes the pixels in front of
// the first 16-byte aligned address one by one; every other thread owns four pixels from an aligned address and writes them with
// one 16-byte store, or one by one at the row's end.
__global__ __launch_bounds__(DL_BLOCK) void k_dl_fill(const DlArgs a, int H, int W, const int32_t* __restrict__ lut_all,
                                                      const uint32_t* __restrict__ win, const int64_t* __restrict__ refined, int oh, int ow,
                                                      int32_t* __restrict__ dst) {
  __shared__ int lut[256];
  const int b = blockIdx.z, oy = blockIdx.y;
  lut[threadIdx.x] = lut_all[b * 256 + threadIdx.x];                       // DL_BLOCK == 256
  __syncthreads();
  const int64_t HW = (int64_t)H * W;
  const uint8_t* __restrict__ m = a.mask[b];
  const uint32_t* wb = win + (int64_t)b * HW;
  const int64_t* rf = refined + a.row0[b];
  int32_t* o = dst + ((int64_t)b * oh + oy) * ow;
  const int64_t src_row = (int64_t)(oy + a.top[b]) * W + a.left[b];
  const bool flip = a.flip[b] != 0;
  const int head = min((int)(((16 - (reinterpret_cast<uintptr_t>(o) & 15)) & 15) >> 2), ow);
  const int t = blockIdx.x * DL_BLOCK + threadIdx.x;                       // 0: the head; g >= 1: pixels head + 4 (g - 1) ...
  int x0, x1;
  if (t == 0) { x0 = 0; x1 = head; }
  else { x0 = head + 4 * (t - 1); x1 = min(x0 + 4, ow); }
  if (x0 >= x1) return;
  if (t > 0 && x1 - x0 == 4) {
    int4 v;
    v.x = dl_pixel(m, wb, rf, lut, src_row + (flip ? ow - 1 - x0 : x0));
    v.y = dl_pixel(m, wb, rf, lut, src_row + (flip ? ow - 2 - x0 : x0 + 1));
    v.z = dl_pixel(m, wb, rf, lut, src_row + (flip ? ow - 3 - x0 : x0 + 2));
    v.w = dl_pixel(m, wb, rf, lut, src_row + (flip ? ow - 4 - x0 : x0 + 3));
    *reinterpret_cast<int4*>(o + x0) = v;
  } else {
    for (int x = x0; x < x1; ++x) o[x] = dl_pixel(m, wb, rf, lut, src_row + (flip ? ow - 1 - x : x));
  }
}

// ------------------------------------------------------------------------------------------------ entry points
MOPA_API size_t mopa_denselabels_workspace_bytes(int B, int H, int W, int64_t n_total, int C) {
  if (B < 1 || B > DL_MAXB || H < 1 || W < 1 || n_total < 0 || C < 2 || C > DL_MAXC) return 0;
  return dl_layout(B, (int64_t)H * W, n_total, C).total;
}

// B images (at most 32) of one size H x W: prob_host[b] (n_b) float32 in [0, 1], label_host[b] (n_b) uint8, pts_host[b] (n_b, 2)
// [row, col] float32 (pts_dtype 0) or float64 (1), mask_host[b] (H, W) uint8 -> dst (B, oh, ow) int32: ids of fewer than
// min_count pixels are filled with the first arg-max of their summed winning rows, the pixels of the others keep the refined
// label of their last point or -100; then the crop window crop_host[b] = {top, left} (null: none, oh = H, ow = W) and the flip.
// counts (B) int32 or null: points that were skipped (outside the image, raw label >= C, probability outside [0, 1]).
// A fixed number of launches for every B, no read-back.
MOPA_API int mopa_denselabels(const void* const* prob_host, const void* const* label_host, const void* const* pts_host, int pts_dtype,
                              const int32_t* n_host, const void* const* mask_host, int B, int H, int W, int C, int min_count,
                              const int32_t* crop_host, int oh, int ow, const int32_t* flip_host, int32_t* dst, int32_t* counts,
                              void* ws, size_t ws_bytes, void* stream) {
  if (!prob_host || !label_host || !pts_host || !n_host || !mask_host || !dst || B < 1 || B > DL_MAXB || H < 1 || W < 1 ||
      (int64_t)H * W >= (1ll << 31) || C < 2 || C > DL_MAXC || oh < 1 || ow < 1 || oh > 65535 || pts_dtype < 0 || pts_dtype > 1)
    return MOPA_ERR_ARG;
  if (!crop_host && (oh != H || ow != W)) return MOPA_ERR_ARG;
  DlArgs a = {};
  int64_t n_total = 0;
  int nmax = 0;
  for (int b = 0; b < B; ++b) {
    if (!mask_host[b] || n_host[b] < 0 || (n_host[b] > 0 && (!prob_host[b] || !label_host[b] || !pts_host[b]))) return MOPA_ERR_ARG;
    a.prob[b] = (const float*)prob_host[b];
    a.label[b] = (const uint8_t*)label_host[b];
    a.pts[b] = pts_host[b];
    a.mask[b] = (const uint8_t*)mask_host[b];
    a.n[b] = n_host[b];
    a.top[b] = crop_host ? crop_host[2 * b] : 0;
    a.left[b] = crop_host ? crop_host[2 * b + 1] : 0;
    if (a.top[b] < 0 || a.left[b] < 0 || (int64_t)a.top[b] + oh > H || (int64_t)a.left[b] + ow > W) return MOPA_ERR_ARG;
    a.flip[b] = (flip_host && flip_host[b]) ? 1 : 0;
    if (n_total + n_host[b] >= (1ll << 31) - 1) return MOPA_ERR_ARG;
    a.row0[b] = (int32_t)n_total;
    n_total += n_host[b];
    nmax = n_host[b] > nmax ? n_host[b] : nmax;
  }
  const DlWs w = dl_layout(B, (int64_t)H * W, n_total, C);
  if (!ws || ws_bytes < w.total || ((uintptr_t)ws & 15)) return MOPA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  uint32_t* win = (uint32_t*)(base + w.win);
  int32_t* area = (int32_t*)(base + w.area);
  unsigned long long* sums = (unsigned long long*)(base + w.sums);
  int32_t* bad = (int32_t*)(base + w.bad);
  int32_t* lut = (int32_t*)(base + w.lut);
  float* conf = (float*)(base + w.conf);
  int32_t* lab = (int32_t*)(base + w.lab);
  int32_t* pix = (int32_t*)(base + w.pix);
  int64_t* refined = (int64_t*)(base + w.refined);
  if (hipMemsetAsync(base, 0, w.zero_bytes, st) != hipSuccess) return MOPA_ERR_LAUNCH;
  if (nmax > 0) {
    const int gx = (int)(cdiv64(nmax, DL_BLOCK) < 64 ? cdiv64(nmax, DL_BLOCK) : 64);
    hipLaunchKernelGGL(k_dl_points, dim3(gx, B), dim3(DL_BLOCK), 0, st, a, pts_dtype, H, W, C, conf, lab, pix, win, bad);
    MOPA_CHECK_LAUNCH();
    const void* ph[DL_MAXB];
    const void* lh[DL_MAXB];
    void* oh_[DL_MAXB];
    for (int b = 0; b < B; ++b) {
      ph[b] = conf + a.row0[b];
      lh[b] = lab + a.row0[b];
      oh_[b] = refined + a.row0[b];
    }
    const int rc = mopa_refine_pseudo_labels_segmented(ph, lh, 2, n_host, oh_, B, C, DL_IGNORE, base + w.refine_ws, w.refine_bytes, stream);
    if (rc != MOPA_OK) return rc;
  }
  const size_t lds = (size_t)256 * C * 8;
  hipLaunchKernelGGL(k_dl_stats, dim3(DL_STAT_BLOCKS, B), dim3(DL_BLOCK), lds, st, a, H, W, C, pix, refined, win, area, sums);
  MOPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dl_lookup, dim3(B), dim3(256), 0, st, C, min_count, area, (const long long*)sums, bad, lut, counts);
  MOPA_CHECK_LAUNCH();
  const int groups = 1 + (ow + 3) / 4 + 1;                                  // the head, the full groups, a partial one at the end
  hipLaunchKernelGGL(k_dl_fill, dim3((groups + DL_BLOCK - 1) / DL_BLOCK, oh, B), dim3(DL_BLOCK), 0, st, a, H, W, lut, win, refined, oh,
                     ow, dst);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
