// SemanticKITTI's per-sample projection on the device: for the B raw scans of an iteration the `z > -3` filter, the low 16
// label bits, the ground mask, the front-half filter, `P2 @ Tr` times the homogeneous points, the perspective divide,
// np.around(., 2), the strict frustum test and ONE stable compaction of every per-point array -- what data_extraction and
// preprocess do per sample on the host (mopa/data/semantic_kitti/semantic_kitti_dataloader.py:349-371,422-507 with
// select_points_in_frustum :236-252).
//
// A fixed number of launches whatever B is: every kernel covers all scans of the call, cut into blocks of KP_ROWS raw rows
// (segbatch.h: the block table, the counts and their scan).  Per-scan pointers and matrices travel as kernel arguments (at most
// KP_MAXB scans per call; the binding splits larger batches).
//   1. k_kp_flags    one byte per raw row (bit 0: z > -3, bit 1: kept) and per block the two counts
//   2. ordered exclusive scan of the counts (mopa_scan_exclusive_i32), then k_kp_counts: [Nz, Nk] per scan for the one read-back
//   3. k_kp_scatter  every output, rows in the order of the scan
// The pseudo-label form projects nothing: the loaded mask over the z-filtered scan is the keep mask.  A row's position in the
// z-filtered scan is known only after the scan of the z counts, so that form runs k_kp_mask and the scan once more between 2
// and 3.  The ground mask is scattered over the raw rows by k_kp_ground from the index lists.
//
// Arithmetic (the bits numpy leaves on the reference's host, fixture G13): a row of the product is the fused chain
// fma(m3, 1, fma(m2, z, fma(m1, y, m0 * x))), the divide and the /100 are correctly rounded, rint rounds half to even, the
// comparisons are IEEE (a NaN from 0/0 and an infinity from x/0 fail them and the row is dropped).  No float atomics; counts are
// integers and the compaction is ordered -> deterministic.
#include "common.h"
#include "segbatch.h"

#define KP_MAXB 32             // scans per call
#define KP_ROWS 1024           // raw rows per block (256 threads x 4 tiles)

struct KpSeg {
  const float4* scan[KP_MAXB];      // (n, 4) float32: x, y, z, remission
  SegTable<KP_MAXB> seg;            // rows and blocks of the call's flat raw numbering
};
struct KpProj {
  float m[KP_MAXB][12];             // proj_matrix (3, 4), row-major
  float w, h;                       // image_size
};
struct KpMask {
  const uint8_t* mask[KP_MAXB];     // (len,) 0/1 over the z-filtered scan
  int32_t len[KP_MAXB];
};
struct KpGround {
  const int32_t* idx[KP_MAXB];      // (g,) indices into the raw scan
  int32_t g[KP_MAXB];
  SegTable<KP_MAXB> seg;
};
struct KpOut {
  const void* label[KP_MAXB];       // (n,) int32 / int64: the label file as loaded
  float* points;                    // (Nk, 3)
  float* feats;                     // (Nk, 1)
  int16_t* seg;                     // (Nk,)
  float2* img;                      // (Nk, 2) [row, col], or null (pseudo-label form)
  uint8_t* keep;                    // (Nz,)
  uint8_t* ground;                  // (Nk,) or null
  float* full_scan;                 // (Nz, 3) or null
  int16_t* all_seg;                 // (Nz,) or null
};

// img_points of one front-half point, rounded to cents, and the frustum test (u: column, v: row)
__device__ __forceinline__ bool kp_project(const float* m, float w, float h, float x, float y, float z, float& u, float& v) {
  float p[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    p[r] = __fmaf_rn(m[4 * r + 3], 1.f, __fmaf_rn(m[4 * r + 2], z, __fmaf_rn(m[4 * r + 1], y, __fmul_rn(m[4 * r], x))));
  u = __fdiv_rn(rintf(__fmul_rn(__fdiv_rn(p[0], p[2]), 100.f)), 100.f);
  v = __fdiv_rn(rintf(__fmul_rn(__fdiv_rn(p[1], p[2]), 100.f)), 100.f);
  return u > 0.f && v > 0.f && u < w && v < h;
}

// ------------------------------------------------------------------------------------------ 1. flags + block counts
// cnt[blk] = rows of the block with z > -3, cnt[nblk + blk] = kept rows of the block (0 without `project`: k_kp_mask sets them)
__global__ __launch_bounds__(256) void k_kp_flags(const KpSeg a, const KpProj pj, int S, int project, uint8_t* __restrict__ flags,
                                                  int* __restrict__ cnt, int nblk) {
  const int s = seg_of_block(a.seg.blk0, S, blockIdx.x);
  const int n = a.seg.n[s];
  const float4* __restrict__ scan = a.scan[s];
  float m[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) m[k] = pj.m[s][k];
  const int base = (blockIdx.x - a.seg.blk0[s]) * KP_ROWS;
  int c[2] = {0, 0};                // rows with z > -3, kept rows
#pragma unroll
  for (int t = 0; t < KP_ROWS / 256; ++t) {
    const int i = base + t * 256 + threadIdx.x;
    if (i < n) {
      const float4 q = scan[i];
      const bool zf = q.z > -3.f;
      bool kept = false;
      if (project && zf && q.x > 0.f) { float u, v; kept = kp_project(m, pj.w, pj.h, q.x, q.y, q.z, u, v); }
      flags[(int64_t)a.seg.row0[s] + i] = (uint8_t)((zf ? 1 : 0) | (kept ? 2 : 0));
      c[0] += zf;
      c[1] += kept;
    }
  }
  block_counts(c, cnt, nblk);
}
// The pseudo-label form: bit 1 of a z-filtered row = mask[its position in the z-filtered scan] (false past the mask's end: the
// binding refuses a mask of another length after the read-back).  scan = exclusive scan of cnt after k_kp_flags.
__global__ __launch_bounds__(256) void k_kp_mask(const KpSeg a, const KpMask mk, int S, uint8_t* __restrict__ flags,
                                                 const int* __restrict__ scan, int* __restrict__ cnt, int nblk) {
  __shared__ int lds[4];
  const int s = seg_of_block(a.seg.blk0, S, blockIdx.x);
  const int n = a.seg.n[s];
  const uint8_t* __restrict__ mask = mk.mask[s];
  const int len = mk.len[s];
  const int base = (blockIdx.x - a.seg.blk0[s]) * KP_ROWS;
  int run = scan[blockIdx.x] - scan[a.seg.blk0[s]];
  int c[2] = {0, 0};
#pragma unroll
  for (int t = 0; t < KP_ROWS / 256; ++t) {
    const int i = base + t * 256 + threadIdx.x;
    const int64_t row = (int64_t)a.seg.row0[s] + i;
    const bool zf = i < n && (flags[row] & 1);
    int tot;
    const int r = block_rank<256>(zf, lds, tot);
    if (zf) {
      const int zp = run + r;
      if (zp < len && mask[zp]) { flags[row] = 3; ++c[1]; }
    }
    run += tot;
  }
  block_counts(c, cnt, nblk, 2u);   // the kept plane only
}
// counts[2 s] = Nz, counts[2 s + 1] = Nk of scan s; counts[2 S] = ground indices outside their scan.  blk0[S] = nblk, and the
// scan has one item more than counts: scan[2 nblk] is the grand total.
__global__ void k_kp_counts(const KpSeg a, int S, const int* __restrict__ scan, int nblk, const int* __restrict__ bad,
                            int64_t* __restrict__ counts) {
  const int i = threadIdx.x;
  if (i < S) {
    counts[2 * i] = scan[a.seg.blk0[i + 1]] - scan[a.seg.blk0[i]];
    counts[2 * i + 1] = scan[nblk + a.seg.blk0[i + 1]] - scan[nblk + a.seg.blk0[i]];
  }
  if (i == S) counts[2 * S] = bad ? *bad : 0;
}

// ------------------------------------------------------------------------------------------ ground mask
// g_mask = zeros(n); g_mask[g_indices] = 1 (numpy's indexing: a negative index counts from the end; one outside is counted)
__global__ __launch_bounds__(256) void k_kp_ground(const KpGround a, uint8_t* __restrict__ gmask, int* __restrict__ bad) {
  const int s = blockIdx.y;
  const int g = a.g[s], n = a.seg.n[s];
  const int32_t* __restrict__ idx = a.idx[s];
  for (int j = blockIdx.x * 256 + threadIdx.x; j < g; j += gridDim.x * 256) {
    int64_t k = idx[j];
    if (k < 0) k += n;
    if (k < 0 || k >= n) atomicAdd(bad, 1);
    else gmask[(int64_t)a.seg.row0[s] + k] = 1;
  }
}

// ------------------------------------------------------------------------------------------ 3. compaction
// A row with bit 0 goes to position scan[blk] + rank of the flat z-filtered numbering, one with bit 1 to scan[nblk + blk] -
// scan[nblk] + rank of the flat kept numbering (the outputs of the scans of a call follow each other).
__global__ __launch_bounds__(256) void k_kp_scatter(const KpSeg a, const KpProj pj, const KpOut o, int S, int label_i64,
                                                    const uint8_t* __restrict__ flags, const uint8_t* __restrict__ gmask,
                                                    const int* __restrict__ scan, int nblk) {
  __shared__ int lds[4];
  const int s = seg_of_block(a.seg.blk0, S, blockIdx.x);
  const int n = a.seg.n[s];
  const float4* __restrict__ src = a.scan[s];
  const void* label = o.label[s];
  float m[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) m[k] = pj.m[s][k];
  const int base = (blockIdx.x - a.seg.blk0[s]) * KP_ROWS;
  int64_t runz = scan[blockIdx.x], runk = (int64_t)scan[nblk + blockIdx.x] - scan[nblk];
#pragma unroll
  for (int t = 0; t < KP_ROWS / 256; ++t) {
    const int i = base + t * 256 + threadIdx.x;
    const int64_t row = (int64_t)a.seg.row0[s] + i;
    const uint8_t fl = i < n ? flags[row] : 0;
    int totz, totk;
    const int rz = block_rank<256>(fl & 1, lds, totz);
    const int rk = block_rank<256>(fl & 2, lds, totk);
    if (fl & 1) {
      const float4 q = src[i];
      const int64_t raw = label_i64 ? ((const int64_t*)label)[i] : (int64_t)((const int32_t*)label)[i];
      const int16_t lab = (int16_t)(uint16_t)(raw & 0xFFFF);
      const int64_t zp = runz + rz;
      o.keep[zp] = (fl >> 1) & 1;
      if (o.full_scan) {
        o.full_scan[3 * zp] = q.x; o.full_scan[3 * zp + 1] = q.y; o.full_scan[3 * zp + 2] = q.z;
        o.all_seg[zp] = lab;
      }
      if (fl & 2) {
        const int64_t kp = runk + rk;
        o.points[3 * kp] = q.x; o.points[3 * kp + 1] = q.y; o.points[3 * kp + 2] = q.z;
        o.feats[kp] = q.w;
        o.seg[kp] = lab;
        if (o.img) {
          float u, v;
          kp_project(m, pj.w, pj.h, q.x, q.y, q.z, u, v);
          o.img[kp] = make_float2(v, u);             // the reference's fliplr: [row, col]
        }
        if (o.ground) o.ground[kp] = gmask[row];
      }
    }
    runz += totz;
    runk += totk;
  }
}

// ------------------------------------------------------------------------------------------ entry points
static int kp_scans(KpSeg& a, const void* const* scan_host, const int32_t* n_host, int B) {
  const int nblk = seg_table_fill(a.seg, n_host, B, KP_ROWS);
  if (nblk < 0 || !scan_host) return -1;
  for (int s = 0; s < B; ++s) {
    if (n_host[s] > 0 && (!scan_host[s] || ((uintptr_t)scan_host[s] & 15))) return -1;
    a.scan[s] = (const float4*)scan_host[s];
  }
  return nblk;
}
static void kp_proj(KpProj& pj, const float* proj_host, int B, int width, int height) {
  for (int s = 0; s < B; ++s)
    for (int k = 0; k < 12; ++k) pj.m[s][k] = proj_host ? proj_host[12 * s + k] : 0.f;
  pj.w = (float)width;
  pj.h = (float)height;
}

MOPA_API int mopa_kittiprep_rows_per_block(void) { return KP_ROWS; }
MOPA_API int mopa_kittiprep_max_scans(void) { return KP_MAXB; }
// workspace: the two count planes (z > -3, kept) of segbatch.h's SegCounts
MOPA_API size_t mopa_kittiprep_workspace_bytes(int64_t total_blocks) {
  if (total_blocks < 0) return 0;
  return seg_counts_bytes(2, total_blocks);
}

// The ground mask of B scans over the call's flat raw numbering: gmask (sum n bytes) is cleared, then gmask[row0[s] + i] = 1 for
// every i of gidx_host[s] (g_host[s] int32 indices into scan s); *bad = number of indices outside their scan.
MOPA_API int mopa_kittiprep_ground(const void* const* gidx_host, const int32_t* g_host, const int32_t* n_host, int32_t B, uint8_t* gmask,
                                   int32_t* bad, void* stream) {
  KpGround a = {};
  if (!gidx_host || !g_host || seg_table_fill(a.seg, n_host, B, KP_ROWS) < 0 || !gmask || !bad) return MOPA_ERR_ARG;
  const int64_t row = a.seg.row0[B];
  int gmax = 0;
  for (int s = 0; s < B; ++s) {
    if (g_host[s] < 0 || (g_host[s] > 0 && !gidx_host[s])) return MOPA_ERR_ARG;
    a.idx[s] = (const int32_t*)gidx_host[s];
    a.g[s] = g_host[s];
    gmax = g_host[s] > gmax ? g_host[s] : gmax;
  }
  hipStream_t st = (hipStream_t)stream;
  if (row > 0 && hipMemsetAsync(gmask, 0, (size_t)row, st) != hipSuccess) return MOPA_ERR_LAUNCH;
  if (hipMemsetAsync(bad, 0, sizeof(int32_t), st) != hipSuccess) return MOPA_ERR_LAUNCH;
  if (gmax == 0) return MOPA_OK;
  const int gx = (int)(cdiv64(gmax, 256) < 64 ? cdiv64(gmax, 256) : 64);
  k_kp_ground<<<dim3(gx, B), 256, 0, st>>>(a, gmask, bad);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// Stages 1 + 2 for B scans: flags (sum n bytes) and counts (2 B + 1 int64: [Nz, Nk] per scan, then *bad or 0), which the caller
// reads back to size the outputs.  Exactly one of proj_host ([B][12] float32: the frustum form, image width x height) and
// mask_host / mask_n_host (B loaded keep masks over the z-filtered scans and their lengths: the pseudo-label form) is given.  The
// workspace carries the scan to mopa_kittiprep_scatter and must not be touched in between.
MOPA_API int mopa_kittiprep_count(const void* const* scan_host, const int32_t* n_host, const float* proj_host, const void* const* mask_host,
                                  const int32_t* mask_n_host, int32_t B, int32_t width, int32_t height, uint8_t* flags, const int32_t* bad,
                                  int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  KpSeg a = {};
  const int nblk = kp_scans(a, scan_host, n_host, B);
  if (nblk < 0 || !flags || !counts || !ws || (proj_host != nullptr) == (mask_host != nullptr) || (mask_host && !mask_n_host)) return MOPA_ERR_ARG;
  if (proj_host && (width <= 0 || height <= 0)) return MOPA_ERR_ARG;
  if (ws_bytes < mopa_kittiprep_workspace_bytes(nblk)) return MOPA_ERR_WORKSPACE;
  KpProj pj = {};
  kp_proj(pj, proj_host, B, width, height);
  KpMask mk = {};
  if (mask_host)
    for (int s = 0; s < B; ++s) {
      if (mask_n_host[s] < 0 || (mask_n_host[s] > 0 && !mask_host[s])) return MOPA_ERR_ARG;
      mk.mask[s] = (const uint8_t*)mask_host[s];
      mk.len[s] = mask_n_host[s];
    }
  hipStream_t st = (hipStream_t)stream;
  const SegCounts c = seg_counts(ws, 2, nblk);
  // the kept counts of the pseudo-label form are zero until k_kp_mask
  if (nblk > 0) k_kp_flags<<<nblk, 256, 0, st>>>(a, pj, B, proj_host != nullptr, flags, c.cnt, nblk);
  int rc = seg_counts_scan(c, stream);
  if (rc) return rc;
  if (mask_host && nblk > 0) {
    k_kp_mask<<<nblk, 256, 0, st>>>(a, mk, B, flags, c.scan, c.cnt, nblk);
    rc = seg_counts_scan(c, stream, false);
    if (rc) return rc;
  }
  k_kp_counts<<<1, 64, 0, st>>>(a, B, c.scan, nblk, bad, counts);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// Stage 3.  The outputs point at the first row of this call's scans: points (Nk, 3), feats (Nk,), seg_labels (Nk,) int16 and
// ori_keep_idx (Nz,) 0/1 always; points_img (Nk, 2) [row, col] with proj_host (null: the pseudo-label form, nothing is projected);
// g_out (Nk,) 0/1 with gmask; full_scan (Nz, 3) and all_seg (Nz,) int16 together or not at all.  label_host: B arrays of int32
// (label_i64 = 0) or int64 ids as loaded.  flags and the workspace are those of mopa_kittiprep_count for the same scans.
MOPA_API int mopa_kittiprep_scatter(const void* const* scan_host, const void* const* label_host, int32_t label_i64, const int32_t* n_host,
                                    const float* proj_host, int32_t B, int32_t width, int32_t height, const uint8_t* flags,
                                    const uint8_t* gmask, float* points, float* feats, int16_t* seg_labels, float* points_img,
                                    uint8_t* ori_keep_idx, uint8_t* g_out, float* full_scan, int16_t* all_seg, void* ws, size_t ws_bytes,
                                    void* stream) {
  KpSeg a = {};
  const int nblk = kp_scans(a, scan_host, n_host, B);
  if (nblk < 0 || !label_host || !flags || !points || !feats || !seg_labels || !ori_keep_idx || !ws) return MOPA_ERR_ARG;
  if ((proj_host != nullptr) != (points_img != nullptr) || (gmask != nullptr) != (g_out != nullptr) || (full_scan != nullptr) != (all_seg != nullptr))
    return MOPA_ERR_ARG;
  if (((uintptr_t)points_img & 7)) return MOPA_ERR_ARG;
  if (ws_bytes < mopa_kittiprep_workspace_bytes(nblk)) return MOPA_ERR_WORKSPACE;
  KpProj pj = {};
  kp_proj(pj, proj_host, B, width, height);
  KpOut o = {};
  for (int s = 0; s < B; ++s) {
    if (n_host[s] > 0 && (!label_host[s] || ((uintptr_t)label_host[s] & (label_i64 ? 7 : 3)))) return MOPA_ERR_ARG;
    o.label[s] = label_host[s];
  }
  o.points = points; o.feats = feats; o.seg = seg_labels; o.img = (float2*)points_img; o.keep = ori_keep_idx; o.ground = g_out;
  o.full_scan = full_scan; o.all_seg = all_seg;
  if (nblk == 0) return MOPA_OK;
  k_kp_scatter<<<nblk, 256, 0, (hipStream_t)stream>>>(a, pj, o, B, label_i64, flags, gmask, seg_counts(ws, 2, nblk).scan, nblk);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
