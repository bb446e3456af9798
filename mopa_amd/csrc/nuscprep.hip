// nuScenes' offline preprocessing of a sweep on the device: for the B raw sweeps of a call the float64 lidar -> ego -> global ->
// ego(cam) -> camera chain, the intrinsics, the perspective divide, the float32 cast and the strict frustum test of
// map_pointcloud_to_image (mopa/data/nuscenes/projection.py:9-90), the detection labels painted from the 3D boxes
// (mopa/data/nuscenes/preprocess.py:116-126 with the devkit's points_in_box), ONE stable compaction of every per-point array
// (preprocess.py:111-114) and the ground mask of the dataset (mopa/data/nuscenes/nuscenes_dataloader.py:305-316).
//
// A fixed number of launches whatever B and the number of boxes are: every kernel covers all scans of the call, cut into blocks
// of NP_ROWS raw rows (segbatch.h: the block table, the counts and their scan).
//   0. k_np_setup    one thread per quaternion or box: a small device table (NP_SCAN doubles per scan: four rotation matrices,
//                    four translations, the 4x4 viewpad; NP_BOX doubles per box: p1, i, j, k, dot(i,i), dot(j,j), dot(k,k), the
//                    class, the rotation matrix).  The per-scan constants of 32 scans do not fit a kernel-argument block, and
//                    computing them here keeps the bits off the host's BLAS.
//   1. k_np_flags    one byte per raw row (1 = kept; this IS valid_mask) and the kept rows per block
//   2. ordered exclusive scan of the block counts (mopa_scan_exclusive_i32), then k_np_counts: Nk per scan for the one read-back
//   3. k_np_scatter  points, points_img [row, col], seg_labels (the box test, on kept points only, frames in LDS), ground
// The ground mask over the raw rows comes from mopa_kittiprep_ground (numpy's index semantics) or is the caller's own mask.
//
// Arithmetic (fixture G15): every product with a matrix is per output element the fused chain
// fma(a[K-1], b[K-1], ... fma(a1, b1, a0 * b0)), K = 3 (rotations, box corners), K = 4 (quaternion product, viewpad); the box
// test's dot(i, v) is the same K = 3 chain (the device's own: the reference's 1-D dot is not one fixed chain on its host, the
// fixture keeps every point away from the bounds or exactly on them); translations are plain adds / subtracts between the
// rotations, the divide and the square root are correctly rounded, the float32 cast comes before the frustum comparisons,
// depth > 0 is tested in float64.  All of it is spelled with __fma_rn / __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn: the compiler
// contracts nothing on its own.  No float atomics; counts are integers and the compaction is ordered -> deterministic.
#include "common.h"
#include "segbatch.h"

#define NP_MAXB 32             // scans per call
#define NP_ROWS 1024           // raw rows per block (256 threads x 4 tiles)
#define NP_TILES (NP_ROWS / 256)
#define NP_LDS_BOXES 64        // box frames per LDS chunk (64 x 16 doubles = 8 KB)
#define NP_CALIB 37            // input doubles per scan: 4 quaternions wxyz | 4 translations | K (3, 3) row-major
#define NP_BOXIN 11            // input doubles per box: centre | wlh | quaternion wxyz | class (-1: none)
#define NP_SCAN 64             // table doubles per scan: R[4][9] | t[4][3] | viewpad[16]
#define NP_FRAME 16            // p1 | i | j | k | ii, jj, kk | class
#define NP_BOX 25              // frame | R[9]

struct NpSeg {
  const float* scan[NP_MAXB];       // (n, cols) float32, x y z first
  SegTable<NP_MAXB> seg;            // rows and blocks of the call's flat raw numbering
  int32_t cols[NP_MAXB];
  int32_t box0[NP_MAXB + 1];        // first box of the scan in the call's box list
};

__device__ __forceinline__ double np_dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return __fma_rn(a2, b2, __fma_rn(a1, b1, __dmul_rn(a0, b0)));
}
__device__ __forceinline__ double np_dot4(double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3) {
  return __fma_rn(a3, b3, __fma_rn(a2, b2, __fma_rn(a1, b1, __dmul_rn(a0, b0))));
}
// pyquaternion's rotation_matrix: normalise unless |1 - q.q| < 1e-14, then (Q @ Qbar^T)[1:, 1:]
__device__ void np_rotation(const double* qin, double* R) {
  double q[4] = {qin[0], qin[1], qin[2], qin[3]};
  const double ss = np_dot4(q[0], q[1], q[2], q[3], q[0], q[1], q[2], q[3]);
  if (!(fabs(__dsub_rn(1.0, ss)) < 1e-14)) {
    const double nrm = __dsqrt_rn(ss);
    if (nrm > 0.0)
      for (int k = 0; k < 4; ++k) q[k] = __ddiv_rn(q[k], nrm);
  }
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double Q[4][4] = {{w, -x, -y, -z}, {x, w, -z, y}, {y, z, w, -x}, {z, -y, x, w}};
  const double Qb[4][4] = {{w, -x, -y, -z}, {x, w, z, -y}, {y, -z, w, x}, {z, y, -x, w}};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      R[3 * r + c] = np_dot4(Q[r + 1][0], Q[r + 1][1], Q[r + 1][2], Q[r + 1][3], Qb[c + 1][0], Qb[c + 1][1], Qb[c + 1][2], Qb[c + 1][3]);
}

// ------------------------------------------------------------------------------------------ 0. the table
// item < 4 B: quaternion `item & 3` of scan `item >> 2` (the first of a scan also copies the translations and builds viewpad);
// then one item per box
__global__ __launch_bounds__(64) void k_np_setup(const double* __restrict__ calib, const double* __restrict__ boxes, int B, int M,
                                                 double* __restrict__ table) {
  const int item = blockIdx.x * 64 + threadIdx.x;
  if (item < 4 * B) {
    const int s = item >> 2, w = item & 3;
    const double* c = calib + (int64_t)s * NP_CALIB;
    double* t = table + (int64_t)s * NP_SCAN;
    np_rotation(c + 4 * w, t + 9 * w);
    if (w == 0) {
      for (int k = 0; k < 12; ++k) t[36 + k] = c[16 + k];
      for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) t[48 + 4 * r + k] = (r < 3 && k < 3) ? c[28 + 3 * r + k] : (r == k ? 1.0 : 0.0);
    }
    return;
  }
  const int b = item - 4 * B;
  if (b >= M) return;
  const double* in = boxes + (int64_t)b * NP_BOXIN;
  double* f = table + (int64_t)B * NP_SCAN + (int64_t)b * NP_BOX;
  double R[9];
  np_rotation(in + 6, R);
  // Box.corners: x = l/2 [1,1,1,1,-1,-1,-1,-1], y = w/2 [1,-1,-1,1,1,-1,-1,1], z = h/2 [1,1,-1,-1,1,1,-1,-1]; wlh = [w, l, h]
  const double hx = __ddiv_rn(in[4], 2.0), hy = __ddiv_rn(in[3], 2.0), hz = __ddiv_rn(in[5], 2.0);
  // the corners points_in_box uses: 0 (+,+,+), 4 (-,+,+), 1 (+,-,+), 3 (+,+,-)
  const double sx[4] = {hx, -hx, hx, hx}, sy[4] = {hy, hy, -hy, hy}, sz[4] = {hz, hz, hz, -hz};
  double c[4][3];
  for (int k = 0; k < 4; ++k)
    for (int r = 0; r < 3; ++r) c[k][r] = __dadd_rn(np_dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], sx[k], sy[k], sz[k]), in[r]);
  for (int r = 0; r < 3; ++r) {
    f[r] = c[0][r];
    f[3 + r] = __dsub_rn(c[1][r], c[0][r]);
    f[6 + r] = __dsub_rn(c[2][r], c[0][r]);
    f[9 + r] = __dsub_rn(c[3][r], c[0][r]);
  }
  for (int a = 0; a < 3; ++a) f[12 + a] = np_dot3(f[3 + 3 * a], f[4 + 3 * a], f[5 + 3 * a], f[3 + 3 * a], f[4 + 3 * a], f[5 + 3 * a]);
  f[15] = in[10];
  for (int k = 0; k < 9; ++k) f[16 + k] = R[k];
}

// The chain of one point.  t: the scan's table.  -> kept; u (column), v (row) as float32
__device__ __forceinline__ bool np_project(const double* __restrict__ t, float w, float h, float xf, float yf, float zf, float& u, float& v) {
  double p[3] = {(double)xf, (double)yf, (double)zf}, q[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) q[r] = __dadd_rn(np_dot3(t[3 * r], t[3 * r + 1], t[3 * r + 2], p[0], p[1], p[2]), t[36 + r]);        // lidar -> ego
#pragma unroll
  for (int r = 0; r < 3; ++r) p[r] = __dadd_rn(np_dot3(t[9 + 3 * r], t[10 + 3 * r], t[11 + 3 * r], q[0], q[1], q[2]), t[39 + r]);   // ego -> global
#pragma unroll
  for (int r = 0; r < 3; ++r) p[r] = __dsub_rn(p[r], t[42 + r]);
#pragma unroll
  for (int r = 0; r < 3; ++r) q[r] = np_dot3(t[18 + r], t[21 + r], t[24 + r], p[0], p[1], p[2]);                                    // R^T: global -> ego(cam)
#pragma unroll
  for (int r = 0; r < 3; ++r) q[r] = __dsub_rn(q[r], t[45 + r]);
#pragma unroll
  for (int r = 0; r < 3; ++r) p[r] = np_dot3(t[27 + r], t[30 + r], t[33 + r], q[0], q[1], q[2]);                                    // R^T: ego -> camera
  double hh[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) hh[r] = np_dot4(t[48 + 4 * r], t[49 + 4 * r], t[50 + 4 * r], t[51 + 4 * r], p[0], p[1], p[2], 1.0);
  u = (float)__ddiv_rn(hh[0], hh[2]);
  v = (float)__ddiv_rn(hh[1], hh[2]);
  return p[2] > 0.0 && u > 0.f && u < w && v > 0.f && v < h;
}

// ------------------------------------------------------------------------------------------ 1. flags + block counts
// A raw row is `cols` floats (5 in a .pcd.bin: 20 bytes, so rows are only 4-byte aligned): three scalar loads per thread; the
// 64 rows of a wave lie in one contiguous stretch, so the three loads hit the same lines.
__global__ __launch_bounds__(256) void k_np_flags(const NpSeg a, int S, const double* __restrict__ table, float w, float h,
                                                  uint8_t* __restrict__ flags, int* __restrict__ cnt) {
  const int s = seg_of_block(a.seg.blk0, S, blockIdx.x);
  const int n = a.seg.n[s], cols = a.cols[s];
  const float* __restrict__ scan = a.scan[s];
  const double* __restrict__ t = table + (int64_t)s * NP_SCAN;
  const int base = (blockIdx.x - a.seg.blk0[s]) * NP_ROWS;
  int c[1] = {0};
#pragma unroll
  for (int tile = 0; tile < NP_TILES; ++tile) {
    const int i = base + tile * 256 + threadIdx.x;
    if (i < n) {
      const float* row = scan + (int64_t)i * cols;
      float u, v;
      const bool kept = np_project(t, w, h, row[0], row[1], row[2], u, v);
      flags[(int64_t)a.seg.row0[s] + i] = kept ? 1 : 0;
      c[0] += kept;
    }
  }
  block_counts(c, cnt, gridDim.x);
}
// counts[s] = Nk of scan s; counts[S] = ground indices outside their scan.  scan has nblk + 1 items: scan[nblk] is the total.
__global__ void k_np_counts(const NpSeg a, int S, const int* __restrict__ scan, const int* __restrict__ bad, int64_t* __restrict__ counts) {
  const int i = threadIdx.x;
  if (i < S) counts[i] = scan[a.seg.blk0[i + 1]] - scan[a.seg.blk0[i]];
  if (i == S) counts[S] = bad ? *bad : 0;
}

// ------------------------------------------------------------------------------------------ 3. compaction + box labels
__global__ __launch_bounds__(256) void k_np_scatter(const NpSeg a, int S, const double* __restrict__ table, float w, float h,
                                                    const uint8_t* __restrict__ flags, const uint8_t* __restrict__ gmask,
                                                    const int* __restrict__ scan, float* __restrict__ points, float2* __restrict__ img,
                                                    uint8_t* __restrict__ seg, uint8_t* __restrict__ ground) {
  __shared__ int lds[4];
  __shared__ double frames[NP_LDS_BOXES * NP_FRAME];
  const int s = seg_of_block(a.seg.blk0, S, blockIdx.x);
  const int n = a.seg.n[s], cols = a.cols[s];
  const float* __restrict__ src = a.scan[s];
  const double* __restrict__ t = table + (int64_t)s * NP_SCAN;
  const double* __restrict__ boxes = table + (int64_t)S * NP_SCAN + (int64_t)a.box0[s] * NP_BOX;
  const int m = a.box0[s + 1] - a.box0[s];
  const int base = (blockIdx.x - a.seg.blk0[s]) * NP_ROWS;
  float x[NP_TILES], y[NP_TILES], z[NP_TILES];
  bool kept[NP_TILES];
  int label[NP_TILES];
#pragma unroll
  for (int tile = 0; tile < NP_TILES; ++tile) {
    const int i = base + tile * 256 + threadIdx.x;
    kept[tile] = i < n && flags[(int64_t)a.seg.row0[s] + i];
    label[tile] = 10;
    x[tile] = y[tile] = z[tile] = 0.f;
    if (kept[tile]) {
      const float* row = src + (int64_t)i * cols;
      x[tile] = row[0]; y[tile] = row[1]; z[tile] = row[2];
    }
  }
  // the last box in input order that holds the point and has a class wins: ascending order, overwriting
  for (int c0 = 0; c0 < m; c0 += NP_LDS_BOXES) {
    const int mc = m - c0 < NP_LDS_BOXES ? m - c0 : NP_LDS_BOXES;
    __syncthreads();
    for (int e = threadIdx.x; e < mc * NP_FRAME; e += 256) frames[e] = boxes[(int64_t)(c0 + e / NP_FRAME) * NP_BOX + e % NP_FRAME];
    __syncthreads();
#pragma unroll
    for (int tile = 0; tile < NP_TILES; ++tile) {
      if (!kept[tile]) continue;
      for (int b = 0; b < mc; ++b) {
        const double* f = frames + b * NP_FRAME;
        if (f[15] < 0.0) continue;
        const double v0 = __dsub_rn((double)x[tile], f[0]), v1 = __dsub_rn((double)y[tile], f[1]), v2 = __dsub_rn((double)z[tile], f[2]);
        const double iv = np_dot3(f[3], f[4], f[5], v0, v1, v2);
        const double jv = np_dot3(f[6], f[7], f[8], v0, v1, v2);
        const double kv = np_dot3(f[9], f[10], f[11], v0, v1, v2);
        if (0.0 <= iv && iv <= f[12] && 0.0 <= jv && jv <= f[13] && 0.0 <= kv && kv <= f[14]) label[tile] = (int)f[15];
      }
    }
  }
  int64_t run = scan[blockIdx.x];
#pragma unroll
  for (int tile = 0; tile < NP_TILES; ++tile) {
    int tot;
    const int r = block_rank<256>(kept[tile], lds, tot);
    if (kept[tile]) {
      const int64_t kp = run + r;
      points[3 * kp] = x[tile]; points[3 * kp + 1] = y[tile]; points[3 * kp + 2] = z[tile];
      float u, v;
      np_project(t, w, h, x[tile], y[tile], z[tile], u, v);
      img[kp] = make_float2(v, u);                       // the reference's fliplr: [row, col]
      seg[kp] = (uint8_t)label[tile];
      if (ground) ground[kp] = gmask[(int64_t)a.seg.row0[s] + base + tile * 256 + threadIdx.x];
    }
    run += tot;
  }
}

// ------------------------------------------------------------------------------------------ entry points
static int np_scans(NpSeg& a, const void* const* scan_host, const int32_t* n_host, const int32_t* cols_host, int B) {
  const int nblk = seg_table_fill(a.seg, n_host, B, NP_ROWS);
  if (nblk < 0 || !scan_host || !cols_host) return -1;
  for (int s = 0; s < B; ++s) {
    if (cols_host[s] < 3 || (n_host[s] > 0 && (!scan_host[s] || ((uintptr_t)scan_host[s] & 3)))) return -1;
    a.scan[s] = (const float*)scan_host[s];
    a.cols[s] = cols_host[s];
  }
  return nblk;
}

MOPA_API int mopa_nuscprep_rows_per_block(void) { return NP_ROWS; }
MOPA_API int mopa_nuscprep_max_scans(void) { return NP_MAXB; }
// box frames per LDS chunk of the scatter kernel (a scan may have any number of boxes: it walks them chunk by chunk)
MOPA_API int mopa_nuscprep_max_boxes(void) { return NP_LDS_BOXES; }
// doubles of the device table for B scans with M boxes in all
MOPA_API size_t mopa_nuscprep_table_bytes(int32_t B, int64_t M) {
  if (B < 0 || M < 0) return 0;
  return ((size_t)B * NP_SCAN + (size_t)M * NP_BOX) * sizeof(double);
}
// workspace: the one count plane (kept rows) of segbatch.h's SegCounts
MOPA_API size_t mopa_nuscprep_workspace_bytes(int64_t total_blocks) {
  if (total_blocks < 0) return 0;
  return seg_counts_bytes(1, total_blocks);
}

// Stage 0.  calib (B, 37) float64 on the device: per scan the four quaternions wxyz (lidar2ego, ego2global of the lidar's pose,
// ego2global of the camera's pose, cam2ego), the four translations in the same order, the intrinsic (3, 3); boxes (M, 11) float64:
// centre, wlh, quaternion wxyz, class (-1: no detection class) -- the boxes of the scans one after the other.  table:
// mopa_nuscprep_table_bytes(B, M).
MOPA_API int mopa_nuscprep_setup(const double* calib, const double* boxes, int32_t B, int32_t M, double* table, void* stream) {
  if (!calib || B < 1 || B > NP_MAXB || M < 0 || (M > 0 && !boxes) || !table) return MOPA_ERR_ARG;
  const int items = 4 * B + M;
  k_np_setup<<<(int)cdiv64(items, 64), 64, 0, (hipStream_t)stream>>>(calib, boxes, B, M, table);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// Stages 1 + 2 for B scans ((n, cols) float32 each, cols >= 3): flags (sum n bytes, 1 = the row is kept: the valid_mask of the
// scans one after the other) and counts (B + 1 int64: Nk per scan, then *bad or 0), which the caller reads back to size the
// outputs.  The workspace carries the scan to mopa_nuscprep_scatter and must not be touched in between.
MOPA_API int mopa_nuscprep_count(const void* const* scan_host, const int32_t* n_host, const int32_t* cols_host, int32_t B, const double* table,
                                 int32_t width, int32_t height, uint8_t* flags, const int32_t* bad, int64_t* counts, void* ws,
                                 size_t ws_bytes, void* stream) {
  NpSeg a = {};
  const int nblk = np_scans(a, scan_host, n_host, cols_host, B);
  if (nblk < 0 || !table || !flags || !counts || !ws || width <= 0 || height <= 0) return MOPA_ERR_ARG;
  if (ws_bytes < mopa_nuscprep_workspace_bytes(nblk)) return MOPA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const SegCounts c = seg_counts(ws, 1, nblk);
  if (nblk > 0) k_np_flags<<<nblk, 256, 0, st>>>(a, B, table, (float)width, (float)height, flags, c.cnt);
  const int rc = seg_counts_scan(c, stream);
  if (rc) return rc;
  k_np_counts<<<1, 64, 0, st>>>(a, B, c.scan, bad, counts);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// Stage 3.  The outputs point at the first kept row of this call's scans: points (Nk, 3) float32, points_img (Nk, 2) float32
// [row, col], seg_labels (Nk,) uint8 (10 = no box; the class of the last box in input order that holds the point and has one),
// g_out (Nk,) 0/1 with gmask (sum n bytes over the raw rows).  boxoff_host: B + 1 offsets into the box list of the table that
// mopa_nuscprep_setup filled for the same B scans.  flags and the workspace are those of mopa_nuscprep_count.
MOPA_API int mopa_nuscprep_scatter(const void* const* scan_host, const int32_t* n_host, const int32_t* cols_host, const int32_t* boxoff_host,
                                   int32_t B, const double* table, int32_t width, int32_t height, const uint8_t* flags, const uint8_t* gmask,
                                   float* points, float* points_img, uint8_t* seg_labels, uint8_t* g_out, void* ws, size_t ws_bytes,
                                   void* stream) {
  NpSeg a = {};
  const int nblk = np_scans(a, scan_host, n_host, cols_host, B);
  if (nblk < 0 || !boxoff_host || !table || !flags || !points || !points_img || !seg_labels || !ws || width <= 0 || height <= 0) return MOPA_ERR_ARG;
  if ((gmask != nullptr) != (g_out != nullptr) || ((uintptr_t)points_img & 7)) return MOPA_ERR_ARG;
  if (boxoff_host[0] != 0) return MOPA_ERR_ARG;
  for (int s = 0; s <= B; ++s) {
    if (s > 0 && boxoff_host[s] < boxoff_host[s - 1]) return MOPA_ERR_ARG;
    a.box0[s] = boxoff_host[s];
  }
  if (ws_bytes < mopa_nuscprep_workspace_bytes(nblk)) return MOPA_ERR_WORKSPACE;
  if (nblk == 0) return MOPA_OK;
  k_np_scatter<<<nblk, 256, 0, (hipStream_t)stream>>>(a, B, table, (float)width, (float)height, flags, gmask, seg_counts(ws, 1, nblk).scan, points,
                                                     (float2*)points_img, seg_labels, g_out);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
