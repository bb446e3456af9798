// Ground estimation on the device: a per-point ground mask for the B scans of an iteration, so that Valid Ground-based Insertion
// (vgi.hip) needs no offline mask.  The algorithm is the published Patchwork core as DESIGN.md section 4 states it -- a concentric
// zone model of 504 patches, per patch a plane fitted from the lowest points (LPR, seed set, num_iter rounds of fit + classify) and
// three tests on the final fit (uprightness, elevation, flatness) -- and NOT Patchwork++: no adaptive thresholds across frames, no
// reflected-noise removal beyond the zone-0 cut, no vertical-plane fitting, no temporal revert.  The yardstick is the float64 numpy
// restatement tests/_ground_reference.py.
//
// A fixed number of launches whatever B is: every kernel covers all scans of the call.  The scans are the segments of ONE (sum N,
// cols) float32 array; a small device table holds row0[B + 1] (first row of a scan) and blk0[B + 1] (first block of a scan: a scan
// is cut into blocks of GR_ROWS rows).  No read-back, no allocation, no float atomics.
//   1. k_gr_bin     patch id per point (int16, -1 = in no patch), mask cleared, per block the count of every patch
//   2. ordered exclusive scan of the counts laid out [scan][patch][block] (mopa_scan_exclusive_i32): where every (patch, block)
//      run starts in the ordering, and with it where every patch starts and ends
//   3. k_gr_order   the ordering: the rows of a scan sorted by patch, stable in point order (ranks by ballot inside a wave, the
//      waves of a block one after the other: the order inside a patch is fixed by construction)
//   4. k_gr_fit     one workgroup per (scan, patch): LPR, seeds, the fit rounds and the tests without leaving the kernel; a patch
//      of at most GR_CAP points is held in LDS (24 KiB: six workgroups per CU), a larger one is streamed from memory through
//      the ordering.  Sums in float64 in a fixed order (per thread in patch order, a fixed shuffle tree, the waves in order); set
//      membership is never stored, it is the previous round's predicate evaluated again by the same expression.  The 3x3
//      eigenproblem: cyclic Jacobi, GR_SWEEPS sweeps, by one thread per workgroup.
// Arithmetic is float64 after loading and is evaluated as written (no contraction into fused multiply-adds).
#include "common.h"
#include "segbatch.h"

#pragma clang fp contract(off)

#define GR_PATCHES 504
#define GR_ROWS 1024           // rows per block of passes 1 and 3
#define GR_THREADS 256         // passes 1 and 3
#ifndef GR_CAP
#define GR_CAP 2048            // points of a patch that stay in LDS (3 x 4 bytes each); measured, profiles/r21_ground.md (-D for its A/B builds)
#endif
#ifndef GR_FIT_THREADS
#define GR_FIT_THREADS 256     // workgroup of the fit
#endif
#define GR_SWEEPS 10
#define GR_NPARAM 18

struct GrParams {
  double h, rmin, rmax, th_seeds, th_dist, upright, noise_cut;
  double elev[4], flat[4];
  int num_min_pts, num_lpr, num_iter;
  double b[5];                 // zone bounds
};
__device__ __constant__ const int GR_RINGS[4] = {2, 4, 4, 4};
__device__ __constant__ const int GR_SECTORS[4] = {16, 32, 54, 32};
__device__ __constant__ const int GR_PATCH0[5] = {0, 32, 160, 376, 504};
__device__ __constant__ const int GR_RING0[4] = {0, 2, 6, 10};

__device__ __forceinline__ int gr_patch_of(float xf, float yf, float zf, const GrParams& P) {
  if (!(isfinite(xf) && isfinite(yf) && isfinite(zf))) return -1;
  const double x = xf, y = yf, z = zf;
  const double r = sqrt(x * x + y * y);
  if (!(r >= P.b[0] && r < P.b[4])) return -1;
  double th = atan2(y, x);
  if (th < 0) th = th + 2 * M_PI;
  const int k = r < P.b[1] ? 0 : r < P.b[2] ? 1 : r < P.b[3] ? 2 : 3;
  if (k == 0 && z < -P.noise_cut * P.h) return -1;
  const double rw = (P.b[k + 1] - P.b[k]) / GR_RINGS[k];
  const double sa = 2 * M_PI / GR_SECTORS[k];
  int ring = (int)((r - P.b[k]) / rw);
  int sector = (int)(th / sa);
  ring = ring < GR_RINGS[k] - 1 ? ring : GR_RINGS[k] - 1;
  sector = sector < GR_SECTORS[k] - 1 ? sector : GR_SECTORS[k] - 1;
  return GR_PATCH0[k] + ring * GR_SECTORS[k] + sector;
}

// ------------------------------------------------------------------------------------------ 1. patch ids + block counts
// cnt[504 blk0[s] + p nb_s + (blk - blk0[s])] = points of patch p in the block (nb_s = blocks of scan s)
__global__ __launch_bounds__(GR_THREADS) void k_gr_bin(const float* __restrict__ pts, int cols, const int32_t* __restrict__ tab, int B,
                                                       int64_t total, const GrParams P, int16_t* __restrict__ pid,
                                                       uint8_t* __restrict__ mask, int* __restrict__ cnt) {
  __shared__ int hist[GR_PATCHES];
  const int32_t* row0 = tab;
  const int32_t* blk0 = tab + B + 1;
  const int s = seg_of_block(blk0, B, blockIdx.x);
  const int n = row0[s + 1] - row0[s];
  const int lb = blockIdx.x - blk0[s];
  const int nb = blk0[s + 1] <= (int)gridDim.x ? blk0[s + 1] - blk0[s] : 0;      // a table that names blocks past the grid is refused
  for (int p = threadIdx.x; p < GR_PATCHES; p += GR_THREADS) hist[p] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[(int64_t)GR_PATCHES * gridDim.x] = 0;   // so that scan[504 nblk], the grand total, exists
  __syncthreads();
  if (lb < nb) {
#pragma unroll
    for (int t = 0; t < GR_ROWS / GR_THREADS; ++t) {
      const int i = lb * GR_ROWS + t * GR_THREADS + threadIdx.x;
      const int64_t row = (int64_t)row0[s] + i;
      if (i < n && row >= 0 && row < total) {
        const float* q = pts + row * cols;
        const int p = gr_patch_of(q[0], q[1], q[2], P);
        pid[row] = (int16_t)p;
        mask[row] = 0;
        if (p >= 0) atomicAdd(&hist[p], 1);          // integer counts: the result does not depend on the order
      }
    }
  }
  __syncthreads();
  if (lb < nb)
    for (int p = threadIdx.x; p < GR_PATCHES; p += GR_THREADS) cnt[(int64_t)GR_PATCHES * blk0[s] + (int64_t)p * nb + lb] = hist[p];
}

// ------------------------------------------------------------------------------------------ 3. the ordering
// order[scan[...] + rank] = flat row; rank = the point's position among the block's points of its patch, in point order.  The
// waves of a block take their GR_ROWS / 4 rows one after the other (wave w waits for wave w - 1 at the barriers).
__global__ __launch_bounds__(GR_THREADS) void k_gr_order(const int32_t* __restrict__ tab, int B, int64_t total,
                                                         const int16_t* __restrict__ pid, const int* __restrict__ scan,
                                                         int* __restrict__ order) {
  __shared__ int run[GR_PATCHES];
  const int32_t* row0 = tab;
  const int32_t* blk0 = tab + B + 1;
  const int s = seg_of_block(blk0, B, blockIdx.x);
  const int n = row0[s + 1] - row0[s];
  const int lb = blockIdx.x - blk0[s];
  const int nb = blk0[s + 1] <= (int)gridDim.x ? blk0[s + 1] - blk0[s] : 0;
  if (lb >= nb) return;                                // uniform over the block
  for (int p = threadIdx.x; p < GR_PATCHES; p += GR_THREADS) run[p] = scan[(int64_t)GR_PATCHES * blk0[s] + (int64_t)p * nb + lb];
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  constexpr int WROWS = GR_ROWS / (GR_THREADS / 64);   // consecutive rows of one wave
  for (int turn = 0; turn < GR_THREADS / 64; ++turn) {
    if (w == turn) {
      for (int t = 0; t < WROWS / 64; ++t) {
        const int i = lb * GR_ROWS + w * WROWS + t * 64 + lane;
        const int64_t row = (int64_t)row0[s] + i;
        const int p = (i < n && row >= 0 && row < total) ? (int)pid[row] : -1;
        bool todo = p >= 0;
        unsigned long long act = __ballot(todo);
        while (act) {                                  // uniform over the wave: one round per distinct patch among the 64 rows
          const int k = __shfl(p, __ffsll((long long)act) - 1);
          const bool mine = todo && p == k;
          const unsigned long long m = __ballot(mine);
          const int at = run[k];
          if (mine) {
            const int64_t dst = (int64_t)at + __popcll(m & below);
            if (dst >= 0 && dst < total) order[dst] = (int)row;
            todo = false;
          }
          __builtin_amdgcn_wave_barrier();
          if (lane == __ffsll((long long)m) - 1) run[k] = at + __popcll(m);
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          act = __ballot(todo);
        }
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------ 4. the fit
// float <-> a uint32 that orders like the float (no NaN reaches here)
__device__ __forceinline__ uint32_t gr_ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gr_unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// sums of K doubles over the workgroup, the same value in every thread: shuffle tree inside a wave, then the waves in order
template <int K>
__device__ __forceinline__ void gr_block_sum(double (&v)[K], double (*red)[10]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = wave_sum_d(v[k]);
    if (lane == 0) red[w][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double t = red[0][k];
#pragma unroll
    for (int u = 1; u < GR_FIT_THREADS / 64; ++u) t = t + red[u][k];
    v[k] = t;
  }
  __syncthreads();
}
__device__ __forceinline__ unsigned long long gr_block_min(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long m = red[0];
#pragma unroll
  for (int k = 1; k < GR_FIT_THREADS / 64; ++k) m = red[k] < m ? red[k] : m;
  __syncthreads();
  return m;
}

// The current set: the seeds (z < zthr) or the points below the previous plane (nrm . p - nrm . mu < th_dist).
struct GrSet {
  int plane;
  double zthr, nx, ny, nz, dmu, th_dist;
};
__device__ __forceinline__ bool gr_in(const GrSet& q, double x, double y, double z) {
  if (!q.plane) return z < q.zthr;
  return ((q.nx * x + q.ny * y) + q.nz * z) - q.dmu < q.th_dist;
}

// One Jacobi rotation of the symmetric matrix in the (p, q) plane; r is the third index.  Numerical Recipes' update.
#define GR_ROT(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                 \
  if (apq != 0.0) {                                                                  \
    const double theta = (aqq - app) / (2.0 * apq);                                  \
    const double t = (theta < 0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0)); \
    const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c, tau = sn / (1.0 + c);       \
    const double h_ = t * apq;                                                       \
    app = app - h_; aqq = aqq + h_; apq = 0.0;                                       \
    { const double g_ = arp, k_ = arq; arp = g_ - sn * (k_ + g_ * tau); arq = k_ + sn * (g_ - k_ * tau); } \
    { const double g_ = v0p, k_ = v0q; v0p = g_ - sn * (k_ + g_ * tau); v0q = k_ + sn * (g_ - k_ * tau); } \
    { const double g_ = v1p, k_ = v1q; v1p = g_ - sn * (k_ + g_ * tau); v1q = k_ + sn * (g_ - k_ * tau); } \
    { const double g_ = v2p, k_ = v2q; v2p = g_ - sn * (k_ + g_ * tau); v2q = k_ + sn * (g_ - k_ * tau); } \
  }

// eig[0..2] = eigenvalues ascending, eig[3..5] = unit eigenvector of the smallest, z component >= 0
__device__ void gr_jacobi(const double* c6, double* eig) {
  double a00 = c6[0], a01 = c6[1], a02 = c6[2], a11 = c6[3], a12 = c6[4], a22 = c6[5];
  double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
  for (int sweep = 0; sweep < GR_SWEEPS; ++sweep) {
    GR_ROT(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
    GR_ROT(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
    GR_ROT(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
  }
  double l0 = a00, l1 = a11, l2 = a22, nx = v00, ny = v10, nz = v20;
  if (l1 < l0) { const double t = l0; l0 = l1; l1 = t; nx = v01; ny = v11; nz = v21; }
  if (l2 < l0) { const double t = l0; l0 = l2; l2 = t; nx = v02; ny = v12; nz = v22; }
  if (l2 < l1) { const double t = l1; l1 = l2; l2 = t; }
  if (nz < 0) { nx = -nx; ny = -ny; nz = -nz; }
  eig[0] = l0; eig[1] = l1; eig[2] = l2; eig[3] = nx; eig[4] = ny; eig[5] = nz;
}

struct GrLds {
  float x[GR_CAP], y[GR_CAP], z[GR_CAP];
  double red[GR_FIT_THREADS / 64][10];
  unsigned long long redm[GR_FIT_THREADS / 64];
  double eig[6];
};

// RES: the patch is in LDS; else every pass reads the points through the ordering
template <bool RES>
__device__ __forceinline__ void gr_point(const GrLds& L, const float* __restrict__ pts, int cols, const int* __restrict__ ord, int j,
                                         double& x, double& y, double& z) {
  if (RES) { x = L.x[j]; y = L.y[j]; z = L.z[j]; }
  else { const float* q = pts + (int64_t)ord[j] * cols; x = q[0]; y = q[1]; z = q[2]; }
}

// Plane through the set `q` of the patch: m < 3 -> false (uniform over the workgroup), else mu[3] and L.eig.
template <bool RES>
__device__ bool gr_fit(GrLds& L, const float* __restrict__ pts, int cols, const int* __restrict__ ord, int n, const GrSet& q, double* mu) {
  double s[4] = {0, 0, 0, 0};
  for (int j = threadIdx.x; j < n; j += GR_FIT_THREADS) {
    double x, y, z;
    gr_point<RES>(L, pts, cols, ord, j, x, y, z);
    if (gr_in(q, x, y, z)) { s[0] += x; s[1] += y; s[2] += z; s[3] += 1.0; }
  }
  gr_block_sum<4>(s, L.red);
  const double m = s[3];
  if (m < 3.0) return false;
  mu[0] = s[0] / m; mu[1] = s[1] / m; mu[2] = s[2] / m;
  double c[6] = {0, 0, 0, 0, 0, 0};
  for (int j = threadIdx.x; j < n; j += GR_FIT_THREADS) {
    double x, y, z;
    gr_point<RES>(L, pts, cols, ord, j, x, y, z);
    if (gr_in(q, x, y, z)) {
      const double dx = x - mu[0], dy = y - mu[1], dz = z - mu[2];
      c[0] += dx * dx; c[1] += dx * dy; c[2] += dx * dz; c[3] += dy * dy; c[4] += dy * dz; c[5] += dz * dz;
    }
  }
  gr_block_sum<6>(c, L.red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = c[k] / (m - 1.0);
    gr_jacobi(c, L.eig);
  }
  __syncthreads();
  return true;
}

template <bool RES>
__device__ void gr_patch(GrLds& L, const float* __restrict__ pts, int cols, const int* __restrict__ ord, int n, int g, const GrParams& P,
                         uint8_t* __restrict__ mask) {
  if (RES) {
    for (int j = threadIdx.x; j < n; j += GR_FIT_THREADS) {
      const float* q = pts + (int64_t)ord[j] * cols;
      L.x[j] = q[0]; L.y[j] = q[1]; L.z[j] = q[2];
    }
    __syncthreads();
  }
  // LPR: the mean of the lowest z, taken one by one in ascending (z, position) order
  const int nl = P.num_lpr < n ? P.num_lpr : n;
  unsigned long long lo = 0;
  double zsum = 0;
  for (int t = 0; t < nl; ++t) {
    unsigned long long best = ~0ull;
    for (int j = threadIdx.x; j < n; j += GR_FIT_THREADS) {
      const float z = RES ? L.z[j] : pts[(int64_t)ord[j] * cols + 2];
      const unsigned long long key = ((unsigned long long)gr_ord(z) << 32) | (unsigned)j;
      if (key >= lo && key < best) best = key;
    }
    best = gr_block_min(best, L.redm);
    zsum += (double)gr_unord((uint32_t)(best >> 32));
    lo = best + 1;
  }
  GrSet q;
  q.plane = 0;
  q.zthr = zsum / nl + P.th_seeds;
  q.th_dist = P.th_dist;
  q.nx = q.ny = q.nz = q.dmu = 0;
  double mu[3];
  for (int it = 0; it < P.num_iter; ++it) {
    if (!gr_fit<RES>(L, pts, cols, ord, n, q, mu)) return;
    const double nx = L.eig[3], ny = L.eig[4], nz = L.eig[5];
    __syncthreads();                                   // L.eig is rewritten by the next fit
    q.plane = 1;
    q.nx = nx; q.ny = ny; q.nz = nz;
    q.dmu = (nx * mu[0] + ny * mu[1]) + nz * mu[2];
  }
  if (!gr_fit<RES>(L, pts, cols, ord, n, q, mu)) return;
  const double l0 = L.eig[0], l1 = L.eig[1], l2 = L.eig[2], nz = L.eig[5];
  bool ok = nz >= P.upright;
  if (g < 4 && mu[2] > -P.h + P.elev[g]) ok = ok && (l0 / ((l0 + l1) + l2) < P.flat[g]);
  if (!ok) return;
  for (int j = threadIdx.x; j < n; j += GR_FIT_THREADS) {
    double x, y, z;
    gr_point<RES>(L, pts, cols, ord, j, x, y, z);
    if (gr_in(q, x, y, z)) mask[ord[j]] = 1;
  }
}

__global__ __launch_bounds__(GR_FIT_THREADS) void k_gr_fit(const float* __restrict__ pts, int cols, const int32_t* __restrict__ tab, int B,
                                                       int64_t total, int nblk, const GrParams P, const int* __restrict__ scan,
                                                       const int* __restrict__ order, uint8_t* __restrict__ mask) {
  __shared__ GrLds L;
  const int s = blockIdx.y, p = blockIdx.x;
  const int32_t* blk0 = tab + B + 1;
  if (blk0[s] < 0 || blk0[s + 1] < blk0[s] || blk0[s + 1] > nblk) return;
  const int nb = blk0[s + 1] - blk0[s];
  const int64_t at = (int64_t)GR_PATCHES * blk0[s] + (int64_t)p * nb;
  const int64_t start = scan[at], end = scan[at + nb];     // at + nb: the next patch, the next scan or the grand total
  if (start < 0 || end > total || end - start < P.num_min_pts) return;
  const int n = (int)(end - start);
  int k = 0;
  while (p >= GR_PATCH0[k + 1]) ++k;
  const int g = GR_RING0[k] + (p - GR_PATCH0[k]) / GR_SECTORS[k];
  if (n <= GR_CAP) gr_patch<true>(L, pts, cols, order + start, n, g, P, mask);
  else gr_patch<false>(L, pts, cols, order + start, n, g, P, mask);
}

// ------------------------------------------------------------------------------------------ entry points
MOPA_API int mopa_ground_patches(void) { return GR_PATCHES; }
MOPA_API int mopa_ground_rows_per_block(void) { return GR_ROWS; }
MOPA_API int mopa_ground_resident_capacity(void) { return GR_CAP; }
MOPA_API int mopa_ground_num_params(void) { return GR_NPARAM; }

// workspace: pid [rows] int16 | order [rows] | cnt [504 nblk + 1] | scan [504 nblk + 1] | total | scratch of the scan
static size_t gr_off_order(int64_t rows) { return align_up((size_t)rows * sizeof(int16_t), 256); }
static size_t gr_off_cnt(int64_t rows) { return gr_off_order(rows) + align_up((size_t)rows * sizeof(int), 256); }
static size_t gr_off_scan(int64_t rows, int64_t nblk) { return gr_off_cnt(rows) + align_up((size_t)(GR_PATCHES * nblk + 1) * sizeof(int), 256); }
static size_t gr_off_sws(int64_t rows, int64_t nblk) { return gr_off_scan(rows, nblk) + align_up((size_t)(GR_PATCHES * nblk + 1 + 16) * sizeof(int), 256); }
MOPA_API size_t mopa_ground_workspace_bytes(int64_t total_rows, int64_t total_blocks) {
  if (total_rows < 0 || total_blocks < 0) return 0;
  return gr_off_sws(total_rows, total_blocks) + mopa_scan_workspace_bytes(GR_PATCHES * total_blocks + 1);
}
// kernel launches of one mopa_ground_estimate over `total_blocks` blocks (it follows the size of the count table, not B)
MOPA_API int mopa_ground_launches(int64_t total_blocks) {
  if (total_blocks <= 0) return 0;
  return 3 + (GR_PATCHES * total_blocks + 1 <= 8192 ? 1 : 3);
}

// The ground mask of B scans that lie behind each other in points (total_rows, cols) float32 (cols >= 3, the first three columns
// are x, y, z): mask[i] = 1 where row i is ground, else 0 (total_rows bytes, all written).  tab (device, 2 (B + 1) int32): row0[B + 1]
// = the first row of every scan and total_rows, then blk0[B + 1] = the first block of every scan and total_blocks, a scan of n rows
// having ceil(n / mopa_ground_rows_per_block()) blocks; total_rows and total_blocks repeat the tables' last entries (the kernels
// refuse rows outside them).  params_host: mopa_ground_num_params() doubles -- sensor_height, rmin, rmax, th_seeds, th_dist,
// uprightness, noise_cut (zone-0 points below -noise_cut * sensor_height are dropped), elevation[4], flatness[4], num_min_pts,
// num_lpr, num_iter.
MOPA_API int mopa_ground_estimate(const float* points, int32_t cols, const int32_t* tab, int32_t B, int64_t total_rows, int64_t total_blocks,
                                  const double* params_host, uint8_t* mask, void* ws, size_t ws_bytes, void* stream) {
  if (B < 1 || B > 65535 || cols < 3 || total_rows < 0 || total_rows >= (int64_t)1 << 30 || total_blocks < 0 || !params_host || !tab) return MOPA_ERR_ARG;
  if (total_blocks > total_rows || total_blocks * GR_ROWS < total_rows || total_blocks > total_rows / GR_ROWS + B) return MOPA_ERR_ARG;
  if (total_rows == 0) return MOPA_OK;
  if (!points || !mask || !ws) return MOPA_ERR_ARG;
  if (ws_bytes < mopa_ground_workspace_bytes(total_rows, total_blocks)) return MOPA_ERR_WORKSPACE;
  GrParams P;
  const double* v = params_host;
  P.h = v[0]; P.rmin = v[1]; P.rmax = v[2]; P.th_seeds = v[3]; P.th_dist = v[4]; P.upright = v[5]; P.noise_cut = v[6];
  for (int k = 0; k < 4; ++k) { P.elev[k] = v[7 + k]; P.flat[k] = v[11 + k]; }
  P.num_min_pts = (int)v[15]; P.num_lpr = (int)v[16]; P.num_iter = (int)v[17];
  if (!(P.rmin > 0 && P.rmax > P.rmin && P.h == P.h) || P.num_min_pts < 3 || P.num_lpr < 1 || P.num_iter < 1 || P.num_iter > 64) return MOPA_ERR_ARG;
  P.b[0] = P.rmin; P.b[1] = (7 * P.rmin + P.rmax) / 8; P.b[2] = (3 * P.rmin + P.rmax) / 4; P.b[3] = (P.rmin + P.rmax) / 2; P.b[4] = P.rmax;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)total_blocks;
  int16_t* pid = (int16_t*)ws;
  int* order = (int*)((char*)ws + gr_off_order(total_rows));
  int* cnt = (int*)((char*)ws + gr_off_cnt(total_rows));
  int* scan = (int*)((char*)ws + gr_off_scan(total_rows, nblk));
  int* tot = scan + GR_PATCHES * (int64_t)nblk + 1;
  void* sws = (char*)ws + gr_off_sws(total_rows, nblk);
  const int items = GR_PATCHES * nblk + 1;               // one more (zero, written by the first block): scan[504 nblk] is the total
  k_gr_bin<<<nblk, GR_THREADS, 0, st>>>(points, cols, tab, B, total_rows, P, pid, mask, cnt);
  MOPA_CHECK_LAUNCH();
  const int rc = mopa_scan_exclusive_i32(cnt, scan, items, tot, sws, mopa_scan_workspace_bytes(items), stream);
  if (rc) return rc;
  k_gr_order<<<nblk, GR_THREADS, 0, st>>>(tab, B, total_rows, pid, scan, order);
  k_gr_fit<<<dim3(GR_PATCHES, B), GR_FIT_THREADS, 0, st>>>(points, cols, tab, B, total_rows, nblk, P, scan, order, mask);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
