// logCORAL loss (mopa/models/losses.py:47-93) on the device: float64 arithmetic on float32 features, no host synchronisation.
//
//   forward   k_coral_colsum   per input, CORAL_GRID blocks walk 64-row tiles: float64 partial column sums
//             k_coral_gram     the same walk: rows centred by the mean (partials summed in index order), float64 partial Gram slabs
//             k_coral_cov      cov = factor * (slabs summed in index order)
//             k_coral_eigen    one workgroup per matrix: the guard over BOTH matrices, parallel cyclic two-sided Jacobi in LDS
//                              (round-robin ordering, Fp / 2 disjoint rotations per step), L = V diag(log|lambda|) V^T
//             k_coral_loss     one workgroup per matrix: D, the loss, S = factor * (dC + dC^T) into the state buffer
//   backward  k_coral_bwd      dX = g * (x - mean) S per row, float64 accumulation, float32 store; exact zeros under the guard
//
// Every sum has a fixed order (no floating-point atomics): two runs give the same bits.  The arithmetic is stated in DESIGN.md
// section 4; yardstick tests/_coral_reference.py, held against the reference's own float64 autograd.
//
// state (doubles): [0] loss, [1] unused, mean[2][F], S[2][F][F].      status (int32): bit 0 the guard fired, bit 1 Jacobi hit its
// sweep bound without converging, bit 2 an eigenvalue was <= 0.
#include "common.h"

#define CORAL_MAX_F 64
#define CORAL_GRID 256        // blocks per input of the two walking kernels: the slab memory does not grow with N
#define CORAL_TILE 64         // rows per tile of the walk
#define CORAL_THREADS 256
#define CORAL_SWEEPS 30       // upper bound of Jacobi sweeps (float64 cyclic Jacobi converges quadratically; 64 x 64 takes ~10)
#define CORAL_JTOL 1e-15      // a pair is rotated while |a_pq| > tol * sqrt(|a_pp| |a_qq|)
#define CORAL_EQUAL 1e-9      // eigenvalues closer than this (relative) take the limit of the divided difference
#define CORAL_EIG_THREADS 1024

struct CoralWs {   // offsets in doubles
  size_t part, slab, cov, L, V, lam, total;
};
static inline CoralWs coral_ws(int F) {
  const size_t FF = (size_t)F * F;
  CoralWs w;
  w.part = 0;
  w.slab = w.part + (size_t)2 * CORAL_GRID * F;
  w.cov = w.slab + (size_t)2 * CORAL_GRID * FF;
  w.L = w.cov + 2 * FF;
  w.V = w.L + 2 * FF;
  w.lam = w.V + 2 * FF;
  w.total = w.lam + (size_t)2 * F;
  return w;
}

struct CoralIn {
  const float* x[2];
  long long n[2];
  int blocks[2];   // blocks of the walk that hold at least one tile
};

// sum of p[b * stride] for b = b0, b0 + step, ... < b1 in that order; the loads of sixteen terms are in flight together (one load per
// add would chain 256 memory latencies)
__device__ __forceinline__ double coral_ordered_sum(const double* __restrict__ p, size_t stride, int b0, int b1, int step) {
  double s = 0.0;
  int b = b0;
  for (; b + 15 * step < b1; b += 16 * step) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = p[(size_t)(b + k * step) * stride];
#pragma unroll
    for (int k = 0; k < 16; ++k) s += v[k];
  }
  for (; b < b1; b += step) s += p[(size_t)b * stride];
  return s;
}

// ---------------------------------------------------------------------------------------------------------------- column sums
// thread = (row lane, column); the lanes of a block are summed in index order.
__global__ __launch_bounds__(CORAL_THREADS) void k_coral_colsum(CoralIn in, int F, double* __restrict__ part, int* __restrict__ status) {
  __shared__ double red[CORAL_THREADS];
  const int side = blockIdx.y, tid = threadIdx.x;
  if (blockIdx.x == 0 && side == 0 && tid == 0) *status = 0;
  if ((int)blockIdx.x >= in.blocks[side]) return;
  const float* __restrict__ x = in.x[side];
  const long long N = in.n[side];
  const int lanes = CORAL_THREADS / F, c = tid % F, rl = tid / F;
  double acc = 0.0;
  if (rl < lanes) {
    for (long long t0 = (long long)blockIdx.x * CORAL_TILE; t0 < N; t0 += (long long)gridDim.x * CORAL_TILE) {
      const long long t1 = t0 + CORAL_TILE < N ? t0 + CORAL_TILE : N;
      for (long long r = t0 + rl; r < t1; r += lanes) acc += (double)x[r * F + c];
    }
  }
  red[tid] = acc;
  __syncthreads();
  if (tid < F) {
    double s = 0.0;
    for (int l = 0; l < lanes; ++l) s += red[l * F + tid];
    part[((size_t)side * CORAL_GRID + blockIdx.x) * F + tid] = s;
  }
}

// ------------------------------------------------------------------------------------------------------- centred Gram matrices
// A tile of 64 centred rows in LDS as doubles; a thread owns a 4 x 4 patch of the F x F result for the rows of its group
// (groups = 256 / patches: at F = 16 sixteen groups share a tile's rows); the groups are summed in index order at the end.
__global__ __launch_bounds__(CORAL_THREADS) void k_coral_gram(CoralIn in, int F, const double* __restrict__ part, double* __restrict__ slab,
                                                               double* __restrict__ state) {
  __shared__ double tile[CORAL_TILE * CORAL_MAX_F];   // [row][F4]; the groups' patches [group][patch][16] over it at the end
  __shared__ double mean[CORAL_MAX_F];
  const int side = blockIdx.y, tid = threadIdx.x;
  if ((int)blockIdx.x >= in.blocks[side]) return;
  const float* __restrict__ x = in.x[side];
  const long long N = in.n[side];
  const int F4 = (F + 3) & ~3, np1 = F4 >> 2, P = np1 * np1, groups = CORAL_THREADS / P;
  {   // the mean: the blocks' partial sums, lane l of 256 / F takes blocks l, l + lanes, ...; then the lanes in index order
    const int lanes = CORAL_THREADS / F, c = tid % F, l = tid / F;
    tile[tid] = l < lanes ? coral_ordered_sum(part + (size_t)side * CORAL_GRID * F + c, F, l, in.blocks[side], lanes) : 0.0;
    __syncthreads();
    if (tid < F4) {
      double s = 0.0;
      if (tid < F) {
        for (int k = 0; k < lanes; ++k) s += tile[k * F + tid];
        s /= (double)N;
        if (blockIdx.x == 0) state[2 + side * F + tid] = s;
      }
      mean[tid] = s;
    }
    __syncthreads();
  }
  const int g = tid / P, patch = tid % P, pi = (patch / np1) * 4, pj = (patch % np1) * 4;
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  for (long long t0 = (long long)blockIdx.x * CORAL_TILE; t0 < N; t0 += (long long)gridDim.x * CORAL_TILE) {
    const long long base = t0 * F, end = N * F;
    for (int e = tid; e < CORAL_TILE * F4; e += CORAL_THREADS) {
      const int r = e / F4, c = e - r * F4;
      const long long at = base + (long long)r * F + c;
      tile[e] = (c < F && at < end) ? (double)x[at] - mean[c] : 0.0;
    }
    __syncthreads();
    if (g < groups) {
      for (int r = g; r < CORAL_TILE; r += groups) {
        const double* row = tile + r * F4;
        const double a0 = row[pi], a1 = row[pi + 1], a2 = row[pi + 2], a3 = row[pi + 3];
        const double b0 = row[pj], b1 = row[pj + 1], b2 = row[pj + 2], b3 = row[pj + 3];
        acc[0] = fma(a0, b0, acc[0]);   acc[1] = fma(a0, b1, acc[1]);   acc[2] = fma(a0, b2, acc[2]);   acc[3] = fma(a0, b3, acc[3]);
        acc[4] = fma(a1, b0, acc[4]);   acc[5] = fma(a1, b1, acc[5]);   acc[6] = fma(a1, b2, acc[6]);   acc[7] = fma(a1, b3, acc[7]);
        acc[8] = fma(a2, b0, acc[8]);   acc[9] = fma(a2, b1, acc[9]);   acc[10] = fma(a2, b2, acc[10]); acc[11] = fma(a2, b3, acc[11]);
        acc[12] = fma(a3, b0, acc[12]); acc[13] = fma(a3, b1, acc[13]); acc[14] = fma(a3, b2, acc[14]); acc[15] = fma(a3, b3, acc[15]);
      }
    }
    __syncthreads();
  }
  if (g < groups) {
#pragma unroll
    for (int k = 0; k < 16; ++k) tile[(g * P + patch) * 16 + k] = acc[k];
  }
  __syncthreads();
  double* out = slab + ((size_t)side * CORAL_GRID + blockIdx.x) * F * F;
  for (int e = tid; e < F * F; e += CORAL_THREADS) {
    const int i = e / F, j = e - i * F;
    const int pt = (i >> 2) * np1 + (j >> 2), k = (i & 3) * 4 + (j & 3);
    double s = 0.0;
    for (int gg = 0; gg < groups; ++gg) s += tile[(gg * P + pt) * 16 + k];
    out[e] = s;
  }
}

__global__ __launch_bounds__(CORAL_THREADS) void k_coral_cov(CoralIn in, int F, double factor, const double* __restrict__ slab,
                                                              double* __restrict__ cov) {
  const int FF = F * F, e = blockIdx.x * CORAL_THREADS + threadIdx.x;
  if (e >= 2 * FF) return;
  const int side = e / FF, k = e - side * FF;
  cov[e] = factor * coral_ordered_sum(slab + (size_t)side * CORAL_GRID * FF + k, FF, 0, in.blocks[side], 1);
}

// -------------------------------------------------------------------------------------------------------------------- eigen stage
// The pair (p, q) of rotation k in step s of the round-robin ordering over n = 2h players (circle method: player n - 1 stays).
__device__ __forceinline__ void coral_pair(int k, int s, int n, int& p, int& q) {
  const int m = n - 1;
  int a = k == 0 ? m : (s + k) % m, b = k == 0 ? s % m : (s - k + m) % m;
  p = a < b ? a : b;
  q = a < b ? b : a;
}

__global__ __launch_bounds__(CORAL_EIG_THREADS) void k_coral_eigen(int F, const double* __restrict__ cov, double* __restrict__ Lout,
                                                                    double* __restrict__ Vout, double* __restrict__ lamout,
                                                                    int* __restrict__ status) {
  extern __shared__ __align__(16) unsigned char coral_lds[];
  const int side = blockIdx.x, tid = threadIdx.x, FF = F * F;
  const int Fp = (F + 1) & ~1, h = Fp >> 1, LD = Fp + 1;   // odd F is padded by a unit diagonal entry; odd row stride against bank conflicts
  double* A = reinterpret_cast<double*>(coral_lds);
  double* V = A + Fp * LD;
  double* rc = V + Fp * LD;   // c, s, t of the step's rotations
  double* rs = rc + h;
  double* rt = rs + h;
  int* rp = reinterpret_cast<int*>(rt + h);
  int* rq = rp + h;
  __shared__ int rotated;

  // the guard: any entry of EITHER covariance > 1e30 or NaN -> both become the identity
  int bad = 0;
  for (int e = tid; e < 2 * FF; e += CORAL_EIG_THREADS) {
    const double v = cov[e];
    bad |= (v > 1e30) || (v != v);
  }
  bad = __syncthreads_or(bad);
  for (int e = tid; e < Fp * Fp; e += CORAL_EIG_THREADS) {
    const int i = e / Fp, j = e - i * Fp;
    double a = i == j ? 1.0 : 0.0;
    if (!bad && i < F && j < F) a = i <= j ? cov[(size_t)side * FF + i * F + j] : cov[(size_t)side * FF + j * F + i];   // symmetric in bits
    A[i * LD + j] = a;
    V[i * LD + j] = i == j ? 1.0 : 0.0;
  }
  if (tid == 0 && side == 0 && bad) atomicOr(status, 1);
  __syncthreads();

  int converged = 0;
  for (int sweep = 0; sweep < CORAL_SWEEPS; ++sweep) {
    if (tid == 0) rotated = 0;
    __syncthreads();
    for (int s = 0; s < Fp - 1; ++s) {
      if (tid < h) {
        int p, q;
        coral_pair(tid, s, Fp, p, q);
        const double app = A[p * LD + p], aqq = A[q * LD + q], apq = A[p * LD + q];
        double c = 1.0, sn = 0.0, t = 0.0;
        if (fabs(apq) > CORAL_JTOL * sqrt(fabs(app)) * sqrt(fabs(aqq))) {
          const double theta = (aqq - app) / (2.0 * apq);
          t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
          if (!(fabs(theta) < 1e150)) t = 0.5 / theta;   // theta^2 would overflow
          c = 1.0 / sqrt(1.0 + t * t);
          sn = t * c;
          rotated = 1;
        }
        rc[tid] = c; rs[tid] = sn; rt[tid] = t; rp[tid] = p; rq[tid] = q;
      }
      __syncthreads();
      // A <- J^T A J by 2 x 2 blocks (pair k rows, pair l columns), upper blocks computed and mirrored
      for (int e = tid; e < h * h; e += CORAL_EIG_THREADS) {
        const int k = e / h, l = e - k * h;
        if (k > l) continue;
        const int p = rp[k], q = rq[k];
        if (k == l) {
          const double t = rt[k], apq = A[p * LD + q];
          A[p * LD + p] -= t * apq;
          A[q * LD + q] += t * apq;
          if (t != 0.0) { A[p * LD + q] = 0.0; A[q * LD + p] = 0.0; }
        } else {
          const int r = rp[l], u = rq[l];
          const double ck = rc[k], sk = rs[k], cl = rc[l], sl = rs[l];
          const double bpr = A[p * LD + r], bpu = A[p * LD + u], bqr = A[q * LD + r], bqu = A[q * LD + u];
          const double tpr = ck * bpr - sk * bqr, tpu = ck * bpu - sk * bqu;
          const double tqr = sk * bpr + ck * bqr, tqu = sk * bpu + ck * bqu;
          const double npr = cl * tpr - sl * tpu, npu = sl * tpr + cl * tpu;
          const double nqr = cl * tqr - sl * tqu, nqu = sl * tqr + cl * tqu;
          A[p * LD + r] = npr; A[r * LD + p] = npr;
          A[p * LD + u] = npu; A[u * LD + p] = npu;
          A[q * LD + r] = nqr; A[r * LD + q] = nqr;
          A[q * LD + u] = nqu; A[u * LD + q] = nqu;
        }
      }
      // V <- V J
      for (int e = tid; e < Fp * h; e += CORAL_EIG_THREADS) {
        const int i = e / h, l = e - i * h;
        const int r = rp[l], u = rq[l];
        const double cl = rc[l], sl = rs[l];
        const double vr = V[i * LD + r], vu = V[i * LD + u];
        V[i * LD + r] = cl * vr - sl * vu;
        V[i * LD + u] = sl * vr + cl * vu;
      }
      __syncthreads();
    }
    const int any = rotated;   // the same value in every thread: read between two barriers
    __syncthreads();
    if (!any) { converged = 1; break; }
  }

  // eigenvalues; log|lambda| (IEEE: log 0 = -inf) takes their place on A's diagonal; L = V diag(log|lambda|) V^T
  int bits = converged ? 0 : 2;
  if (tid < F) {
    const double lam = A[tid * LD + tid];
    if (lam <= 0.0) bits |= 4;
    lamout[side * F + tid] = lam;
    A[tid * LD + tid] = log(fabs(lam));
  }
  bits = __syncthreads_or(bits);
  if (tid == 0 && bits) atomicOr(status, bits);
  for (int e = tid; e < FF; e += CORAL_EIG_THREADS) {
    const int i = e / F, j = e - i * F;
    double s = 0.0;
    for (int k = 0; k < F; ++k) s = fma(V[i * LD + k] * A[k * LD + k], V[j * LD + k], s);
    Lout[(size_t)side * FF + e] = s;
    Vout[(size_t)side * FF + e] = V[i * LD + j];
  }
}
static size_t coral_eigen_lds(int F) {
  const int Fp = (F + 1) & ~1, h = Fp >> 1, LD = Fp + 1;
  return (size_t)2 * Fp * LD * 8 + (size_t)3 * h * 8 + (size_t)2 * h * 4;
}

// --------------------------------------------------------------------------------------------------------------------- loss stage
__device__ __forceinline__ double coral_block_sum(double v, double* red) {   // fixed order: wave shuffles, then the waves in index order
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(CORAL_EIG_THREADS) void k_coral_loss(int F, double factor, const double* __restrict__ L, const double* __restrict__ Vg,
                                                                   const double* __restrict__ lamg, double* __restrict__ state,
                                                                   float* __restrict__ loss) {
  extern __shared__ __align__(16) unsigned char coral_lds[];
  __shared__ double red[CORAL_EIG_THREADS / 64];
  const int side = blockIdx.x, tid = threadIdx.x, FF = F * F, LD = F | 1;
  double* V = reinterpret_cast<double*>(coral_lds);
  double* B1 = V + F * LD;
  double* B2 = B1 + F * LD;
  double* lam = B2 + F * LD;   // |lambda|
  const double sign = side == 0 ? 1.0 : -1.0, inv = 1.0 / ((double)F * (double)F);
  double sq = 0.0;
  for (int e = tid; e < FF; e += CORAL_EIG_THREADS) {
    const int i = e / F, j = e - i * F;
    const double d = L[e] - L[FF + e];
    sq = fma(d, d, sq);
    B1[i * LD + j] = sign * 2.0 * d * inv;          // +-G
    V[i * LD + j] = Vg[(size_t)side * FF + e];
  }
  if (tid < F) lam[tid] = fabs(lamg[side * F + tid]);
  const double total = coral_block_sum(sq, red);    // (its barriers also publish V, B1, lam)
  if (side == 0 && tid == 0) {
    state[0] = total * inv;
    *loss = (float)(total * inv);
  }
  // B2 = (+-G) V
  for (int e = tid; e < FF; e += CORAL_EIG_THREADS) {
    const int i = e / F, j = e - i * F;
    double s = 0.0;
    for (int k = 0; k < F; ++k) s = fma(B1[i * LD + k], V[k * LD + j], s);
    B2[i * LD + j] = s;
  }
  __syncthreads();
  // B1 = (V^T B2) o K
  for (int e = tid; e < FF; e += CORAL_EIG_THREADS) {
    const int i = e / F, j = e - i * F;
    double s = 0.0;
    for (int k = 0; k < F; ++k) s = fma(V[k * LD + i], B2[k * LD + j], s);
    const double a = fmax(lam[i], lam[j]), b = fmin(lam[i], lam[j]), d = a - b;
    const double K = d <= CORAL_EQUAL * a ? 2.0 / (a + b) : log1p(d / b) / d;
    B1[i * LD + j] = s * K;
  }
  __syncthreads();
  // B2 = B1 V^T
  for (int e = tid; e < FF; e += CORAL_EIG_THREADS) {
    const int i = e / F, j = e - i * F;
    double s = 0.0;
    for (int k = 0; k < F; ++k) s = fma(B1[i * LD + k], V[j * LD + k], s);
    B2[i * LD + j] = s;
  }
  __syncthreads();
  // B1 = V B2 = dC
  for (int e = tid; e < FF; e += CORAL_EIG_THREADS) {
    const int i = e / F, j = e - i * F;
    double s = 0.0;
    for (int k = 0; k < F; ++k) s = fma(V[i * LD + k], B2[k * LD + j], s);
    B1[i * LD + j] = s;
  }
  __syncthreads();
  double* S = state + 2 + 2 * F + (size_t)side * FF;
  for (int e = tid; e < FF; e += CORAL_EIG_THREADS) {
    const int i = e / F, j = e - i * F;
    S[e] = factor * (B1[i * LD + j] + B1[j * LD + i]);
  }
}
static size_t coral_loss_lds(int F) { return ((size_t)3 * F * (F | 1) + F) * 8; }

// ---------------------------------------------------------------------------------------------------------------------- backward
// A thread owns 4 rows x 4 columns of a tile of R = 4 * (256 / column patches) rows; g * S (float64) and the tile are in LDS.
__global__ __launch_bounds__(CORAL_THREADS) void k_coral_bwd(const float* __restrict__ x, long long N, int F, const double* __restrict__ mean_g,
                                                              const double* __restrict__ S_g, const int* __restrict__ status,
                                                              const float* __restrict__ gout, float* __restrict__ dx) {
  __shared__ double S[CORAL_MAX_F * CORAL_MAX_F];     // [F4][F4], zero padded
  __shared__ float tile[CORAL_MAX_F * CORAL_MAX_F];   // [R][F4], as loaded: the mean is subtracted in float64 at the read
  __shared__ double mean[CORAL_MAX_F];
  const int tid = threadIdx.x;
  const int F4 = (F + 3) & ~3, ncp = F4 >> 2, rg = CORAL_THREADS / ncp, R = 4 * rg;
  const long long tiles = (N + R - 1) / R, end = N * F;
  if (*status & 1) {   // the guard fired: no gradient flows (x - mean may hold NaN, so it is not multiplied by zeros)
    for (long long e = (long long)blockIdx.x * CORAL_THREADS + tid; e < end; e += (long long)gridDim.x * CORAL_THREADS) dx[e] = 0.f;
    return;
  }
  const double g = (double)*gout;
  for (int e = tid; e < F4 * F4; e += CORAL_THREADS) {
    const int i = e / F4, j = e - i * F4;
    S[e] = (i < F && j < F) ? g * S_g[i * F + j] : 0.0;
  }
  if (tid < F4) mean[tid] = tid < F ? mean_g[tid] : 0.0;
  __syncthreads();
  const int cp = tid % ncp, rgi = tid / ncp, j0 = cp * 4, r0 = rgi * 4;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long base = t * R * F;
    for (int e = tid; e < R * F4; e += CORAL_THREADS) {
      const int r = e / F4, c = e - r * F4;
      const long long at = base + (long long)r * F + c;
      tile[e] = (c < F && at < end) ? x[at] : 0.f;
    }
    __syncthreads();
    if (rgi < rg) {
      double acc[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[k] = 0.0;
      for (int i = 0; i < F; ++i) {
        const double* s = S + i * F4 + j0;
        const double s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3], mi = mean[i];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const double a = (double)tile[(r0 + rr) * F4 + i] - mi;
          acc[rr * 4 + 0] = fma(a, s0, acc[rr * 4 + 0]);
          acc[rr * 4 + 1] = fma(a, s1, acc[rr * 4 + 1]);
          acc[rr * 4 + 2] = fma(a, s2, acc[rr * 4 + 2]);
          acc[rr * 4 + 3] = fma(a, s3, acc[rr * 4 + 3]);
        }
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const long long row = t * R + r0 + rr;
        if (row < N) {
#pragma unroll
          for (int cc = 0; cc < 4; ++cc)
            if (j0 + cc < F) dx[row * F + j0 + cc] = (float)acc[rr * 4 + cc];
        }
      }
    }
    __syncthreads();
  }
}

// --------------------------------------------------------------------------------------------------------------------- entry points
MOPA_API size_t mopa_logcoral_workspace_bytes(int F) {
  if (F < 1 || F > CORAL_MAX_F) return 0;
  return coral_ws(F).total * sizeof(double);
}

MOPA_API size_t mopa_logcoral_state_bytes(int F) {
  if (F < 1 || F > CORAL_MAX_F) return 0;
  return ((size_t)2 + 2 * F + (size_t)2 * F * F) * sizeof(double);
}

static int coral_lds_attr(const void* kern, size_t bytes, int slot) {
  static std::atomic<bool> attr[64][2];   // per device: the attribute belongs to the device's code object
  const int dev = mopa_device_index();
  if (dev < 0) return MOPA_ERR_LAUNCH;
  if (!attr[dev][slot].load(std::memory_order_acquire)) {
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return MOPA_ERR_LAUNCH;
    attr[dev][slot].store(true, std::memory_order_release);
  }
  return MOPA_OK;
}

// x_src (n_src, F), x_trg (n_trg, F) float32 row-major; batch_size = x_src.shape[0] BEFORE flattening (the reference's factor
// 1 / (batch_size - 1) scales both covariances); loss: one float32; state: mopa_logcoral_state_bytes(F), read by mopa_logcoral_bwd;
// status: one int32 (bits above), rewritten by every call.
MOPA_API int mopa_logcoral_fwd(const float* x_src, int64_t n_src, const float* x_trg, int64_t n_trg, int F, int64_t batch_size, float* loss,
                               void* state, int* status, void* ws, size_t ws_bytes, void* stream) {
  if (F < 1 || F > CORAL_MAX_F || n_src < 2 || n_trg < 2 || batch_size < 2 || !x_src || !x_trg || !loss || !state || !status || !ws)
    return MOPA_ERR_ARG;
  if (((uintptr_t)state & 7) || ((uintptr_t)ws & 7)) return MOPA_ERR_ARG;
  const CoralWs w = coral_ws(F);
  if (ws_bytes < w.total * sizeof(double)) return MOPA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* d = (double*)ws;
  CoralIn in;
  in.x[0] = x_src; in.x[1] = x_trg;
  in.n[0] = n_src; in.n[1] = n_trg;
  int gmax = 1;
  for (int s = 0; s < 2; ++s) {
    const int64_t tiles = cdiv64(in.n[s], CORAL_TILE);
    in.blocks[s] = (int)(tiles < CORAL_GRID ? tiles : CORAL_GRID);
    if (in.blocks[s] > gmax) gmax = in.blocks[s];
  }
  const double factor = 1.0 / (double)(batch_size - 1);
  const size_t lds_e = coral_eigen_lds(F), lds_l = coral_loss_lds(F);
  int rc = coral_lds_attr(reinterpret_cast<const void*>(k_coral_eigen), coral_eigen_lds(CORAL_MAX_F), 0);
  if (rc == MOPA_OK) rc = coral_lds_attr(reinterpret_cast<const void*>(k_coral_loss), coral_loss_lds(CORAL_MAX_F), 1);
  if (rc != MOPA_OK) return rc;
  k_coral_colsum<<<dim3(gmax, 2), CORAL_THREADS, 0, st>>>(in, F, d + w.part, status);
  MOPA_CHECK_LAUNCH();
  k_coral_gram<<<dim3(gmax, 2), CORAL_THREADS, 0, st>>>(in, F, d + w.part, d + w.slab, (double*)state);
  MOPA_CHECK_LAUNCH();
  k_coral_cov<<<(unsigned)cdiv64(2 * F * F, CORAL_THREADS), CORAL_THREADS, 0, st>>>(in, F, factor, d + w.slab, d + w.cov);
  MOPA_CHECK_LAUNCH();
  k_coral_eigen<<<2, CORAL_EIG_THREADS, lds_e, st>>>(F, d + w.cov, d + w.L, d + w.V, d + w.lam, status);
  MOPA_CHECK_LAUNCH();
  k_coral_loss<<<2, CORAL_EIG_THREADS, lds_l, st>>>(F, factor, d + w.L, d + w.V, d + w.lam, (double*)state, loss);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// dx (n, F) float32 = g * (x - mean[side]) S[side] for the input of `side` (0 = source, 1 = target) of the forward call that wrote
// `state` and `status`; g: one float32 on the device (the upstream gradient of the loss).
MOPA_API int mopa_logcoral_bwd(const float* x, int64_t n, int F, int side, const void* state, const int* status, const float* g, float* dx,
                               void* stream) {
  if (F < 1 || F > CORAL_MAX_F || n < 2 || side < 0 || side > 1 || !x || !state || !status || !g || !dx) return MOPA_ERR_ARG;
  if ((uintptr_t)state & 7) return MOPA_ERR_ARG;
  const double* s = (const double*)state;
  const int F4 = (F + 3) & ~3, R = 4 * (CORAL_THREADS / (F4 >> 2));
  const int64_t tiles = cdiv64(n, R);
  const unsigned grid = (unsigned)(tiles < 1024 ? tiles : 1024);
  k_coral_bwd<<<grid, CORAL_THREADS, 0, (hipStream_t)stream>>>(x, (long long)n, F, s + 2 + side * F, s + 2 + 2 * F + (size_t)side * F * F, status, g, dx);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
