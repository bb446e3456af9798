// Validation metrics on the device: one pass over the per-point logits of both networks gives the 2D / 3D / xM (and
// entropy-fused) predictions, their confusion matrices, the two logged entropy means and the two logged CE losses, and
// optionally the pseudo-label dump -- the reference does this on the host behind three `.cpu().numpy()` copies per batch
// and three sklearn confusion_matrix calls per scan.
//
// Reference: mopa/data/utils/validate.py:112-131 (predictions, softmax ensembling, entropy means, entropy fusion),
// :140-170 (per-scan Evaluator.update, pseudo-label dump), :184-185 (CE); mopa/data/utils/evaluate.py:12-26 (Evaluator.update
// = sklearn.metrics.confusion_matrix with labels=); mopa/models/losses.py:10-19 (prob_2_entropy).  Fixture: G9.
//
// Integers (confusion counts) go through per-block LDS histograms flushed with integer atomics: exact in any order.  Float sums
// (entropies, CE) are per-thread doubles -> per-block partials -> one finalize block summing them in index order: the same
// bits run to run.
#include "common.h"

#define EV_MAXC 64
#define EV_BLOCK 256          // threads per block = rows per tile
#define EV_NPART 5            // per-block partials: entropy 2D, entropy 3D, CE 2D, CE 3D, #valid labels
#define EV_MAXGRID 2048
#define EV_LDS_MAX 65536
#define EV_IGNORE (-100)

struct EvalArgs {
  const float* l2;            // (N, ld2)
  const float* l3;            // (N, ld3) or null: 2D only
  const int64_t* label;       // (N,)
  const int32_t* lut;         // class value -> matrix index or -1; null = identity on [0, L)
  int64_t ld2, ld3;
  int n, C, lut_size, L;
  int64_t* conf[4];           // 2D, 3D, xM, entropy-fused: [L][L] int64 each (rows = ground truth), added to; null = not wanted
  float inv_log2c;
  uint8_t* ps_pred;           // [2][N] or null
  float* ps_prob;             // [2][N]
  double* partial;            // [EV_NPART][gridDim.x]
};

__device__ __forceinline__ double ev_block_sum(double v, double* lds) {
  v = wave_sum_d(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t += lds[k];
  return t;
}

// class value -> matrix index, -1 = dropped (sklearn's labels= semantics)
__device__ __forceinline__ int ev_index(int64_t v, const int32_t* __restrict__ lut, int lut_size, int L) {
  if (lut) return (v >= 0 && v < lut_size) ? lut[v] : -1;
  return (v >= 0 && v < L) ? (int)v : -1;
}

// max, first argmax (torch.argmax: ties -> lowest index, a NaN wins) and s = sum_c exp(z_c - max)
struct RowStat { float mx, s; int arg; };
__device__ __forceinline__ RowStat ev_row_stat(const float* z, int C) {
  RowStat r;
  r.mx = z[0];
  r.arg = 0;
  for (int c = 1; c < C; ++c) {
    const float v = z[c];
    if (v > r.mx || (v != v && r.mx == r.mx)) { r.mx = v; r.arg = c; }
  }
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(z[c] - r.mx);
  r.s = s;
  return r;
}

// Coalesced copy of rows [r0, r0 + nr) of a contiguous (N, C) matrix into tile[row * Cp + c] with 16-byte loads (the rows
// start at element r0 * C, r0 a multiple of 256: 16-byte aligned whenever the matrix is).
__device__ __forceinline__ void ev_stage(const float* __restrict__ x, int64_t r0, int nr, int C, int Cp, float invC,
                                         float* __restrict__ tile) {
  const float* src = x + r0 * C;
  const int nf = nr * C, nv = nf >> 2;
  for (int v = threadIdx.x; v < nv; v += blockDim.x) {
    const float4 q = reinterpret_cast<const float4*>(src)[v];
    const float e4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = 4 * v + j;
      const int r = (int)(((float)e + 0.5f) * invC);   // exact: e < 2^14 and (e + 0.5) / C is >= 0.5 / C from an integer
      tile[r * Cp + (e - r * C)] = e4[j];
    }
  }
  for (int e = 4 * nv + threadIdx.x; e < nf; e += blockDim.x) {
    const int r = (int)(((float)e + 0.5f) * invC);
    tile[r * Cp + (e - r * C)] = src[e];
  }
}

// STAGED: both logit matrices are contiguous and 16-byte aligned, and their row tiles fit in LDS beside the histograms.
template <bool STAGED>
__global__ __launch_bounds__(EV_BLOCK) void k_eval_logits(EvalArgs a) {
  extern __shared__ __align__(16) unsigned char ev_lds[];
  const int L = a.L, LL = L * L, C = a.C;
  const bool has3 = a.l3 != nullptr, want_h = a.conf[3] != nullptr;
  int nmat = 0, slot[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) slot[k] = a.conf[k] ? nmat++ : -1;
  int* hist = reinterpret_cast<int*>(ev_lds);                              // [nmat][L][L]
  const int Cp = C | 1;                                                    // odd row pitch: conflict-free row reads
  float* tile2 = reinterpret_cast<float*>(ev_lds + ((nmat * LL * 4 + 15) & ~15));
  float* tile3 = tile2 + EV_BLOCK * Cp;
  for (int b = threadIdx.x; b < nmat * LL; b += blockDim.x) hist[b] = 0;
  __syncthreads();
  const float invC = 1.f / (float)C;

  double acc_e2 = 0.0, acc_e3 = 0.0, acc_c2 = 0.0, acc_c3 = 0.0, acc_n = 0.0;
  const int64_t ntiles = ((int64_t)a.n + EV_BLOCK - 1) / EV_BLOCK;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t r0 = t * EV_BLOCK;
    const int nr = (int)min((int64_t)EV_BLOCK, (int64_t)a.n - r0);
    if constexpr (STAGED) {
      ev_stage(a.l2, r0, nr, C, Cp, invC, tile2);
      if (has3) ev_stage(a.l3, r0, nr, C, Cp, invC, tile3);
      __syncthreads();
    }
    if (threadIdx.x < nr) {
      const int64_t i = r0 + threadIdx.x;
      const float* z2 = STAGED ? tile2 + threadIdx.x * Cp : a.l2 + i * a.ld2;
      const float* z3 = STAGED ? tile3 + threadIdx.x * Cp : a.l3 + i * a.ld3;
      const int64_t y = a.label[i];

      const RowStat s2 = ev_row_stat(z2, C);
      RowStat s3 = {0.f, 1.f, 0};
      if (has3) s3 = ev_row_stat(z3, C);
      // p = softmax(z).  The logged entropy is that of softmax(p) (validate.py:121-122 applies softmax to probabilities):
      // q_c = e_c / t, e_c = exp(p_c - pmax), pmax = 1 / s, so sum_c q_c log2 q_c = log2(e) sum_c e_c (p_c - pmax) / t - log2 t
      // (q_c >= exp(-1) / C: prob_2_entropy's +1e-30 is below fp32 resolution there).
      const float pm2 = 1.f / s2.s, pm3 = 1.f / s3.s;
      float t2 = 0.f, u2 = 0.f, t3 = 0.f, u3 = 0.f, h2 = 0.f, h3 = 0.f, bx = 0.f;
      int ax = 0;
      for (int c = 0; c < C; ++c) {
        const float p2 = expf(z2[c] - s2.mx) / s2.s;
        const float e2 = expf(p2 - pm2);
        t2 += e2;
        u2 = fmaf(e2, p2 - pm2, u2);
        if (has3) {
          const float p3 = expf(z3[c] - s3.mx) / s3.s;
          const float e3 = expf(p3 - pm3);
          t3 += e3;
          u3 = fmaf(e3, p3 - pm3, u3);
          const float x = p2 + p3;                                         // validate.py:117-119: fp32 sum, then argmax
          if (c == 0 || x > bx) { bx = x; ax = c; }
          if (want_h) { h2 += p2 * log2f(p2 + 1e-30f); h3 += p3 * log2f(p3 + 1e-30f); }
        }
      }
      acc_e2 += (double)((log2f(t2) - u2 * 1.4426950408889634f / t2) * a.inv_log2c);
      if (has3) acc_e3 += (double)((log2f(t3) - u3 * 1.4426950408889634f / t3) * a.inv_log2c);
      if (y != EV_IGNORE && y >= 0 && y < C) {                             // F.cross_entropy, ignore_index -100
        acc_c2 += (double)(s2.mx + logf(s2.s) - z2[y]);
        if (has3) acc_c3 += (double)(s3.mx + logf(s3.s) - z3[y]);
        acc_n += 1.0;
      }
      int af = 0;
      if (want_h) {
        // entropy fusion (validate.py:126-131): w_m = exp(-sum_c prob_2_entropy(p_m)_c), normalised over the two modalities
        const float r2 = expf(h2 * a.inv_log2c), r3 = expf(h3 * a.inv_log2c);
        const float w2 = r2 / (r2 + r3), w3 = r3 / (r2 + r3);
        float bf = 0.f;
        for (int c = 0; c < C; ++c) {
          const float x = w2 * (expf(z2[c] - s2.mx) / s2.s) + w3 * (expf(z3[c] - s3.mx) / s3.s);
          if (c == 0 || x > bf) { bf = x; af = c; }
        }
      }
      if (a.ps_pred) {
        a.ps_pred[i] = (uint8_t)s2.arg;
        a.ps_prob[i] = pm2;                                                // softmax at the argmax = exp(0) / s
        if (has3) { a.ps_pred[a.n + i] = (uint8_t)s3.arg; a.ps_prob[a.n + i] = pm3; }
      }
      // confusion matrices: a ground truth of -100 becomes num_classes (evaluate.py:22), then both sides go through labels=
      const int gi = ev_index(y == EV_IGNORE ? (int64_t)L : y, a.lut, a.lut_size, L);
      if (gi >= 0) {
        const int pk[4] = {s2.arg, s3.arg, ax, af};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (slot[k] < 0) continue;
          const int pi = ev_index(pk[k], a.lut, a.lut_size, L);
          if (pi >= 0) atomicAdd(&hist[slot[k] * LL + gi * L + pi], 1);
        }
      }
    }
    if constexpr (STAGED) __syncthreads();                                 // the tiles are refilled next
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (slot[k] < 0) continue;
    const int* h = hist + slot[k] * LL;
    for (int b = threadIdx.x; b < LL; b += blockDim.x)
      if (h[b]) atomicAdd(reinterpret_cast<unsigned long long*>(a.conf[k] + b), (unsigned long long)h[b]);
  }
  double* red = reinterpret_cast<double*>(ev_lds);                        // the histograms are flushed: their LDS is reused
  const double v[EV_NPART] = {acc_e2, acc_e3, acc_c2, acc_c3, acc_n};
#pragma unroll
  for (int k = 0; k < EV_NPART; ++k) {
    const double s = ev_block_sum(v[k], red);
    if (threadIdx.x == 0) a.partial[k * gridDim.x + blockIdx.x] = s;
  }
}

// One block: the per-block partials in index order -> entropy means over N * C elements, CE means over the valid labels
// (0 / 0 = NaN when every label is ignored, like F.cross_entropy).
__global__ void k_eval_finalize(const double* __restrict__ partial, int nblk, int has3, double inv_nc, float* __restrict__ scalars) {
  __shared__ double lds[8];
  double s[EV_NPART];
#pragma unroll
  for (int k = 0; k < EV_NPART; ++k) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblk; b += blockDim.x) acc += partial[k * nblk + b];
    s[k] = ev_block_sum(acc, lds);
  }
  if (threadIdx.x == 0) {
    const float qnan = __builtin_nanf("");
    scalars[0] = (float)(s[0] * inv_nc);
    scalars[1] = has3 ? (float)(s[1] * inv_nc) : qnan;
    scalars[2] = (float)(s[2] / s[4]);
    scalars[3] = has3 ? (float)(s[3] / s[4]) : qnan;
  }
}

MOPA_API size_t mopa_eval_logits_workspace_bytes(int32_t n, int32_t C) {
  return align_up((size_t)EV_NPART * EV_MAXGRID * sizeof(double), 256);
}

// logit_2d (N, ld_2d) fp32; logit_3d (N, ld_3d) fp32 or null (2D only); label (N,) int64, -100 = ignore.
// lut (lut_size,) int32: class value -> matrix index in [0, n_labels) or -1 (sklearn's labels=); null = identity.
// conf_*: (n_labels, n_labels) int64, rows = ground truth, ADDED to; null = not computed (3D / xM / fused need logit_3d).
// scalars (4,) fp32 out: entropy mean 2D, 3D, CE 2D, CE 3D (the 3D entries NaN without logit_3d).
// ps_pred (2, N) uint8 / ps_prob (2, N) fp32: per-point prediction and softmax at it (2D row, then 3D row); null = none.
MOPA_API int mopa_eval_logits(const float* logit_2d, int64_t ld_2d, const float* logit_3d, int64_t ld_3d, const int64_t* label,
                              int32_t N, int32_t C, const int32_t* lut, int32_t lut_size, int32_t n_labels, int64_t* conf_2d,
                              int64_t* conf_3d, int64_t* conf_xm, int64_t* conf_ety, float* scalars, uint8_t* ps_pred,
                              float* ps_prob, void* ws, size_t ws_bytes, void* stream) {
  if (N <= 0 || C <= 1 || C > EV_MAXC || n_labels <= 0 || n_labels > EV_MAXC || ld_2d < C || !logit_2d || !label || !scalars)
    return MOPA_ERR_ARG;
  if (logit_3d && ld_3d < C) return MOPA_ERR_ARG;
  if (!logit_3d && (conf_3d || conf_xm || conf_ety)) return MOPA_ERR_ARG;
  if (lut && lut_size <= 0) return MOPA_ERR_ARG;
  if ((ps_pred == nullptr) != (ps_prob == nullptr)) return MOPA_ERR_ARG;
  if (ws_bytes < mopa_eval_logits_workspace_bytes(N, C)) return MOPA_ERR_WORKSPACE;
  EvalArgs a;
  a.l2 = logit_2d; a.l3 = logit_3d; a.label = label; a.lut = lut;
  a.ld2 = ld_2d; a.ld3 = logit_3d ? ld_3d : 0;
  a.n = N; a.C = C; a.lut_size = lut ? lut_size : 0; a.L = n_labels;
  a.conf[0] = conf_2d; a.conf[1] = conf_3d; a.conf[2] = conf_xm; a.conf[3] = conf_ety;
  a.inv_log2c = 1.f / log2f((float)C);
  a.ps_pred = ps_pred; a.ps_prob = ps_prob;
  a.partial = (double*)ws;
  int nmat = 0;
  for (int k = 0; k < 4; ++k) nmat += a.conf[k] != nullptr;
  const size_t hist = align_up((size_t)nmat * n_labels * n_labels * 4, 16);
  const size_t red = EV_BLOCK / 64 * sizeof(double);
  const size_t tiles = (size_t)(logit_3d ? 2 : 1) * EV_BLOCK * (C | 1) * sizeof(float);
  const bool aligned = ((uintptr_t)logit_2d & 15) == 0 && (!logit_3d || ((uintptr_t)logit_3d & 15) == 0);
  const bool staged = aligned && ld_2d == C && (!logit_3d || ld_3d == C) && hist + tiles <= EV_LDS_MAX;
  size_t lds = staged ? hist + tiles : hist;
  if (lds < red) lds = red;
  if (lds > EV_LDS_MAX) return MOPA_ERR_ARG;
  const int cus = mopa_cu_count();
  int64_t g = 4 * (int64_t)(cus > 0 ? cus : 256);
  const int64_t ntiles = cdiv64(N, EV_BLOCK);
  if (g > ntiles) g = ntiles;
  if (g > EV_MAXGRID) g = EV_MAXGRID;
  hipStream_t st = (hipStream_t)stream;
  if (staged) k_eval_logits<true><<<(int)g, EV_BLOCK, lds, st>>>(a);
  else k_eval_logits<false><<<(int)g, EV_BLOCK, lds, st>>>(a);
  k_eval_finalize<<<1, 256, 0, st>>>((const double*)ws, (int)g, logit_3d != nullptr, 1.0 / ((double)N * C), scalars);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// ------------------------------------------------------------------------------------------ Evaluator.update(pred, gt)
__global__ __launch_bounds__(256) void k_confusion_update(const int64_t* __restrict__ pred, const int64_t* __restrict__ gt, int64_t n,
                                                          const int32_t* __restrict__ lut, int lut_size, int L,
                                                          int64_t* __restrict__ conf) {
  extern __shared__ int cu_hist[];   // [L][L]
  const int LL = L * L;
  for (int b = threadIdx.x; b < LL; b += blockDim.x) cu_hist[b] = 0;
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t y = gt[i];
    const int gi = ev_index(y == EV_IGNORE ? (int64_t)L : y, lut, lut_size, L);
    const int pi = ev_index(pred[i], lut, lut_size, L);
    if (gi >= 0 && pi >= 0) atomicAdd(&cu_hist[gi * L + pi], 1);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < LL; b += blockDim.x)
    if (cu_hist[b]) atomicAdd(reinterpret_cast<unsigned long long*>(conf + b), (unsigned long long)cu_hist[b]);
}

// pred, gt (n,) int64; conf (n_labels, n_labels) int64, rows = ground truth, ADDED to; lut as for mopa_eval_logits.
MOPA_API int mopa_confusion_update(const int64_t* pred, const int64_t* gt, int64_t n, const int32_t* lut, int32_t lut_size,
                                   int32_t n_labels, int64_t* conf, void* stream) {
  if (n <= 0 || n_labels <= 0 || n_labels > EV_MAXC || !pred || !gt || !conf) return MOPA_ERR_ARG;
  if (lut && lut_size <= 0) return MOPA_ERR_ARG;
  int64_t g = cdiv64(n, 256);
  const int cus = mopa_cu_count();
  const int64_t cap = 2 * (int64_t)(cus > 0 ? cus : 256);
  if (g > cap) g = cap;
  k_confusion_update<<<(int)g, 256, (size_t)n_labels * n_labels * sizeof(int), (hipStream_t)stream>>>(
      pred, gt, n, lut, lut ? lut_size : 0, n_labels, conf);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
