// Loss kernels of the hot path: cross-modal KL, weighted cross-entropy with ignore label, softmax over the
// class dimension, and the SAM-mask consistency loss.  All are HBM-bound row reductions over (N, C) with small C:
// one thread per row, wave-shuffle + LDS block reduction, deterministic two-stage sums (block partials -> one
// finalize block accumulating in double).  Scalars (loss value, upstream gradient, normalisers) stay on the device:
// no host sync between forward and backward.
//
// Reference call sites (all in mopa/train/train_xmuda_mopa.py): KL :389-398,:440-445; CE :354-363,:456-465,:563-567;
// softmax + mask_cons_loss :472-480 with mopa/common/utils/loss.py:241-283.  Oracle: oracle/losses.py.
#include "common.h"
#include "softmax_row.h"   // row_lse, row_softmax_at: shared with lovasz.hip

#define MAXC 64
#define LOSS_BLOCK 256

__device__ __forceinline__ double block_sum_d(double v, double* lds) {
  v = wave_sum_d(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t += lds[k];
  return t;
}

// ------------------------------------------------------------------------------------------ softmax KL
// loss = mean_i sum_c q_ic (log q_ic - log p_ic),  p = softmax(a_i), q = softmax(b_i)  (b is the detached target).
__global__ __launch_bounds__(LOSS_BLOCK) void k_kl_partial(const float* __restrict__ a, const float* __restrict__ b, int N, int C,
                                                            double* __restrict__ partial) {
  __shared__ double lds[8];
  double acc = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const float* ar = a + (int64_t)i * C;
    const float* br = b + (int64_t)i * C;
    const float la = row_lse(ar, C), lb = row_lse(br, C);
    float t = 0.f;
    for (int c = 0; c < C; ++c) {
      const float lq = br[c] - lb, q = expf(lq);
      t += (q > 0.f) ? q * (lq - (ar[c] - la)) : 0.f;
    }
    acc += (double)t;
  }
  const double s = block_sum_d(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ void k_scalar_finalize(const double* __restrict__ partial, int n, double scale, float* __restrict__ out) {
  __shared__ double lds[8];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partial[i];
  const double s = block_sum_d(acc, lds);
  if (threadIdx.x == 0) *out = (float)(s * scale);
}
// da_ic = gout * (p_ic - q_ic) / N
__global__ void k_kl_bwd(const float* __restrict__ a, const float* __restrict__ b, int N, int C, const float* __restrict__ gout,
                         float* __restrict__ da) {
  const float g = *gout / (float)N;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const float* ar = a + (int64_t)i * C;
    const float* br = b + (int64_t)i * C;
    const float la = row_lse(ar, C), lb = row_lse(br, C);
    for (int c = 0; c < C; ++c) da[(int64_t)i * C + c] = g * (expf(ar[c] - la) - expf(br[c] - lb));
  }
}

MOPA_API size_t mopa_loss_workspace_bytes(int64_t n_rows) { return align_up((size_t)(2 * 2048 + 16) * sizeof(double), 256); }

MOPA_API int mopa_softmax_kl_fwd(const float* logit_p, const float* logit_q, int32_t N, int32_t C, float* loss, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (N <= 0 || C <= 0 || C > MAXC) return MOPA_ERR_ARG;
  if (ws_bytes < mopa_loss_workspace_bytes(N)) return MOPA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int g = stream_grid(N, LOSS_BLOCK);
  k_kl_partial<<<g, LOSS_BLOCK, 0, st>>>(logit_p, logit_q, N, C, (double*)ws);
  k_scalar_finalize<<<1, 256, 0, st>>>((const double*)ws, g, 1.0 / N, loss);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
MOPA_API int mopa_softmax_kl_bwd(const float* logit_p, const float* logit_q, int32_t N, int32_t C, const float* gout,
                                 float* dlogit_p, void* stream) {
  if (N <= 0 || C <= 0 || C > MAXC) return MOPA_ERR_ARG;
  k_kl_bwd<<<stream_grid(N, LOSS_BLOCK), LOSS_BLOCK, 0, (hipStream_t)stream>>>(logit_p, logit_q, N, C, gout, dlogit_p);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// ------------------------------------------------------------------------------------------ weighted CE, ignore label
// loss = sum_i w[y_i] * (lse(z_i) - z_i[y_i]) / sum_i w[y_i]   over rows with y_i != ignore (torch cross_entropy 'mean').
__global__ __launch_bounds__(LOSS_BLOCK) void k_wce_partial(const float* __restrict__ z, const int64_t* __restrict__ y,
                                                             const float* __restrict__ w, int N, int C, int64_t ignore,
                                                             double* __restrict__ partial, int* __restrict__ status) {
  __shared__ double lds[8];
  double num = 0.0, den = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const int64_t yi = y[i];
    if (yi == ignore) continue;
    if (yi < 0 || yi >= C) { atomicOr(status, 1); continue; }
    const float* zr = z + (int64_t)i * C;
    const float wi = w ? w[yi] : 1.f;
    num += (double)(wi * (row_lse(zr, C) - zr[yi]));
    den += (double)wi;
  }
  const double sn = block_sum_d(num, lds);
  const double sd = block_sum_d(den, lds);
  if (threadIdx.x == 0) { partial[blockIdx.x] = sn; partial[gridDim.x + blockIdx.x] = sd; }
}
__global__ void k_wce_finalize(const double* __restrict__ partial, int n, float* __restrict__ loss, float* __restrict__ den_out) {
  __shared__ double lds[8];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) { a += partial[i]; b += partial[n + i]; }
  const double sn = block_sum_d(a, lds);
  const double sd = block_sum_d(b, lds);
  if (threadIdx.x == 0) { *loss = (float)(sn / sd); *den_out = (float)sd; }
}
__global__ void k_wce_bwd(const float* __restrict__ z, const int64_t* __restrict__ y, const float* __restrict__ w, int N, int C,
                          int64_t ignore, const float* __restrict__ den, const float* __restrict__ gout, float* __restrict__ dz) {
  const float g = *gout / *den;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const int64_t yi = y[i];
    float* d = dz + (int64_t)i * C;
    if (yi == ignore || yi < 0 || yi >= C) {
      for (int c = 0; c < C; ++c) d[c] = 0.f;
      continue;
    }
    const float* zr = z + (int64_t)i * C;
    const float l = row_lse(zr, C);
    const float s = g * (w ? w[yi] : 1.f);
    for (int c = 0; c < C; ++c) d[c] = s * (expf(zr[c] - l) - (c == yi ? 1.f : 0.f));
  }
}

// status: device int, bit0 set when a label is outside [0,C) and != ignore.
MOPA_API int mopa_wce_fwd(const float* logits, const int64_t* labels, const float* class_weight, int32_t N, int32_t C,
                          int64_t ignore_index, float* loss, float* den, int32_t* status, void* ws, size_t ws_bytes,
                          void* stream) {
  if (N <= 0 || C <= 0 || C > MAXC) return MOPA_ERR_ARG;
  if (ws_bytes < mopa_loss_workspace_bytes(N)) return MOPA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int g = stream_grid(N, LOSS_BLOCK);
  k_wce_partial<<<g, LOSS_BLOCK, 0, st>>>(logits, labels, class_weight, N, C, ignore_index, (double*)ws, status);
  k_wce_finalize<<<1, 256, 0, st>>>((const double*)ws, g, loss, den);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
MOPA_API int mopa_wce_bwd(const float* logits, const int64_t* labels, const float* class_weight, int32_t N, int32_t C,
                          int64_t ignore_index, const float* den, const float* gout, float* dlogits, void* stream) {
  if (N <= 0 || C <= 0 || C > MAXC) return MOPA_ERR_ARG;
  k_wce_bwd<<<stream_grid(N, LOSS_BLOCK), LOSS_BLOCK, 0, (hipStream_t)stream>>>(logits, labels, class_weight, N, C,
                                                                                  ignore_index, den, gout, dlogits);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// ------------------------------------------------------------------------------------------ per-point training losses
// The loss-and-metric block between the forward and backward passes (train_xmuda_mopa.py:353-418,:437-469,:563-576) in ONE row
// pass over the per-point logits of both networks: the two weighted CE values, the two cross-modal KL values, SegIoU's two
// confusion matrices and pc_mm_acc's two counts -- for every row segment of a MERGED pass (source, target and the VGI batch as
// row segments of one logit tensor per network; bn_groups / bn_group_points upstream) in one forward launch pair and one backward
// launch per network, with entropy minimisation (mopa/models/losses.py:21-34 on the softmax of the main head,
// train_xmuda.py:323-330) as a third per-segment term.  A network's rows are the concatenation, in segment order, of the segments
// it takes part in.  The FORWARD has one kernel set: the one-call entry point (mopa_point_losses_fwd, one domain half) runs it
// over a table of one segment.  The backward has two kernels: k_point_losses_bwd (one call, its pointers `__restrict__` kernel
// parameters, 59 VGPRs) is 1.35x faster on one segment than k_point_losses_seg_bwd (49 VGPRs), which reads its pointers from the
// table (profiles/r33_trainloss_one_body.md).
//
// A block serves exactly one segment of n_s rows: g_s = stream_grid(n_s, 256) virtual blocks, partials [S][PL_SEG_TERMS][g_s].
// Partition, accumulation order and the CE / KL expressions are those of k_wce_partial / k_kl_partial / k_wce_finalize /
// k_scalar_finalize above on the segment's rows, so every CE / KL scalar and every gradient row without an entropy part has the
// bits of the single entry point (tests/test_gpu_trainloss.py, test_gpu_trainloss_merged.py); the integers go through per-block
// LDS counters flushed with integer atomics, like k_eval_logits (evaluate.hip).  The backward is one launch per network, as the
// reference backpropagates the two networks' loss sums separately.
#define PL_MAXGRID 2048
#define PL_MAXSEG 8
#define PL_SEG_TERMS 8   // per-block partials of a segment: CE numerator, CE normaliser, KL sum, entropy sum of the 2D, then the 3D network

// first maximal index; a NaN wins (torch.argmax, ev_row_stat of evaluate.hip)
__device__ __forceinline__ int row_argmax(const float* __restrict__ z, int C) {
  float mx = z[0];
  int arg = 0;
  for (int c = 1; c < C; ++c) {
    const float v = z[c];
    if (v > mx || (v != v && mx == mx)) { mx = v; arg = c; }
  }
  return arg;
}

// one row's KL term, the loop of k_kl_partial
__device__ __forceinline__ float kl_row(const float* __restrict__ ar, float la, const float* __restrict__ br, float lb, int C) {
  float t = 0.f;
  for (int c = 0; c < C; ++c) {
    const float lq = br[c] - lb, q = expf(lq);
    t += (q > 0.f) ? q * (lq - (ar[c] - la)) : 0.f;
  }
  return t;
}

// The sum of a row's CE and KL gradient parts on a shared head: one rounding of the two finished parts, as a tensor add of
// k_wce_bwd's and k_kl_bwd's results gives -- neither part's multiply may be contracted into this add.  The add is written
// out under the pragma: __fadd_rn is a plain `x + y` in the HIP headers, compiled with THEIR contraction setting, and was fused
// with the KL part's multiply into one v_pk_fma_f32.
__device__ __forceinline__ float add_parts(float ce_part, float kl_part) {
#pragma clang fp contract(off)
  return ce_part + kl_part;
}

#define PL_SEG_KL 1
#define PL_SEG_WEIGHTED 2
#define PL_SEG_MINENT 4
#define PL_LN2 0.6931471805599453f

// One entry of the host-side descriptor table `segs_host` (ten 64-bit words per segment).
struct PointLossSeg {
  int64_t n;                 // rows
  int64_t row0[2];           // first row in the 2D / 3D logits, -1: the network takes no part in this segment
  const int64_t* y[2];       // (n,) labels per network, or null: no CE and no confusion matrix
  const uint8_t* acc_mask;   // (n,) or null
  int64_t* conf[2];          // (C, C) int64, ADDED to; or null
  int64_t* acc_out;          // [2], ADDED to; or null
  int64_t flags;             // PL_SEG_KL | PL_SEG_WEIGHTED | PL_SEG_MINENT
};
static_assert(sizeof(PointLossSeg) == 80, "segs_host is ten 64-bit words per segment");

struct PointLossSegArgs {
  PointLossSeg seg[PL_MAXSEG];
  int blk0[PL_MAXSEG + 1];   // first block of every segment; blk0[S] = the grid
  const float* zm[2];        // merged main-head logits of the 2D / 3D network, or null
  const float* zx[2];        // merged logits of the head the KL term trains (== zm without a dual head), or null: no KL
  const float* w;
  int64_t ignore;
  int S, C;
  double* partial;           // segment s: PL_SEG_TERMS * blk0[s] + [PL_SEG_TERMS][g_s]
  int* status;
};

// the segment a block serves: the last one that starts at or before it (a zero-row segment owns no block)
__device__ __forceinline__ int seg_of_block(const int* blk0, int S) {
  int s = 0;
  for (int j = 1; j < S; ++j) s = (int)blockIdx.x >= blk0[j] ? j : s;
  return s;
}

// one row's sum_c p_c log2(p_c + 1e-30), p = exp(z - lse)
__device__ __forceinline__ float ent_row(const float* __restrict__ zr, float l, int C) {
  float e = 0.f;
  for (int c = 0; c < C; ++c) {
    const float p = expf(zr[c] - l);
    e += p * log2f(p + 1e-30f);
  }
  return e;
}
// d(p log2(p + 1e-30))/dp
__device__ __forceinline__ float ent_slope(float p) { return log2f(p + 1e-30f) + p / ((p + 1e-30f) * PL_LN2); }

__global__ __launch_bounds__(LOSS_BLOCK) void k_point_losses_seg(PointLossSegArgs a) {
  extern __shared__ int pl_hist[];   // [#matrices][C][C]
  __shared__ double lds[8];
  __shared__ int pl_acc[2];
  const int s = seg_of_block(a.blk0, a.S);
  const PointLossSeg& sg = a.seg[s];
  const int vb = blockIdx.x - a.blk0[s], g = a.blk0[s + 1] - a.blk0[s], N = (int)sg.n;
  const int C = a.C, CC = C * C;
  const int flags = (int)sg.flags;
  const float* zm[2];
  const float* zx[2];
  bool ce[2], kl[2], ent[2], shared[2];
  int64_t* conf[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const bool in = sg.row0[k] >= 0;
    zm[k] = in ? a.zm[k] + sg.row0[k] * C : nullptr;
    zx[k] = in && a.zx[k] ? a.zx[k] + sg.row0[k] * C : nullptr;
    ce[k] = in && sg.y[k];
    ent[k] = in && (flags & PL_SEG_MINENT);
    shared[k] = a.zx[k] == a.zm[k];
    conf[k] = ce[k] ? sg.conf[k] : nullptr;
  }
  const bool both = (flags & PL_SEG_KL) && zm[0] && zm[1];
  kl[0] = both && zx[0];
  kl[1] = both && zx[1];
  const float* w = (flags & PL_SEG_WEIGHTED) ? a.w : nullptr;
  const uint8_t* acc_mask = ce[1] ? sg.acc_mask : nullptr;

  int* hist[2] = {conf[0] ? pl_hist : nullptr, conf[1] ? pl_hist + (conf[0] ? CC : 0) : nullptr};
  const int nh = ((conf[0] ? 1 : 0) + (conf[1] ? 1 : 0)) * CC;
  for (int b = threadIdx.x; b < nh; b += blockDim.x) pl_hist[b] = 0;
  if (threadIdx.x < 2) pl_acc[threadIdx.x] = 0;
  __syncthreads();

  double num[2] = {0.0, 0.0}, den[2] = {0.0, 0.0}, ksum[2] = {0.0, 0.0}, esum[2] = {0.0, 0.0};
  int hit = 0, seen = 0;
  for (int i = vb * blockDim.x + threadIdx.x; i < N; i += g * blockDim.x) {
    int64_t yi[2] = {0, 0};
    bool keep[2] = {false, false};
    float lm[2] = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (ce[k]) {
        yi[k] = sg.y[k][i];
        if (yi[k] != a.ignore) {
          if (yi[k] < 0 || yi[k] >= C) atomicOr(a.status, 1);
          else keep[k] = true;
        }
      }
      if (keep[k] || kl[1 - k] || (kl[k] && shared[k]) || ent[k]) lm[k] = row_lse(zm[k] + (int64_t)i * C, C);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float* zr = zm[k] + (int64_t)i * C;
      if (keep[k]) {
        const float wi = w ? w[yi[k]] : 1.f;
        num[k] += (double)(wi * (lm[k] - zr[yi[k]]));
        den[k] += (double)wi;
      }
      if (kl[k]) {
        const float* ar = zx[k] + (int64_t)i * C;
        const float la = shared[k] ? lm[k] : row_lse(ar, C);
        ksum[k] += (double)kl_row(ar, la, zm[1 - k] + (int64_t)i * C, lm[1 - k], C);
      }
      if (ent[k]) esum[k] += (double)ent_row(zr, lm[k], C);
      const bool masked = k == 1 && acc_mask && acc_mask[i];
      if ((hist[k] && keep[k]) || masked) {
        const int arg = row_argmax(zr, C);
        if (hist[k] && keep[k]) atomicAdd(&hist[k][(int)yi[k] * C + arg], 1);
        if (masked) { seen += 1; hit += (int64_t)arg == yi[k] ? 1 : 0; }
      }
    }
  }
  if (acc_mask) {
    hit = wave_sum_i(hit);
    seen = wave_sum_i(seen);
    if ((threadIdx.x & 63) == 0 && seen) { atomicAdd(&pl_acc[0], hit); atomicAdd(&pl_acc[1], seen); }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nh; b += blockDim.x) {
    int64_t* dst = b < CC && conf[0] ? conf[0] + b : conf[1] + (b - (conf[0] ? CC : 0));
    if (pl_hist[b]) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)pl_hist[b]);
  }
  if (acc_mask && threadIdx.x < 2 && pl_acc[threadIdx.x])
    atomicAdd(reinterpret_cast<unsigned long long*>(sg.acc_out + threadIdx.x), (unsigned long long)pl_acc[threadIdx.x]);
  double* part = a.partial + (size_t)PL_SEG_TERMS * a.blk0[s] + vb;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (ce[k]) {
      const double sn = block_sum_d(num[k], lds);
      const double sd = block_sum_d(den[k], lds);
      if (threadIdx.x == 0) { part[(size_t)(4 * k) * g] = sn; part[(size_t)(4 * k + 1) * g] = sd; }
    }
    if (kl[k]) {
      const double sk = block_sum_d(ksum[k], lds);
      if (threadIdx.x == 0) part[(size_t)(4 * k + 2) * g] = sk;
    }
    if (ent[k]) {
      const double se = block_sum_d(esum[k], lds);
      if (threadIdx.x == 0) part[(size_t)(4 * k + 3) * g] = se;
    }
  }
}

struct PointLossSegFin {
  int blk0[PL_MAXSEG + 1];
  int has[PL_MAXSEG];        // bit 4k / 4k+1 / 4k+2: CE / KL / entropy term of network k
  double kl_scale[PL_MAXSEG];    // 1 / n_s
  double ent_scale[PL_MAXSEG];   // -1 / (n_s log2 C)
  const double* partial;
  float* scalars;            // [S][2][stride]: ce, den, kl, ent
  int stride;                // 4; 3 in the one-call layout, which has no entropy term
};

// One block per segment: k_wce_finalize's / k_scalar_finalize's sums over the segment's g_s partials.
__global__ void k_point_losses_seg_finalize(PointLossSegFin f) {
  __shared__ double lds[8];
  const int s = blockIdx.x, n = f.blk0[s + 1] - f.blk0[s], has = f.has[s];
  const double* base = f.partial + (size_t)PL_SEG_TERMS * f.blk0[s];
  for (int k = 0; k < 2; ++k) {
    float* out = f.scalars + (2 * s + k) * f.stride;
    if (has >> (4 * k) & 1) {
      const double* p = base + (size_t)(4 * k) * n;
      double a = 0.0, b = 0.0;
      for (int i = threadIdx.x; i < n; i += blockDim.x) { a += p[i]; b += p[n + i]; }
      const double sn = block_sum_d(a, lds);
      const double sd = block_sum_d(b, lds);
      if (threadIdx.x == 0) { out[0] = (float)(sn / sd); out[1] = (float)sd; }
    }
    if (has >> (4 * k + 1) & 1) {
      const double* p = base + (size_t)(4 * k + 2) * n;
      double acc = 0.0;
      for (int i = threadIdx.x; i < n; i += blockDim.x) acc += p[i];
      const double sk = block_sum_d(acc, lds);
      if (threadIdx.x == 0) out[2] = (float)(sk * f.kl_scale[s]);
    }
    if (has >> (4 * k + 2) & 1) {
      const double* p = base + (size_t)(4 * k + 3) * n;
      double acc = 0.0;
      for (int i = threadIdx.x; i < n; i += blockDim.x) acc += p[i];
      const double se = block_sum_d(acc, lds);
      if (threadIdx.x == 0) out[3] = (float)(se * f.ent_scale[s]);
    }
  }
}

struct PointLossSegBwdArgs {
  PointLossSeg seg[PL_MAXSEG];
  int blk0[PL_MAXSEG + 1];   // over the segments this network takes part in
  const float* z_main;
  const float* z_xm;
  const float* z_other;
  const float* w;
  int64_t ignore;
  int S, C, net;
  float log2c;
  const float* scalars;
  const float* g;            // [S][3]: upstream gradients of (ce, kl, ent)
  float* dz_main;
  float* dz_xm;
};

// One network's gradients over all of its rows: per segment k_point_losses_bwd's expressions with gce = g_ce / den_s and
// gkl = g_kl / n_s, zeros where the segment has no term for a head, and the entropy part
//   -g_ent / (n_s log2 C) * p_c * (t_c - sum_i p_i t_i),  t = ent_slope(p)
// added to dz_main after the CE / KL parts (add_parts: no multiply is contracted into either add).
__global__ __launch_bounds__(LOSS_BLOCK) void k_point_losses_seg_bwd(PointLossSegBwdArgs a) {
  const int s = seg_of_block(a.blk0, a.S);
  const PointLossSeg& sg = a.seg[s];
  const int vb = blockIdx.x - a.blk0[s], gb = a.blk0[s + 1] - a.blk0[s], N = (int)sg.n;
  const int C = a.C, k = a.net, flags = (int)sg.flags;
  const int64_t* y = sg.y[k];
  const float* w = (flags & PL_SEG_WEIGHTED) ? a.w : nullptr;
  const bool ce = y != nullptr;
  const bool kl = (flags & PL_SEG_KL) && sg.row0[1 - k] >= 0 && a.z_xm && a.z_other;
  const bool ent = flags & PL_SEG_MINENT;
  const bool one_head = !a.z_xm || a.z_xm == a.z_main;   // dz_main is the only output
  const bool shared = kl && one_head;
  const float* gs = a.g + 3 * s;
  const float gce = ce ? gs[0] / a.scalars[8 * s + 4 * k + 1] : 0.f;
  const float gkl = kl ? gs[1] / (float)N : 0.f;
  const float gent = ent ? -gs[2] / ((float)N * a.log2c) : 0.f;
  const float* z_main = a.z_main + sg.row0[k] * C;
  const float* z_xm = kl ? a.z_xm + sg.row0[k] * C : nullptr;
  const float* z_other = kl ? a.z_other + sg.row0[1 - k] * C : nullptr;
  float* dz_main = a.dz_main + sg.row0[k] * C;
  float* dz_xm = one_head ? nullptr : a.dz_xm + sg.row0[k] * C;
  for (int i = vb * blockDim.x + threadIdx.x; i < N; i += gb * blockDim.x) {
    int64_t yi = 0;
    bool keep = false;
    if (ce) {
      yi = y[i];
      keep = !(yi == a.ignore || yi < 0 || yi >= C);
    }
    const float* zr = z_main + (int64_t)i * C;
    float l = 0.f, sc = 0.f;
    if (keep) {
      l = row_lse(zr, C);
      sc = gce * (w ? w[yi] : 1.f);
    }
    float le = 0.f, dot = 0.f;
    if (ent) {
      le = keep ? l : row_lse(zr, C);
      for (int c = 0; c < C; ++c) {
        const float p = expf(zr[c] - le);
        dot += p * ent_slope(p);
      }
    }
    float* d = dz_main + (int64_t)i * C;
    if (shared) {
      const float* br = z_other + (int64_t)i * C;
      const float la = keep ? l : (ent ? le : row_lse(zr, C)), lb = row_lse(br, C);
      for (int c = 0; c < C; ++c) {
        const float pk = gkl * (expf(zr[c] - la) - expf(br[c] - lb));
        float v;
        if (ce) v = add_parts(keep ? sc * (expf(zr[c] - l) - (c == yi ? 1.f : 0.f)) : 0.f, pk);
        else v = pk;
        if (ent) {
          const float p = expf(zr[c] - le);
          v = add_parts(v, gent * p * (ent_slope(p) - dot));
        }
        d[c] = v;
      }
      continue;
    }
    for (int c = 0; c < C; ++c) {
      float v = keep ? sc * (expf(zr[c] - l) - (c == yi ? 1.f : 0.f)) : 0.f;
      if (ent) {
        const float p = expf(zr[c] - le);
        v = add_parts(v, gent * p * (ent_slope(p) - dot));
      }
      d[c] = v;
    }
    if (dz_xm) {
      float* dx = dz_xm + (int64_t)i * C;
      if (kl) {
        const float* ar = z_xm + (int64_t)i * C;
        const float* br = z_other + (int64_t)i * C;
        const float la = row_lse(ar, C), lb = row_lse(br, C);
        for (int c = 0; c < C; ++c) dx[c] = gkl * (expf(ar[c] - la) - expf(br[c] - lb));
      } else {
        for (int c = 0; c < C; ++c) dx[c] = 0.f;
      }
    }
  }
}

MOPA_API size_t mopa_point_losses_seg_workspace_bytes(int32_t S) {
  return align_up((size_t)(S > 0 ? S : 1) * PL_SEG_TERMS * PL_MAXGRID * sizeof(double), 256);
}

// Checks one network's column of the table: its row0 entries are -1 or the running sum of the rows before (the network's rows
// are the concatenation of its segments), every one given needs the logits, and the sum is the tensor's row count.
static bool seg_rows_ok(const PointLossSeg* sg, int S, int k, const float* z, int64_t n_rows) {
  int64_t at = 0;
  for (int s = 0; s < S; ++s) {
    if (sg[s].n < 0 || sg[s].n > INT32_MAX) return false;
    if (sg[s].row0[k] < 0) {
      if (sg[s].row0[k] != -1) return false;
      continue;
    }
    if (!z || sg[s].row0[k] != at) return false;
    at += sg[s].n;
  }
  return at == (z ? n_rows : 0);
}

// The terms of one segment (PointLossSegFin::has): per network a CE term where labels are given, a KL term with flag 1 where both
// networks take part and the network's KL head is given, an entropy term with flag 4 where the network takes part.
static int seg_terms(const PointLossSeg& d, const float* const* zx) {
  int has = 0;
  for (int k = 0; k < 2; ++k) {
    if (d.y[k]) has |= 1 << (4 * k);
    if ((d.flags & PL_SEG_KL) && d.row0[0] >= 0 && d.row0[1] >= 0 && zx[k]) has |= 2 << (4 * k);
    if ((d.flags & PL_SEG_MINENT) && d.row0[k] >= 0) has |= 4 << (4 * k);
  }
  return has;
}

// The forward launch pair over a table its entry point has checked; `stride` floats of `scalars` per network.
static int launch_point_losses(const float* const* zm, const float* const* zx, const float* w, const PointLossSeg* sg, int S, int C,
                               int64_t ignore, float* scalars, int stride, int32_t* status, void* ws, void* stream) {
  PointLossSegArgs a;
  PointLossSegFin f;
  int grid = 0;
  size_t lds = 0;
  for (int s = 0; s < S; ++s) {
    const PointLossSeg& d = sg[s];
    a.seg[s] = d;
    a.blk0[s] = f.blk0[s] = grid;
    grid += d.n > 0 ? stream_grid(d.n, LOSS_BLOCK) : 0;   // <= PL_MAXGRID each
    f.has[s] = seg_terms(d, zx);
    f.kl_scale[s] = 1.0 / (double)d.n;                    // n = 0: inf, and 0 * inf = NaN as .mean() of nothing
    f.ent_scale[s] = -1.0 / ((double)d.n * log2((double)C));
    const size_t need = (size_t)((d.conf[0] ? 1 : 0) + (d.conf[1] ? 1 : 0)) * C * C * sizeof(int);   // <= 32 KB at MAXC
    lds = need > lds ? need : lds;
  }
  for (int s = S; s <= PL_MAXSEG; ++s) a.blk0[s] = f.blk0[s] = grid;
  a.zm[0] = zm[0]; a.zm[1] = zm[1]; a.zx[0] = zx[0]; a.zx[1] = zx[1];
  a.w = w; a.ignore = ignore; a.S = S; a.C = C;
  a.partial = (double*)ws; a.status = status;
  f.partial = (const double*)ws; f.scalars = scalars; f.stride = stride;
  hipStream_t st = (hipStream_t)stream;
  if (grid) k_point_losses_seg<<<grid, LOSS_BLOCK, lds, st>>>(a);
  k_point_losses_seg_finalize<<<S, 256, 0, st>>>(f);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// The loss-and-metric block of all row segments of a merged pass.  z*_main / z*_xm (N2 | N3, C) fp32 contiguous, as in
// mopa_point_losses_fwd (z*_xm null: that network has no KL term).  segs_host: S <= 8 descriptors of ten int64 each --
// n, row0_2d, row0_3d (-1: the network takes no part), y_2d, y_3d, acc_mask, conf_2d, conf_3d, acc_out (device pointers,
// nullable), flags (1 kl, 2 weighted, 4 minent).  Per segment and network: a CE term where labels are given, a KL term with
// flag 1 where both networks take part, an entropy term with flag 4.  scalars fp32 [S][2][4] = (ce, den, kl, ent); the
// entries of absent terms are left untouched; a segment of 0 rows gives NaN terms.  status as mopa_point_losses_fwd, shared.
MOPA_API int mopa_point_losses_seg_fwd(const float* z2_main, const float* z2_xm, const float* z3_main, const float* z3_xm,
                                       const float* class_weight, const int64_t* segs_host, int32_t S, int64_t N2, int64_t N3,
                                       int32_t C, int64_t ignore_index, float* scalars, int32_t* status, void* ws, size_t ws_bytes,
                                       void* stream) {
  if (S <= 0 || S > PL_MAXSEG || C <= 0 || C > MAXC || !scalars || !segs_host || N2 < 0 || N3 < 0) return MOPA_ERR_ARG;
  if ((z2_xm && !z2_main) || (z3_xm && !z3_main)) return MOPA_ERR_ARG;
  const PointLossSeg* sg = reinterpret_cast<const PointLossSeg*>(segs_host);
  if (!seg_rows_ok(sg, S, 0, z2_main, N2) || !seg_rows_ok(sg, S, 1, z3_main, N3)) return MOPA_ERR_ARG;
  const float* zm[2] = {z2_main, z3_main};
  const float* zx[2] = {z2_xm, z3_xm};
  int any = 0;
  for (int s = 0; s < S; ++s) {
    const PointLossSeg& d = sg[s];
    if (d.flags & ~(int64_t)(PL_SEG_KL | PL_SEG_WEIGHTED | PL_SEG_MINENT)) return MOPA_ERR_ARG;
    if ((d.flags & PL_SEG_MINENT) && C < 2) return MOPA_ERR_ARG;   // the reference divides by log2(1)
    for (int k = 0; k < 2; ++k) {
      if (d.y[k] && (d.row0[k] < 0 || !status)) return MOPA_ERR_ARG;
      if (d.conf[k] && !d.y[k]) return MOPA_ERR_ARG;
    }
    if (d.acc_mask && (!d.y[1] || !d.acc_out)) return MOPA_ERR_ARG;
    any |= seg_terms(d, zx);
  }
  if (!any) return MOPA_ERR_ARG;
  if (ws_bytes < mopa_point_losses_seg_workspace_bytes(S)) return MOPA_ERR_WORKSPACE;
  return launch_point_losses(zm, zx, class_weight, sg, S, C, ignore_index, scalars, 4, status, ws, stream);
}

// One network's backward over all of its N rows (net 0: the 2D network, 1: the 3D network), the same table.  z_main (N, C) and
// dz_main are needed; z_xm with dz_xm when the network has KL terms (z_xm == z_main needs dz_xm == dz_main), z_other_main
// (N_other, C) is the other network's main head, the detached KL target.  scalars: mopa_point_losses_seg_fwd's (the
// normalisers); g fp32 [S][3]: upstream gradients of (ce, kl, ent) per segment.  Every row of dz_main -- and of dz_xm on a dual
// head -- is written: zeros where its segment has no term for that head.
MOPA_API int mopa_point_losses_seg_bwd(int32_t net, const float* z_main, const float* z_xm, const float* z_other_main,
                                       const float* class_weight, const int64_t* segs_host, int32_t S, int64_t N, int64_t N_other,
                                       int32_t C, int64_t ignore_index, const float* scalars, const float* g, float* dz_main,
                                       float* dz_xm, void* stream) {
  if (net < 0 || net > 1 || S <= 0 || S > PL_MAXSEG || C <= 0 || C > MAXC || !segs_host || N < 0 || N_other < 0) return MOPA_ERR_ARG;
  if (!z_main || !dz_main || !scalars || !g) return MOPA_ERR_ARG;
  if ((z_xm != nullptr) != (dz_xm != nullptr) || (z_xm && !z_other_main)) return MOPA_ERR_ARG;
  if (z_xm && (z_xm == z_main) != (dz_xm == dz_main)) return MOPA_ERR_ARG;
  const PointLossSeg* sg = reinterpret_cast<const PointLossSeg*>(segs_host);
  if (!seg_rows_ok(sg, S, net, z_main, N)) return MOPA_ERR_ARG;
  if (z_other_main && !seg_rows_ok(sg, S, 1 - net, z_other_main, N_other)) return MOPA_ERR_ARG;
  PointLossSegBwdArgs a;
  int grid = 0;
  for (int s = 0; s < S; ++s) {
    const PointLossSeg& d = sg[s];
    if (d.flags & ~(int64_t)(PL_SEG_KL | PL_SEG_WEIGHTED | PL_SEG_MINENT)) return MOPA_ERR_ARG;
    if ((d.flags & PL_SEG_MINENT) && C < 2) return MOPA_ERR_ARG;
    if (d.y[net] && d.row0[net] < 0) return MOPA_ERR_ARG;
    a.seg[s] = d;
    a.blk0[s] = grid;
    grid += (d.row0[net] >= 0 && d.n > 0) ? stream_grid(d.n, LOSS_BLOCK) : 0;
  }
  for (int s = S; s <= PL_MAXSEG; ++s) a.blk0[s] = grid;
  a.z_main = z_main; a.z_xm = z_xm; a.z_other = z_other_main; a.w = class_weight; a.ignore = ignore_index;
  a.S = S; a.C = C; a.net = net; a.log2c = log2f((float)C);
  a.scalars = scalars; a.g = g; a.dz_main = dz_main; a.dz_xm = dz_xm;
  if (grid) k_point_losses_seg_bwd<<<grid, LOSS_BLOCK, 0, (hipStream_t)stream>>>(a);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// ------------------------------------------------------------------------------------------ ... and over one domain half
// The one-call form.  Forward: one segment of N rows that both networks (where given) take part in, through the segment
// kernels, in its own memory layout (scalars at 3 floats per network).  Backward: a kernel of its own, see above.
MOPA_API size_t mopa_point_losses_workspace_bytes(int64_t n_rows) { return mopa_point_losses_seg_workspace_bytes(1); }

// z*_main / z*_xm (N, C) fp32 contiguous; a network's KL term exists when its z*_xm and the OTHER network's z*_main are given
// (z*_xm may equal z*_main: no dual head), its CE term and confusion matrix when its z*_main and y are.  y2 / y3 (N,) int64,
// may be the same pointer.  class_weight (C,) or null.  scalars fp32[8]: ce_2d, den_2d, kl_2d, ce_3d, den_3d, kl_3d, two spare;
// the entries of absent terms are left untouched.  conf_2d / conf_3d (C, C) int64, rows = label, ADDED to, nullable.
// acc_mask (N,) uint8 nullable with acc_out int64[2], ADDED to: #(mask && argmax(z3_main) == y3), #mask.
// status: device int, bit0 set when a label is outside [0,C) and != ignore (as mopa_wce_fwd).
MOPA_API int mopa_point_losses_fwd(const float* z2_main, const float* z2_xm, const float* z3_main, const float* z3_xm,
                                   const int64_t* y2, const int64_t* y3, const float* class_weight, int32_t N, int32_t C,
                                   int64_t ignore_index, float* scalars, int64_t* conf_2d, int64_t* conf_3d,
                                   const uint8_t* acc_mask, int64_t* acc_out, int32_t* status, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (N <= 0 || C <= 0 || C > MAXC || !scalars) return MOPA_ERR_ARG;
  if ((y2 && !z2_main) || (y3 && !z3_main) || ((y2 || y3) && !status)) return MOPA_ERR_ARG;
  if ((conf_2d && !y2) || (conf_3d && !y3)) return MOPA_ERR_ARG;
  if (acc_mask && (!y3 || !acc_out)) return MOPA_ERR_ARG;
  const int has = (y2 ? 1 : 0) | (z2_xm && z3_main ? 2 : 0) | (y3 ? 4 : 0) | (z3_xm && z2_main ? 8 : 0);
  if (!has) return MOPA_ERR_ARG;
  if (ws_bytes < mopa_point_losses_workspace_bytes(N)) return MOPA_ERR_WORKSPACE;
  const float* zm[2] = {z2_main, z3_main};
  const float* zx[2] = {z2_xm, z3_xm};
  for (int k = 0; k < 2; ++k)   // a KL head given without its own main head: it takes the main head's place, the other's KL has no target
    if (!zm[k] && zx[k] && zm[1 - k]) { zm[k] = zx[k]; zx[1 - k] = nullptr; }
  PointLossSeg d = {};
  d.n = N;
  d.row0[0] = zm[0] ? 0 : -1; d.row0[1] = zm[1] ? 0 : -1;
  d.y[0] = y2; d.y[1] = y3; d.acc_mask = acc_mask;
  d.conf[0] = conf_2d; d.conf[1] = conf_3d; d.acc_out = acc_out;
  d.flags = ((has & 10) ? PL_SEG_KL : 0) | (class_weight ? PL_SEG_WEIGHTED : 0);
  return launch_point_losses(zm, zx, class_weight, &d, 1, C, ignore_index, scalars, 3, status, ws, stream);
}

// One network's gradients: dz_main = d(g[0] ce)/dz_main (k_wce_bwd's expression), dz_xm = d(g[1] kl)/dz_xm (k_kl_bwd's);
// on a shared head (z_xm == z_main, dz_xm == dz_main) the sum of the two.
__global__ __launch_bounds__(LOSS_BLOCK) void k_point_losses_bwd(const float* __restrict__ z_main, const float* __restrict__ z_xm,
                                                                  const float* __restrict__ z_other, const int64_t* __restrict__ y,
                                                                  const float* __restrict__ w, int N, int C, int64_t ignore,
                                                                  const float* __restrict__ den, const float* __restrict__ g,
                                                                  float* dz_main, float* dz_xm) {
  const bool ce = y != nullptr, kl = z_other != nullptr, shared = kl && z_xm == z_main;
  const float gce = ce ? g[0] / *den : 0.f;
  const float gkl = kl ? g[1] / (float)N : 0.f;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    int64_t yi = 0;
    bool keep = false;
    if (ce) {
      yi = y[i];
      keep = !(yi == ignore || yi < 0 || yi >= C);
    }
    const float* zr = z_main + (int64_t)i * C;
    float l = 0.f, s = 0.f;
    if (keep) {
      l = row_lse(zr, C);
      s = gce * (w ? w[yi] : 1.f);
    }
    if (shared) {
      const float* br = z_other + (int64_t)i * C;
      const float la = keep ? l : row_lse(zr, C), lb = row_lse(br, C);
      float* d = dz_main + (int64_t)i * C;
      for (int c = 0; c < C; ++c) {
        const float pk = gkl * (expf(zr[c] - la) - expf(br[c] - lb));
        if (ce) d[c] = add_parts(keep ? s * (expf(zr[c] - l) - (c == yi ? 1.f : 0.f)) : 0.f, pk);
        else d[c] = pk;
      }
      continue;
    }
    if (ce) {
      float* d = dz_main + (int64_t)i * C;
      if (keep) for (int c = 0; c < C; ++c) d[c] = s * (expf(zr[c] - l) - (c == yi ? 1.f : 0.f));
      else for (int c = 0; c < C; ++c) d[c] = 0.f;
    }
    if (kl) {
      const float* ar = z_xm + (int64_t)i * C;
      const float* br = z_other + (int64_t)i * C;
      const float la = row_lse(ar, C), lb = row_lse(br, C);
      for (int c = 0; c < C; ++c) dz_xm[(int64_t)i * C + c] = gkl * (expf(ar[c] - la) - expf(br[c] - lb));
    }
  }
}

// One network's backward.  y null: no CE part; z_other_main (the detached KL target) null: no KL part.  den: the network's
// normaliser in `scalars`; g fp32[2]: upstream gradients of (ce, kl).  z_xm == z_main (shared head) needs dz_xm == dz_main,
// which then receives the sum of the two parts; otherwise dz_main gets the CE part and dz_xm the KL part.
MOPA_API int mopa_point_losses_bwd(const float* z_main, const float* z_xm, const float* z_other_main, const int64_t* y,
                                   const float* class_weight, int32_t N, int32_t C, int64_t ignore_index, const float* den,
                                   const float* g, float* dz_main, float* dz_xm, void* stream) {
  if (N <= 0 || C <= 0 || C > MAXC || !g) return MOPA_ERR_ARG;
  if (!y && !z_other_main) return MOPA_ERR_ARG;
  if (y && (!z_main || !den || !dz_main)) return MOPA_ERR_ARG;
  if (z_other_main && (!z_xm || !dz_xm)) return MOPA_ERR_ARG;
  if (z_xm && (z_xm == z_main) != (dz_xm == dz_main)) return MOPA_ERR_ARG;
  k_point_losses_bwd<<<stream_grid(N, LOSS_BLOCK), LOSS_BLOCK, 0, (hipStream_t)stream>>>(
      z_main, z_xm, z_other_main, y, class_weight, N, C, ignore_index, den, g, dz_main, dz_xm);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// ------------------------------------------------------------------------------------------ softmax over the last dim
__global__ void k_softmax_fwd(const float* __restrict__ z, int64_t N, int C, float* __restrict__ p) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const float* zr = z + i * C;
    const float l = row_lse(zr, C);
    for (int c = 0; c < C; ++c) p[i * C + c] = row_softmax_at(zr[c], l);
  }
}
// dz = p * (dp - sum_c dp*p)
__global__ void k_softmax_bwd(const float* __restrict__ p, const float* __restrict__ dp, int64_t N, int C, float* __restrict__ dz) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    float dot = 0.f;
    for (int c = 0; c < C; ++c) dot = fmaf(p[i * C + c], dp[i * C + c], dot);
    for (int c = 0; c < C; ++c) dz[i * C + c] = p[i * C + c] * (dp[i * C + c] - dot);
  }
}
MOPA_API int mopa_softmax_fwd(const float* logits, int64_t n_rows, int32_t C, float* probs, void* stream) {
  if (n_rows <= 0 || C <= 0 || C > MAXC) return MOPA_ERR_ARG;
  k_softmax_fwd<<<stream_grid(n_rows, 256), 256, 0, (hipStream_t)stream>>>(logits, n_rows, C, probs);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
MOPA_API int mopa_softmax_bwd(const float* probs, const float* dprobs, int64_t n_rows, int32_t C, float* dlogits, void* stream) {
  if (n_rows <= 0 || C <= 0 || C > MAXC) return MOPA_ERR_ARG;
  k_softmax_bwd<<<stream_grid(n_rows, 256), 256, 0, (hipStream_t)stream>>>(probs, dprobs, n_rows, C, dlogits);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// ------------------------------------------------------------------------------------------ SAM-mask consistency loss
// probs (B, HW, C); masks (B, HW) int32 with ids in [0, MAXID) valid, negative = ignore (loss.py:265-266).
// Per (image b, id m): n = #pixels, mu = mean_n P, V = sum_{n,c} (P - mu)^2.
//   loss_m = V / (n C) - [min_entropy] sum_c mu_c log2(mu_c + 1e-30) / log2(Knorm)     (Knorm = probs.shape[1], B.2)
//   loss   = mean_b ( mean_{m valid in b} loss_m )   (an image without valid ids adds 0 but counts, loss.py:278-281)
// Two segmented-reduction passes (means, then centred squares) keep fp32 accurate.  The per-id sums are ORDERED: a wave
// takes 64 consecutive pixels (lane = pixel), walks the distinct ids among them (leader = the first lane not yet served)
// and sums the matching lanes with the fixed xor-butterfly of wave_sum -- wavefront shuffles, no float atomics -- into
// a wave-private LDS accumulator that a single lane per channel read-add-writes; the waves of a block take their
// 64-pixel groups in a fixed order and their accumulators are added in wave order; per-block slabs + an ordered slab
// reduction.  Same bits run to run (tests/test_gpu_losses.py::test_mask_cons_loss_is_bit_reproducible).  SAM masks are
// spatially coherent: a group of 64 row-adjacent pixels holds 1-3 ids, so the leader loop is short.
#define MAXID 256
#define MC_PIX_PER_BLOCK 4096

static inline int mc_waves(int W) {   // waves per block: the wave-private accumulators have to fit 64 KB of LDS
  const int nw = 65536 / (MAXID * W * (int)sizeof(float));
  return nw >= 4 ? 4 : nw >= 2 ? 2 : 1;
}

__global__ __launch_bounds__(256) void k_mc_pass(const float* __restrict__ probs, const int* __restrict__ masks, int HW, int C,
                                                  const float* __restrict__ mu /*null in pass 1: [B][MAXID][C]*/,
                                                  float* __restrict__ slabs /*[B][nblk][MAXID][W]*/, int nblk, int W) {
  extern __shared__ float acc[];  // [waves][MAXID][W]   pass1: W=C+1 (sums, count) ; pass2: W=1 (centred squares)
  const int b = blockIdx.y, nthr = blockDim.x, nw = nthr >> 6;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < nw * MAXID * W; i += nthr) acc[i] = 0.f;
  __syncthreads();
  float* mine = acc + wv * MAXID * W;
  const int p0 = blockIdx.x * MC_PIX_PER_BLOCK, p1 = min(HW, p0 + MC_PIX_PER_BLOCK);
  for (int g0 = p0 + wv * 64; g0 < p1; g0 += nthr) {   // wave-uniform: whole groups of 64 pixels
    const int pix = g0 + lane;
    int id = pix < p1 ? masks[(int64_t)b * HW + pix] : -1;
    if (id >= MAXID) id = -1;
    const float* pr = probs + ((int64_t)b * HW + (pix < p1 ? pix : p0)) * C;
    float v2 = 0.f;
    if (mu && id >= 0) {
      const float* m = mu + ((int64_t)b * MAXID + id) * C;
      for (int c = 0; c < C; ++c) { const float d = pr[c] - m[c]; v2 = fmaf(d, d, v2); }
    }
    unsigned long long todo = __ballot(id >= 0);
    while (todo) {
      const int lid = __shfl(id, __ffsll((long long)todo) - 1, 64);
      const bool hit = id == lid;
      const unsigned long long mb = __ballot(hit);
      todo &= ~mb;
      if (!mu) {
        float keep = 0.f;   // lane c ends up with channel c's sum, lane C with the pixel count
        for (int c = 0; c < C; ++c) {
          const float s = wave_sum(hit ? pr[c] : 0.f);
          if (lane == c) keep = s;
        }
        if (lane == C) keep = (float)__popcll(mb);
        if (lane <= C) mine[lid * W + lane] += keep;
      } else {
        const float s = wave_sum(hit ? v2 : 0.f);
        if (lane == 0) mine[lid] += s;
      }
    }
  }
  __syncthreads();
  float* dst = slabs + ((int64_t)b * nblk + blockIdx.x) * MAXID * W;
  for (int i = threadIdx.x; i < MAXID * W; i += nthr) {
    float s = acc[i];
    for (int w = 1; w < nw; ++w) s += acc[w * MAXID * W + i];
    dst[i] = s;
  }
}

// tab[b][id] = {n, V} ; mu[b][id][c]
__global__ void k_mc_means(const float* __restrict__ slabs, int nblk, int C, float* __restrict__ mu, float* __restrict__ cnt) {
  const int b = blockIdx.y, W = C + 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < MAXID * W; i += gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += (double)slabs[((int64_t)b * nblk + k) * MAXID * W + i];
    const int id = i / W, c = i - id * W;
    if (c == C) cnt[b * MAXID + id] = (float)s;
    else mu[((int64_t)b * MAXID + id) * C + c] = (float)s;  // still a sum; divided below once cnt is known
  }
}
__global__ void k_mc_divide(float* __restrict__ mu, const float* __restrict__ cnt, int B, int C) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * MAXID * C; i += gridDim.x * blockDim.x) {
    const float n = cnt[i / C];
    mu[i] = n > 0.f ? mu[i] / n : 0.f;
  }
}
// one block: per-image / total loss; also nvalid[b] (number of valid ids) for the backward.
__global__ void k_mc_finalize(const float* __restrict__ slabs2, int nblk, const float* __restrict__ mu, const float* __restrict__ cnt,
                              int B, int C, float log2K, int min_entropy, float* __restrict__ nvalid, float* __restrict__ loss) {
  __shared__ double lds[8];
  double total = 0.0;
  for (int b = 0; b < B; ++b) {
    double acc = 0.0, nv = 0.0;
    for (int id = threadIdx.x; id < MAXID; id += blockDim.x) {
      const float n = cnt[b * MAXID + id];
      if (n <= 0.f) continue;
      double V = 0.0;
      for (int k = 0; k < nblk; ++k) V += (double)slabs2[((int64_t)b * nblk + k) * MAXID + id];
      double l = V / ((double)n * C);
      if (min_entropy) {
        double e = 0.0;
        for (int c = 0; c < C; ++c) {
          const float m = mu[((int64_t)b * MAXID + id) * C + c];
          e += (double)(m * log2f(m + 1e-30f));
        }
        l -= e / (double)log2K;
      }
      acc += l;
      nv += 1.0;
    }
    const double sa = block_sum_d(acc, lds);
    const double sv = block_sum_d(nv, lds);
    if (threadIdx.x == 0) nvalid[b] = (float)sv;
    if (sv > 0.0) total += sa / sv;
  }
  if (threadIdx.x == 0) *loss = (float)(total / B);
}
// dP = g/(B*M_b) * [ 2 (P - mu)/(n C) - (log2(mu+1e-30) + mu/((mu+1e-30) ln2)) / (n log2K) ]
__global__ void k_mc_bwd(const float* __restrict__ probs, const int* __restrict__ masks, int B, int HW, int C, const float* __restrict__ mu,
                         const float* __restrict__ cnt, const float* __restrict__ nvalid, float log2K, int min_entropy,
                         const float* __restrict__ gout, float* __restrict__ dprobs) {
  const float g = *gout / (float)B;
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW);
    const int id = masks[i];
    float* d = dprobs + i * C;
    if (id < 0 || id >= MAXID) {
      for (int c = 0; c < C; ++c) d[c] = 0.f;
      continue;
    }
    const float n = cnt[b * MAXID + id];
    const float s = g / nvalid[b];
    const float* m = mu + ((int64_t)b * MAXID + id) * C;
    for (int c = 0; c < C; ++c) {
      float v = 2.f * (probs[i * C + c] - m[c]) / (n * C);
      if (min_entropy) v -= (log2f(m[c] + 1e-30f) + m[c] / ((m[c] + 1e-30f) * 0.6931471805599453f)) / (n * log2K);
      d[c] = s * v;
    }
  }
}

static inline int mc_nblk(int HW) { return (HW + MC_PIX_PER_BLOCK - 1) / MC_PIX_PER_BLOCK; }

// ws layout: slabs1 [B][nblk][MAXID][C+1] | slabs2 [B][nblk][MAXID]
MOPA_API size_t mopa_mask_cons_workspace_bytes(int32_t B, int32_t HW, int32_t C) {
  return align_up((size_t)B * mc_nblk(HW) * MAXID * (C + 2) * sizeof(float), 256);
}
// state (saved for backward): mu [B][MAXID][C] | cnt [B][MAXID] | nvalid [B]   -> (B*MAXID*(C+1) + B) floats
MOPA_API size_t mopa_mask_cons_state_floats(int32_t B, int32_t C) { return (size_t)B * MAXID * (C + 1) + B; }

// k_norm = 1 (a one-row image) only without the entropy term: its normaliser log2(k_norm) would be 0.
MOPA_API int mopa_mask_cons_fwd(const float* probs, const int32_t* masks, int32_t B, int32_t HW, int32_t C, int32_t k_norm,
                                int32_t min_entropy, float* loss, float* state, void* ws, size_t ws_bytes, void* stream) {
  if (B <= 0 || HW <= 0 || C <= 0 || C > 32 || k_norm < 1 || (min_entropy && k_norm < 2)) return MOPA_ERR_ARG;
  if (ws_bytes < mopa_mask_cons_workspace_bytes(B, HW, C)) return MOPA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = mc_nblk(HW);
  float* slabs1 = (float*)ws;
  float* slabs2 = slabs1 + (size_t)B * nblk * MAXID * (C + 1);
  float* mu = state;
  float* cnt = mu + (size_t)B * MAXID * C;
  float* nvalid = cnt + (size_t)B * MAXID;
  dim3 grid(nblk, B);
  const int nw1 = mc_waves(C + 1), nw2 = mc_waves(1);
  k_mc_pass<<<grid, 64 * nw1, (size_t)nw1 * MAXID * (C + 1) * sizeof(float), st>>>(probs, masks, HW, C, nullptr, slabs1, nblk, C + 1);
  k_mc_means<<<dim3(4, B), 256, 0, st>>>(slabs1, nblk, C, mu, cnt);
  k_mc_divide<<<stream_grid((int64_t)B * MAXID * C, 256), 256, 0, st>>>(mu, cnt, B, C);
  k_mc_pass<<<grid, 64 * nw2, (size_t)nw2 * MAXID * sizeof(float), st>>>(probs, masks, HW, C, mu, slabs2, nblk, 1);
  k_mc_finalize<<<1, 256, 0, st>>>(slabs2, nblk, mu, cnt, B, C, log2f((float)k_norm), min_entropy, nvalid, loss);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
MOPA_API int mopa_mask_cons_bwd(const float* probs, const int32_t* masks, int32_t B, int32_t HW, int32_t C, int32_t k_norm,
                                int32_t min_entropy, const float* state, const float* gout, float* dprobs, void* stream) {
  if (B <= 0 || HW <= 0 || C <= 0 || C > 32 || k_norm < 1 || (min_entropy && k_norm < 2)) return MOPA_ERR_ARG;
  const float* mu = state;
  const float* cnt = mu + (size_t)B * MAXID * C;
  const float* nvalid = cnt + (size_t)B * MAXID;
  k_mc_bwd<<<stream_grid((int64_t)B * HW, 256), 256, 0, (hipStream_t)stream>>>(probs, masks, B, HW, C, mu, cnt, nvalid,
                                                                                log2f((float)k_norm), min_entropy, gout, dprobs);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
