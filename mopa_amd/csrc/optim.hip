// Adam over one flat fp32 parameter buffer (all parameters of a network are views into it, so one launch updates
// the whole model and the same flat gradient buffer is what RCCL all-reduces).  Matches torch.optim.Adam
// (the reference's optimiser: mopa/common/solver/build.py:7-21 -> getattr(torch.optim, 'Adam'), yaml lr 1e-3):
//   g += wd * p;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
//   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
//
// Gradient statistics and the guarded update (opt-in; FlatAdam(max_grad_norm=, skip_nonfinite=)): mopa_grad_stats reads the flat
// gradient once and leaves, in device memory, the norm / max |g| / non-finite count of every parameter and a 32-byte step record
// (total norm, clip coefficient of torch.nn.utils.clip_grad_norm_, go / no-go); mopa_adam_flat_guarded is k_adam_flat's body behind
// that record.  No host read anywhere, no atomics: slab records summed in a fixed order (same bits run to run, whatever the grid).
//
// The same for the other optimizers the reference's config can name (FlatSGD, FlatAdamW): mopa_sgd_flat == torch.optim.SGD
// (momentum, dampening, Nesterov, L2 weight decay), mopa_adamw_flat == torch.optim.AdamW (decoupled weight decay), each with a
// guarded form behind the same step record.
#include "common.h"

// The update of both Adam kernels: ONE body, so that the guarded kernel with coef == 1 leaves the plain kernel's bits.  Which
// products fuse into an FMA is WRITTEN OUT (contraction is off in this function): left to the compiler it follows the code around
// the expression -- the same source inlined into a second kernel fused other operands than k_adam_flat did on its own (the same
// instruction counts, other bits; DESIGN 3.3 item 8 saw it across translation units).  The choices below are the ones every
// build of k_adam_flat so far has made, float4 loop and scalar tail each as it was, so no trained weight moves by a bit.
__device__ __forceinline__ void adam_flat_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                               float wd, float bc1, float bc2_sqrt, float grad_scale, int64_t first,
                                               int64_t stride) {
#pragma clang fp contract(off)
  const int64_t n4 = n >> 2;
  const float step = lr / bc1;
  for (int64_t i = first; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    float* pp = &pv.x; const float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gg = __builtin_fmaf(gp[k], grad_scale, wd * pp[k]);
      mp[k] = __builtin_fmaf(b1, mp[k], (1.f - b1) * gg);
      vp[k] = __builtin_fmaf(b2, vp[k], (1.f - b2) * gg * gg);
      pp[k] -= step * mp[k] / (sqrtf(vp[k]) / bc2_sqrt + eps);
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  for (int64_t i = (n4 << 2) + first; i < n; i += stride) {   // (only the first sum was ever fused here)
    const float gg = __builtin_fmaf(g[i], grad_scale, wd * p[i]);
    m[i] = b1 * m[i] + (1.f - b1) * gg;
    v[i] = b2 * v[i] + (1.f - b2) * gg * gg;
    p[i] -= step * m[i] / (sqrtf(v[i]) / bc2_sqrt + eps);
  }
}

__global__ __launch_bounds__(256) void k_adam_flat(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                                    float wd, float bc1, float bc2_sqrt, float grad_scale) {
  adam_flat_body(p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
                 (int64_t)gridDim.x * blockDim.x);
}

// ---- gradient statistics
#define GS_CHUNK 8192          // floats per chunk: 256 threads x 8 float4 (23.6 M floats of the 2D network = ~2,900 chunks)
#define GS_LOADS (GS_CHUNK / 4 / 256)

struct GsChunk {               // one record of the DEVICE chunk table: grads[lo, hi) belongs to parameter `param`
  int64_t param, lo, hi;       // lo % 4 == 0, 0 <= hi - lo <= GS_CHUNK; records sorted by param (FlatAdam: optim.py::stat_chunks)
};
struct GsSlab {                // what the partial pass leaves per chunk (16 bytes)
  double sumsq;                // sum of g^2 in double (a float product is exact there); NaN / Inf elements go in as they are
  float absmax;                // max |g| over the finite elements
  int nonfinite;               // NaN and +-Inf elements
};
struct GsStepRec {             // the step record (32 bytes) -- read by k_adam_flat_guarded, kept across steps for the counters
  float norm;                  // |grad_scale| * sqrt(sum over the whole buffer)
  int nonfinite;
  float coef;                  // clip_grad_norm_'s factor: max_norm / (norm + 1e-6f) clamped to 1; 1 without clipping
  int applied;                 // !(skip_nonfinite && nonfinite > 0)
  int64_t n_skipped, n_clipped;
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// One block per chunk at a time (grid-stride).  The order of the additions is a function of the chunk alone: thread t adds its
// float4s in index order (t, t + 256, ...) and then tail element t, wave_sum_d's butterfly, the four waves in wave order.
__global__ __launch_bounds__(256) void k_grad_stats_partial(const float* __restrict__ g, const GsChunk* __restrict__ tab, int n_chunks,
                                                             GsSlab* __restrict__ slab) {
  __shared__ double s_sum[4];
  __shared__ float s_max[4];
  __shared__ int s_nf[4];
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t lo = tab[c].lo;
    int64_t len64 = tab[c].hi - lo;
    if (len64 < 0 || lo < 0 || (lo & 3)) len64 = 0;   // a record this kernel cannot read as float4s counts as empty
    const int len = (int)(len64 > GS_CHUNK ? GS_CHUNK : len64), n4 = len >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(g + lo);
    float4 x[GS_LOADS];
#pragma unroll
    for (int k = 0; k < GS_LOADS; ++k) {              // every load in flight before the first add; +0 for the absent ones is exact
      const int i = tid + k * 256;
      x[k] = i < n4 ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float tail = tid < (len & 3) ? g[lo + (n4 << 2) + tid] : 0.f;
    double sum = 0.0;
    float amax = 0.f;
    int nf = 0;
    auto take = [&](float e) {
      const bool fin = (__float_as_uint(e) & 0x7f800000u) != 0x7f800000u;
      sum += (double)e * (double)e;
      amax = fmaxf(amax, fin ? fabsf(e) : 0.f);
      nf += fin ? 0 : 1;
    };
#pragma unroll
    for (int k = 0; k < GS_LOADS; ++k) { take(x[k].x); take(x[k].y); take(x[k].z); take(x[k].w); }
    take(tail);
    sum = wave_sum_d(sum);
    amax = wave_max(amax);
    nf = wave_sum_i(nf);
    if ((tid & 63) == 0) { s_sum[tid >> 6] = sum; s_max[tid >> 6] = amax; s_nf[tid >> 6] = nf; }
    __syncthreads();
    if (tid == 0) {
      GsSlab r;
      r.sumsq = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
      r.absmax = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
      r.nonfinite = s_nf[0] + s_nf[1] + s_nf[2] + s_nf[3];
      slab[c] = r;
    }
    __syncthreads();
  }
}

// One block.  Thread t of a round owns parameter base + t: it finds the parameter's records in the sorted table (two binary
// searches, stepped together) and adds their slabs in chunk order; thread 0 then adds the round's 256 sums in parameter order into
// the running total.  Any number of parameters: nothing here is sized by it.
__global__ __launch_bounds__(256) void k_grad_stats_final(const GsSlab* __restrict__ slab, const GsChunk* __restrict__ tab, int n_chunks,
                                                           int n_params, float gs_abs, float max_norm, int skip_nonfinite,
                                                           float* __restrict__ stats, GsStepRec* __restrict__ rec) {
  __shared__ double s_sum[256];
  __shared__ int s_nf[256];
  const int tid = threadIdx.x;
  float* norm = stats;
  float* absmax = stats + n_params;
  int* nonfinite = reinterpret_cast<int*>(stats + 2 * (int64_t)n_params);
  double total = 0.0;          // thread 0's
  int64_t total_nf = 0;
  for (int base = 0; base < n_params; base += 256) {
    const int p = base + tid;
    double sum = 0.0;
    float amax = 0.f;
    int nf = 0;
    if (p < n_params) {
      int a0 = 0, b0 = n_chunks, a1 = 0, b1 = n_chunks;   // first record with param >= p, and with param >= p + 1
      while (a0 < b0 || a1 < b1) {
        if (a0 < b0) { const int mid = (a0 + b0) >> 1; if (tab[mid].param < p) a0 = mid + 1; else b0 = mid; }
        if (a1 < b1) { const int mid = (a1 + b1) >> 1; if (tab[mid].param <= p) a1 = mid + 1; else b1 = mid; }
      }
      for (int c = a0; c < a1; c += 16) {                 // 16 records in flight per round trip; an absent one adds +0: exact
        GsSlab r[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) r[k] = c + k < a1 ? slab[c + k] : GsSlab{0.0, 0.f, 0};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          sum += r[k].sumsq;
          amax = fmaxf(amax, r[k].absmax);
          nf += r[k].nonfinite;
        }
      }
      norm[p] = (float)(sqrt(sum) * (double)gs_abs);
      absmax[p] = (float)((double)amax * (double)gs_abs);
      nonfinite[p] = nf;
    }
    s_sum[tid] = sum;
    s_nf[tid] = nf;
    __syncthreads();
    if (tid == 0) {                                       // (threads past n_params left zeros)
      for (int j = 0; j < 256 && base + j < n_params; j += 32) {
#pragma unroll
        for (int k = 0; k < 32; ++k) { total += s_sum[j + k]; total_nf += s_nf[j + k]; }
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float tnorm = (float)(sqrt(total) * (double)gs_abs);
    float coef = 1.f;
    if (max_norm > 0.f) {
      const float c = max_norm / (tnorm + 1e-6f);
      coef = c >= 1.f ? 1.f : c;                        // a NaN norm leaves a NaN coefficient, as torch's clamp does
    }
    const int applied = !(skip_nonfinite && total_nf > 0);
    rec->norm = tnorm;
    rec->nonfinite = (int)(total_nf > 0x7fffffff ? 0x7fffffff : total_nf);
    rec->coef = coef;
    rec->applied = applied;
    if (!applied) rec->n_skipped += 1;
    else if (coef < 1.f) rec->n_clipped += 1;
  }
}

// k_adam_flat behind the step record: nothing is stored when the step is not applied, else the gradient is scaled by
// grad_scale * coef -- one multiply, formed once, so coef == 1 is k_adam_flat bit for bit.
__global__ __launch_bounds__(256) void k_adam_flat_guarded(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                                            float wd, float bc1, float bc2_sqrt, float grad_scale,
                                                            const GsStepRec* __restrict__ rec) {
  const int applied = rec->applied;
  const float coef = rec->coef;
  if (!applied) return;
  adam_flat_body(p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale * coef, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
                 (int64_t)gridDim.x * blockDim.x);
}

// ---- AdamW (torch.optim.AdamW): decoupled weight decay, p *= 1 - lr * wd, then Adam's update with no L2 term in the gradient.
// A body of its own, so that adam_flat_body -- and with it every bit mopa_adam_flat has ever left -- stays as it is; the pairings
// are written out for the same reason, the same ones in the float4 loop and in the tail.
__device__ __forceinline__ float adamw_one(float p, float g, float& m, float& v, float decay, float step, float b1, float b2, float eps,
                                           float bc2_sqrt, float grad_scale) {
#pragma clang fp contract(off)
  const float gg = g * grad_scale;
  p = p * decay;
  m = __builtin_fmaf(b1, m, (1.f - b1) * gg);
  v = __builtin_fmaf(b2, v, (1.f - b2) * gg * gg);
  return p - step * m / (sqrtf(v) / bc2_sqrt + eps);
}

__device__ __forceinline__ void adamw_flat_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                                float wd, float bc1, float bc2_sqrt, float grad_scale, int64_t first,
                                                int64_t stride) {
#pragma clang fp contract(off)
  const int64_t n4 = n >> 2;
  const float step = lr / bc1;
  const float decay = 1.f - lr * wd;
  for (int64_t i = first; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    float* pp = &pv.x; const float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) pp[k] = adamw_one(pp[k], gp[k], mp[k], vp[k], decay, step, b1, b2, eps, bc2_sqrt, grad_scale);
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  for (int64_t i = (n4 << 2) + first; i < n; i += stride)
    p[i] = adamw_one(p[i], g[i], m[i], v[i], decay, step, b1, b2, eps, bc2_sqrt, grad_scale);
}

__global__ __launch_bounds__(256) void k_adamw_flat(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                     float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                                     float wd, float bc1, float bc2_sqrt, float grad_scale) {
  adamw_flat_body(p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
                  (int64_t)gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(256) void k_adamw_flat_guarded(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                                             float wd, float bc1, float bc2_sqrt, float grad_scale,
                                                             const GsStepRec* __restrict__ rec) {
  const int applied = rec->applied;
  const float coef = rec->coef;
  if (!applied) return;           // (the decay is part of the step: a skipped step leaves p alone too)
  adamw_flat_body(p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale * coef, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
                  (int64_t)gridDim.x * blockDim.x);
}

// ---- SGD (torch.optim.SGD, element for element):
//   g' = grad_scale g + wd p;  buf = g' on the first applied step, else momentum buf + (1 - dampening) g';
//   u = g' + momentum buf (nesterov) | buf | g' (momentum == 0);  p -= lr u
// `buf` is not touched (and may be null) when momentum == 0.  One body for the plain and the guarded kernel, pairings written out.
__device__ __forceinline__ float sgd_one(float p, float g, float& b, float lr, float mom, float undamp, float wd, bool use_mom,
                                         bool nesterov, bool first, float grad_scale) {
#pragma clang fp contract(off)
  const float gg = __builtin_fmaf(g, grad_scale, wd * p);
  float u = gg;
  if (use_mom) {
    b = first ? gg : __builtin_fmaf(mom, b, undamp * gg);
    u = nesterov ? __builtin_fmaf(mom, b, gg) : b;
  }
  return __builtin_fmaf(-lr, u, p);
}

__device__ __forceinline__ void sgd_flat_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int64_t n,
                                              float lr, float mom, float damp, float wd, bool nesterov, bool first, float grad_scale,
                                              int64_t first_i, int64_t stride) {
#pragma clang fp contract(off)
  const int64_t n4 = n >> 2;
  const bool use_mom = mom != 0.f;
  const float undamp = 1.f - damp;
  for (int64_t i = first_i; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (use_mom && !first) bv = reinterpret_cast<float4*>(buf)[i];
    float* pp = &pv.x; const float* gp = &gv.x; float* bp = &bv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) pp[k] = sgd_one(pp[k], gp[k], bp[k], lr, mom, undamp, wd, use_mom, nesterov, first, grad_scale);
    reinterpret_cast<float4*>(p)[i] = pv;
    if (use_mom) reinterpret_cast<float4*>(buf)[i] = bv;
  }
  for (int64_t i = (n4 << 2) + first_i; i < n; i += stride) {
    float b = (use_mom && !first) ? buf[i] : 0.f;
    p[i] = sgd_one(p[i], g[i], b, lr, mom, undamp, wd, use_mom, nesterov, first, grad_scale);
    if (use_mom) buf[i] = b;
  }
}

__global__ __launch_bounds__(256) void k_sgd_flat(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int64_t n,
                                                   float lr, float mom, float damp, float wd, int nesterov, int first, float grad_scale) {
  sgd_flat_body(p, g, buf, n, lr, mom, damp, wd, nesterov != 0, first != 0, grad_scale, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
                (int64_t)gridDim.x * blockDim.x);
}

// k_sgd_flat behind the step record.  "First" is not the host's to know here (whether step 1 was applied is decided on the device):
// it is read from `buf_valid`, one int32 in device memory that is 0 until a step has been applied.  k_sgd_mark_valid, enqueued
// behind this kernel on the same stream, sets it -- after every thread here has read it.
__global__ __launch_bounds__(256) void k_sgd_flat_guarded(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                           int64_t n, float lr, float mom, float damp, float wd, int nesterov,
                                                           const int* __restrict__ buf_valid, float grad_scale,
                                                           const GsStepRec* __restrict__ rec) {
  const int applied = rec->applied;
  const float coef = rec->coef;
  if (!applied) return;
  const bool first = buf_valid != nullptr && *buf_valid == 0;
  sgd_flat_body(p, g, buf, n, lr, mom, damp, wd, nesterov != 0, first, grad_scale * coef, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
                (int64_t)gridDim.x * blockDim.x);
}

__global__ void k_sgd_mark_valid(int* __restrict__ buf_valid, const GsStepRec* __restrict__ rec) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && rec->applied) *buf_valid = 1;
}

// bias_correction1 = 1 - beta1^t, bias_correction2_sqrt = sqrt(1 - beta2^t) are computed by the caller (host scalars).
// grad_scale multiplies the gradient first (1/world_size after a sum all-reduce).
MOPA_API int mopa_adam_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                            float beta1, float beta2, float eps, float weight_decay, float bias_correction1,
                            float bias_correction2_sqrt, float grad_scale, void* stream) {
  if (n <= 0) return MOPA_ERR_ARG;
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) return MOPA_ERR_ARG;
  k_adam_flat<<<stream_grid(n / 4 + 1, 256), 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2,
                                                                            eps, weight_decay, bias_correction1,
                                                                            bias_correction2_sqrt, grad_scale);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// Floats per chunk of mopa_grad_stats' chunk table (a compile-time constant, a multiple of 4).
MOPA_API int mopa_grad_stats_chunk(void) { return GS_CHUNK; }

// One slab record per chunk.
MOPA_API size_t mopa_grad_stats_workspace_bytes(int64_t n_chunks) { return sizeof(GsSlab) * (size_t)(n_chunks > 0 ? n_chunks : 1); }

// Statistics of grad_scale * grads, per parameter and over the whole buffer, in two launches.
//   chunk_tab  DEVICE table of n_chunks records {int64 param, lo, hi}: grads[lo, hi) is a piece of parameter `param`;
//              lo % 4 == 0, hi - lo <= mopa_grad_stats_chunk(), records sorted by param, every element in exactly one record
//   stats      float norm[n_params], float absmax[n_params], int32 nonfinite[n_params]  (3 * n_params * 4 bytes):
//              norm = (float)(sqrt(sum g^2) * |grad_scale|) formed in double, absmax over the finite elements, scaled alike
//   rec        32 bytes, 8-byte aligned: float norm (NaN / Inf elements propagate), int32 nonfinite, float coef, int32 applied,
//              int64 n_skipped, int64 n_clipped.  coef = max_norm / (norm + 1e-6f) in float, exactly 1 where that is >= 1 or
//              max_norm <= 0; applied = !(skip_nonfinite && nonfinite > 0).  The two counters are ADDED to (zero them once):
//              n_skipped when applied == 0, n_clipped when applied and coef < 1.
//   ws         mopa_grad_stats_workspace_bytes(n_chunks), 16-byte aligned
MOPA_API int mopa_grad_stats(const float* grads, const void* chunk_tab, int64_t n_chunks, int64_t n_params, float grad_scale,
                             float max_norm, int skip_nonfinite, float* stats, void* rec, void* ws, size_t ws_bytes, void* stream) {
  if (n_chunks <= 0 || n_params <= 0 || n_chunks > INT32_MAX || n_params > INT32_MAX / 4) return MOPA_ERR_ARG;
  if (!grads || !chunk_tab || !stats || !rec || !ws) return MOPA_ERR_ARG;
  if (((uintptr_t)grads & 15) != 0 || ((uintptr_t)ws & 15) != 0 || ((uintptr_t)chunk_tab & 7) != 0 || ((uintptr_t)rec & 7) != 0 ||
      ((uintptr_t)stats & 3) != 0)
    return MOPA_ERR_ARG;
  if (ws_bytes < mopa_grad_stats_workspace_bytes(n_chunks)) return MOPA_ERR_WORKSPACE;
  const int grid = (int)(n_chunks < 2048 ? n_chunks : 2048);
  k_grad_stats_partial<<<grid, 256, 0, (hipStream_t)stream>>>(grads, (const GsChunk*)chunk_tab, (int)n_chunks, (GsSlab*)ws);
  MOPA_CHECK_LAUNCH();
  k_grad_stats_final<<<1, 256, 0, (hipStream_t)stream>>>((const GsSlab*)ws, (const GsChunk*)chunk_tab, (int)n_chunks, (int)n_params,
                                                         fabsf(grad_scale), max_norm, skip_nonfinite, stats, (GsStepRec*)rec);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// mopa_adam_flat behind the step record `rec` of mopa_grad_stats (device memory, read by every thread once): no store at all
// when rec.applied == 0, else the same update with grad_scale * rec.coef in place of grad_scale.
MOPA_API int mopa_adam_flat_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, float bias_correction1,
                                    float bias_correction2_sqrt, float grad_scale, const void* rec, void* stream) {
  if (n <= 0 || !rec) return MOPA_ERR_ARG;
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) return MOPA_ERR_ARG;
  if (((uintptr_t)rec & 7) != 0) return MOPA_ERR_ARG;
  k_adam_flat_guarded<<<stream_grid(n / 4 + 1, 256), 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, exp_avg_sq, n, lr, beta1,
                                                                                    beta2, eps, weight_decay, bias_correction1,
                                                                                    bias_correction2_sqrt, grad_scale,
                                                                                    (const GsStepRec*)rec);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// torch.optim.AdamW on the flat buffer: mopa_adam_flat's arguments; weight_decay multiplies the parameter (p *= 1 - lr * wd) and
// stays out of the gradient.
MOPA_API int mopa_adamw_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                             float beta1, float beta2, float eps, float weight_decay, float bias_correction1,
                             float bias_correction2_sqrt, float grad_scale, void* stream) {
  if (n <= 0) return MOPA_ERR_ARG;
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) return MOPA_ERR_ARG;
  k_adamw_flat<<<stream_grid(n / 4 + 1, 256), 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2,
                                                                             eps, weight_decay, bias_correction1,
                                                                             bias_correction2_sqrt, grad_scale);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// mopa_adamw_flat behind the step record of mopa_grad_stats, as mopa_adam_flat_guarded is mopa_adam_flat behind it.
MOPA_API int mopa_adamw_flat_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, float bias_correction1,
                                     float bias_correction2_sqrt, float grad_scale, const void* rec, void* stream) {
  if (n <= 0 || !rec) return MOPA_ERR_ARG;
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) return MOPA_ERR_ARG;
  if (((uintptr_t)rec & 7) != 0) return MOPA_ERR_ARG;
  k_adamw_flat_guarded<<<stream_grid(n / 4 + 1, 256), 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, exp_avg_sq, n, lr, beta1,
                                                                                     beta2, eps, weight_decay, bias_correction1,
                                                                                     bias_correction2_sqrt, grad_scale,
                                                                                     (const GsStepRec*)rec);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// torch.optim.SGD on the flat buffer.  first != 0: this is the first step that writes momentum_buf (buf = g', no dampening, as
// torch clones the gradient).  momentum_buf may be null when momentum == 0 (it is neither read nor written then).
MOPA_API int mopa_sgd_flat(float* params, const float* grads, float* momentum_buf, int64_t n, float lr, float momentum,
                           float dampening, float weight_decay, int nesterov, int first, float grad_scale, void* stream) {
  if (n <= 0 || !params || !grads) return MOPA_ERR_ARG;
  if (momentum != 0.f && !momentum_buf) return MOPA_ERR_ARG;
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)momentum_buf) & 15) != 0) return MOPA_ERR_ARG;
  k_sgd_flat<<<stream_grid(n / 4 + 1, 256), 256, 0, (hipStream_t)stream>>>(params, grads, momentum != 0.f ? momentum_buf : nullptr, n, lr,
                                                                           momentum, dampening, weight_decay, nesterov, first,
                                                                           grad_scale);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// mopa_sgd_flat behind the step record `rec`.  In place of `first` it takes `buf_valid`, one int32 in DEVICE memory (4-byte
// aligned; may be null when momentum == 0): 0 = momentum_buf has not been written yet, so the step -- if rec says it is applied --
// is the first; a second, one-thread launch behind the update then sets it to 1.  A skipped step leaves it, and everything else,
// alone: the next applied step is still the first.
MOPA_API int mopa_sgd_flat_guarded(float* params, const float* grads, float* momentum_buf, int64_t n, float lr, float momentum,
                                   float dampening, float weight_decay, int nesterov, int* buf_valid, float grad_scale,
                                   const void* rec, void* stream) {
  if (n <= 0 || !rec || !params || !grads) return MOPA_ERR_ARG;
  if (momentum != 0.f && (!momentum_buf || !buf_valid)) return MOPA_ERR_ARG;
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)momentum_buf) & 15) != 0) return MOPA_ERR_ARG;
  if (((uintptr_t)rec & 7) != 0 || ((uintptr_t)buf_valid & 3) != 0) return MOPA_ERR_ARG;
  const bool use_mom = momentum != 0.f;
  k_sgd_flat_guarded<<<stream_grid(n / 4 + 1, 256), 256, 0, (hipStream_t)stream>>>(params, grads, use_mom ? momentum_buf : nullptr, n, lr,
                                                                                   momentum, dampening, weight_decay, nesterov,
                                                                                   use_mom ? buf_valid : nullptr, grad_scale,
                                                                                   (const GsStepRec*)rec);
  MOPA_CHECK_LAUNCH();
  if (use_mom) {
    k_sgd_mark_valid<<<1, 64, 0, (hipStream_t)stream>>>(buf_valid, (const GsStepRec*)rec);
    MOPA_CHECK_LAUNCH();
  }
  return MOPA_OK;
}
