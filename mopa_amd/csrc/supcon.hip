// Supervised contrastive loss (SupConLoss of mopa/models/losses.py:123-184, TRAIN.PC_MM.lambda_ctr_src / lambda_ctr_trg) and the row
// normalisation it is fed with (l2_norm of mopa/common/utils/loss.py:230-238) on the device.  No (Na, Nq) array exists anywhere:
// every S = A Q^T / T tile lives in the accumulators of v_mfma_f32_32x32x2_f32 and is consumed there.
//
//   forward   k_supcon_fwd       grid (anchor tiles of SC_TA rows, pool chunks): the anchor tile and one pool tile of SC_TQ rows at a
//                                time in LDS (zero padded there to an even width), four waves, one 32 x 32 tile of S each; per
//                                (row, lane) a running maximum m with rescaling, E = sum over negatives of exp(S - m), the sum of S
//                                over positives and the count of positives; per chunk the 32 lanes of a row are merged by an xor
//                                butterfly, then the two column halves in index order
//             k_supcon_finalize  one workgroup: per row the chunk partials merged in chunk order (float64), D = E + eps |N|,
//                                mlpp = sum_P S / n - m - log D, validity, the rows summed in a fixed order in float64; writes
//                                loss64, the float32 loss, the status word and the state of the backward
//   backward  k_supcon_bwd<side> grid (tiles of the rows that get the gradient, splits of the other side's walk): S tiles recomputed
//                                by the same instruction sequence (the same bits), W = [P] / n - [N] exp(S - m) / D from the saved
//                                row state, W through LDS into a second MFMA product W X; every sixteen tiles the accumulator is
//                                added to a second one (a float32 chain never runs over more than 1024 terms)
//             k_supcon_sum       only when the walk was split (few owned tiles): the splits' slabs summed in index order, in float64
//   l2 norm   k_l2norm_fwd/bwd   one wavefront per row: squares summed in float64 (lane l holds columns l and l + 64, then an xor
//                                butterfly 32, 16, ..., 1), norm rounded to float32, y = x / (norm > 1e-8f ? norm : 1e-8f)
//
// Chunking is a function of (Na, Nq) alone (sc_plan below), never of the device: with ta = ceil(Na / 64) and tq = ceil(Nq / 64) the
// forward uses ceil(tq / ceil(tq / min(64, tq, max(1, 1024 / ta)))) pool chunks; the backward splits its walk the same way with a bound
// of 32.  No floating-point atomics; the same inputs give the same bits on every run and every device of the family.
//
// workspace (mopa_supcon_workspace_bytes): the larger of the forward's partials, 28 bytes per (chunk, anchor), and a backward's
// slabs, 4 F bytes per (split, owned row); chunks * ta and splits * tiles are at most about 1024 + 64, so beyond 20 * Na (forward, one
// chunk) this is a constant of a few MB, far below 64 * (Na + Nq) * F * 4.
// state (mopa_supcon_state_bytes): doubles [0] loss64, [1] scale = 1 / divisor (NaN in the default mode when a row is invalid, 0 when no
// row is valid under skip_invalid); then floats m[Na], 1 / D[Na], 1 / n[Na] (the last two 0 for a row left out).
// status (int32): bit 0 an anchor has no positive, bit 1 an anchor has no negative, bit 2 a non-finite S was met.
#include "common.h"
#include <float.h>
#include <math.h>

#define SC_MAX_F 128
#define SC_TA 64                 // anchor rows per tile
#define SC_TQ 64                 // pool rows per tile
#define SC_THREADS 256
#define SC_TARGET_BLOCKS 1024    // chunks / splits are added until the grid has about this many workgroups
#define SC_MAX_CHUNKS 64
#define SC_MAX_SPLIT 32
#define SC_FLUSH 16              // tiles between two flushes of the backward's accumulator
#define SC_EPS 1e-5f             // the reference's float32 path adds float32(1e-5) per negative pair
#define SC_FIN_THREADS 1024
#define SC_MAX_ROWS 2147483584LL // 2^31 - 64: tile and count arithmetic in int
#define L2_EPS 1e-8f

typedef float sc_f16v __attribute__((ext_vector_type(16)));

struct ScPlan {
  int tiles_per_part;   // tiles of the walked side per chunk / split
  int parts;
};
// `own` tiles get one workgroup per part; the walked side's `walk` tiles are dealt out in `parts` contiguous runs
static inline ScPlan sc_plan(int64_t own_tiles, int64_t walk_tiles, int max_parts) {
  int64_t want = SC_TARGET_BLOCKS / own_tiles;
  if (want < 1) want = 1;
  if (want > max_parts) want = max_parts;
  if (want > walk_tiles) want = walk_tiles;
  ScPlan p;
  p.tiles_per_part = (int)cdiv64(walk_tiles, want);
  p.parts = (int)cdiv64(walk_tiles, p.tiles_per_part);
  return p;
}
static inline bool sc_shape_ok(int64_t Na, int64_t Nq, int F) {
  return F >= 1 && F <= SC_MAX_F && Na >= 1 && Nq >= 1 && Na <= SC_MAX_ROWS && Nq <= SC_MAX_ROWS;
}

struct ScParts {   // the forward's per (chunk, anchor) partials, [chunk][Na] each
  double* sp;      // sum of S over positives
  float* m;
  float* E;
  int* np;         // positives
  int* nn;         // negatives
  int* bad;        // a non-finite S
};
static inline size_t sc_parts_bytes(int64_t Na, int chunks) { return (size_t)chunks * (size_t)Na * 28; }
static inline ScParts sc_parts(void* ws, int64_t Na, int chunks) {
  const size_t n = (size_t)chunks * (size_t)Na;
  ScParts p;
  p.sp = (double*)ws;
  p.m = (float*)(p.sp + n);
  p.E = p.m + n;
  p.np = (int*)(p.E + n);
  p.nn = p.np + n;
  p.bad = p.nn + n;
  return p;
}

__device__ __forceinline__ int sc_ld(int F) { return ((F + 1) & ~1) | 1; }   // even padded width + 1: odd row stride in LDS

// 64 rows of x from row0 into dst[64][LD]: columns >= F and rows >= N are zeros
__device__ __forceinline__ void sc_stage(float* __restrict__ dst, const float* __restrict__ x, long long row0, long long N, int F, int LD) {
  const int Fp = (F + 1) & ~1;
  for (int e = threadIdx.x; e < 64 * Fp; e += SC_THREADS) {
    const int r = e / Fp, c = e - r * Fp;
    const long long row = row0 + r;
    dst[r * LD + c] = (c < F && row < N) ? x[row * F + c] : 0.f;
  }
}
__device__ __forceinline__ void sc_stage_labels(long long* __restrict__ dst, const long long* __restrict__ lab, long long row0, long long N) {
  if (threadIdx.x < 64) dst[threadIdx.x] = row0 + threadIdx.x < N ? lab[row0 + threadIdx.x] : 0;
}

// the wave's 32 x 32 tile of R C^T: rows rt * 32 .. of R, rows ct * 32 .. of C; per element the fmaf chain over k = 0, 1, ..., Fp - 1
// from 0 (the padding adds exact zeros).  Result: column = lane & 31, row = sc_row(reg, lane).
__device__ __forceinline__ sc_f16v sc_s_tile(const float* __restrict__ R, const float* __restrict__ C, int LD, int Fp, int rt, int ct, int lane) {
  sc_f16v acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* a = R + (rt * 32 + (lane & 31)) * LD + (lane >> 5);
  const float* b = C + (ct * 32 + (lane & 31)) * LD + (lane >> 5);
  for (int k = 0; k < Fp; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b[k], acc, 0, 0, 0);
  return acc;
}
__device__ __forceinline__ int sc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// (m, E) <- the merge of two running (maximum, scaled sum) pairs; an empty pair is (-inf, 0)
__device__ __forceinline__ void sc_merge(float& m, float& E, float m2, float E2) {
  const float M = fmaxf(m, m2);
  const float s1 = m == M ? 1.f : expf(m - M), s2 = m2 == M ? 1.f : expf(m2 - M);
  E = __fadd_rn(__fmul_rn(E, s1), __fmul_rn(E2, s2));
  m = M;
}

// -------------------------------------------------------------------------------------------------------------------------- forward
static size_t sc_fwd_lds(int F) {
  const int LD = ((F + 1) & ~1) | 1;
  return (size_t)2 * 64 * LD * 4 + 2 * 64 * 8 + 128 * 8 + 5 * 128 * 4;
}

__global__ __launch_bounds__(SC_THREADS) void k_supcon_fwd(const long long* __restrict__ la, const float* __restrict__ A, long long Na,
                                                            const float* __restrict__ Q, const long long* __restrict__ lc, long long Nq, int F,
                                                            float T, int tiles_per_chunk, ScParts out) {
  extern __shared__ __align__(16) unsigned char sc_lds[];
  const int LD = sc_ld(F), Fp = LD - 1;
  float* As = reinterpret_cast<float*>(sc_lds);
  float* Qs = As + 64 * LD;
  long long* las = reinterpret_cast<long long*>(Qs + 64 * LD);
  long long* lcs = las + 64;
  double* x_sp = reinterpret_cast<double*>(lcs + 64);   // [column half][row] of the cross-wave merge
  float* x_m = reinterpret_cast<float*>(x_sp + 128);
  float* x_E = x_m + 128;
  int* x_np = reinterpret_cast<int*>(x_E + 128);
  int* x_cnt = x_np + 128;
  int* x_bad = x_cnt + 128;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, rt = w >> 1, ct = w & 1;
  const long long a0 = (long long)blockIdx.x * SC_TA;
  const long long tq = (Nq + SC_TQ - 1) / SC_TQ;
  const long long t0 = (long long)blockIdx.y * tiles_per_chunk;
  const long long t1 = t0 + tiles_per_chunk < tq ? t0 + tiles_per_chunk : tq;

  sc_stage(As, A, a0, Na, F, LD);
  sc_stage_labels(las, la, a0, Na);
  __syncthreads();
  long long lar[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) lar[r] = las[rt * 32 + sc_row(r, lane)];

  float m[16], E[16], sp[16];
  int np[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { m[r] = -INFINITY; E[r] = 0.f; sp[r] = 0.f; np[r] = 0; }
  int cnt = 0, bad = 0;

  for (long long t = t0; t < t1; ++t) {
    const long long q0 = t * SC_TQ;
    __syncthreads();
    sc_stage(Qs, Q, q0, Nq, F, LD);
    sc_stage_labels(lcs, lc, q0, Nq);
    __syncthreads();
    const sc_f16v acc = sc_s_tile(As, Qs, LD, Fp, rt, ct, lane);
    const int cj = ct * 32 + (lane & 31);
    if (q0 + cj < Nq) {
      const long long lcj = lcs[cj];
      ++cnt;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float s = acc[r] / T;
        bad |= !(fabsf(s) <= FLT_MAX);
        const bool pos = lar[r] == lcj;
        const float d = s - m[r];
        const float e = expf(-fabsf(d));
        if (d > 0.f) {
          E[r] = __fmul_rn(E[r], e) + (pos ? 0.f : 1.f);
          m[r] = s;
        } else {
          E[r] += pos ? 0.f : e;
        }
        if (pos) { sp[r] += s; ++np[r]; }
      }
    }
  }

  // the 32 lanes of a row half: xor butterfly 1, 2, 4, 8, 16 (lane 0 / 32 of each half keeps the result)
  double spd[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) spd[r] = (double)sp[r];
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float m2 = __shfl_xor(m[r], o, 64), E2 = __shfl_xor(E[r], o, 64);
      sc_merge(m[r], E[r], m2, E2);
      spd[r] += __shfl_xor(spd[r], o, 64);
      np[r] += __shfl_xor(np[r], o, 64);
    }
    cnt += __shfl_xor(cnt, o, 64);
    bad |= __shfl_xor(bad, o, 64);
  }
  if ((lane & 31) == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int at = ct * 64 + rt * 32 + sc_row(r, lane);
      x_sp[at] = spd[r]; x_m[at] = m[r]; x_E[at] = E[r]; x_np[at] = np[r]; x_cnt[at] = cnt; x_bad[at] = bad;
    }
  }
  __syncthreads();
  if (tid < 64 && a0 + tid < Na) {
    float mm = x_m[tid], EE = x_E[tid];
    sc_merge(mm, EE, x_m[64 + tid], x_E[64 + tid]);
    const int npp = x_np[tid] + x_np[64 + tid], cc = x_cnt[tid] + x_cnt[64 + tid];
    const size_t at = (size_t)blockIdx.y * (size_t)Na + (size_t)(a0 + tid);
    out.sp[at] = x_sp[tid] + x_sp[64 + tid];
    out.m[at] = mm;
    out.E[at] = EE;
    out.np[at] = npp;
    out.nn[at] = cc - npp;
    out.bad[at] = x_bad[tid] | x_bad[64 + tid];
  }
}

// One workgroup.  Thread t takes rows t, t + 1024, ...; the threads' sums are added by an xor butterfly per wave, the waves in index order.
__global__ __launch_bounds__(SC_FIN_THREADS) void k_supcon_finalize(ScParts in, long long Na, int chunks, int skip_invalid,
                                                                     float* __restrict__ loss, double* __restrict__ state,
                                                                     int* __restrict__ status) {
  __shared__ double red[SC_FIN_THREADS / 64];
  __shared__ long long redn[SC_FIN_THREADS / 64];
  const int tid = threadIdx.x;
  float* rm = reinterpret_cast<float*>(state + 2);
  float* rD = rm + Na;
  float* rn = rD + Na;
  double sum = 0.0;
  long long nvalid = 0;
  int bits = 0;
  for (long long row = tid; row < Na; row += SC_FIN_THREADS) {
    double M = -INFINITY, E = 0.0, S = 0.0;
    long long nP = 0, nN = 0;
    int bad = 0;
    for (int c = 0; c < chunks; ++c) {
      const size_t at = (size_t)c * (size_t)Na + (size_t)row;
      const double m2 = (double)in.m[at], E2 = (double)in.E[at];
      const double Mx = fmax(M, m2);
      const double s1 = M == Mx ? 1.0 : exp(M - Mx), s2 = m2 == Mx ? 1.0 : exp(m2 - Mx);
      E = E * s1 + E2 * s2;
      M = Mx;
      S += in.sp[at];
      nP += in.np[at];
      nN += in.nn[at];
      bad |= in.bad[at];
    }
    const double D = E + (double)SC_EPS * (double)nN;
    const bool valid = nP > 0 && nN > 0;
    bits |= (nP == 0 ? 1 : 0) | (nN == 0 ? 2 : 0) | (bad ? 4 : 0);
    if (valid) {
      sum += S / (double)nP - M - log(D);
      ++nvalid;
    }
    const bool keep = valid || !skip_invalid;
    rm[row] = (float)M;
    rD[row] = keep ? (float)(1.0 / D) : 0.f;
    rn[row] = keep ? (float)(1.0 / (double)nP) : 0.f;
  }
  sum = wave_sum_d(sum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nvalid += __shfl_xor(nvalid, o, 64);
  if ((tid & 63) == 0) { red[tid >> 6] = sum; redn[tid >> 6] = nvalid; }
  // (__syncthreads_or reduces a predicate, not a word: one call per bit; the first also publishes red / redn)
  bits = (__syncthreads_or(bits & 1) ? 1 : 0) | (__syncthreads_or(bits & 2) ? 2 : 0) | (__syncthreads_or(bits & 4) ? 4 : 0);
  if (tid == 0) {
    double s = 0.0;
    long long n = 0;
    for (int k = 0; k < SC_FIN_THREADS / 64; ++k) { s += red[k]; n += redn[k]; }
    double l64, scale;
    if (skip_invalid) {
      l64 = n > 0 ? -s / (double)n : 0.0;
      scale = n > 0 ? 1.0 / (double)n : 0.0;
    } else if (n < Na) {
      l64 = (double)NAN;
      scale = (double)NAN;
    } else {
      l64 = -s / (double)Na;
      scale = 1.0 / (double)Na;
    }
    state[0] = l64;
    state[1] = scale;
    *loss = (float)l64;
    *status = bits;
  }
}

// ------------------------------------------------------------------------------------------------------------------------- backward
static size_t sc_bwd_lds(int F) {
  const int LD = ((F + 1) & ~1) | 1;
  return (size_t)2 * 64 * LD * 4 + 64 * 65 * 4 + 2 * 64 * 8 + 3 * 64 * 4;
}

// SIDE 0: the workgroup owns 64 anchor rows and walks pool tiles; SIDE 1: it owns 64 pool rows and walks anchor tiles.
// out: dx (scaled by c = -g * scale / T) when the walk is not split, else this split's slab (unscaled).
template <int SIDE>
__global__ __launch_bounds__(SC_THREADS) void k_supcon_bwd(const float* __restrict__ own, const long long* __restrict__ lown, long long Nown,
                                                            const float* __restrict__ walk, const long long* __restrict__ lwalk,
                                                            long long Nwalk, int F, float T, int tiles_per_split, int splits,
                                                            const double* __restrict__ state, long long Na, const float* __restrict__ g,
                                                            float* __restrict__ dx, float* __restrict__ slab) {
  extern __shared__ __align__(16) unsigned char sc_lds[];
  const int LD = sc_ld(F), Fp = LD - 1;
  float* Os = reinterpret_cast<float*>(sc_lds);
  float* Ws = Os + 64 * LD;
  float* Wt = Ws + 64 * LD;                                   // [owned row][walked row], stride 65
  long long* los = reinterpret_cast<long long*>(Wt + 64 * 65);
  long long* lws = los + 64;
  float* sm = reinterpret_cast<float*>(lws + 64);             // the anchors' m, 1 / D, 1 / n: of the owned tile (SIDE 0) or the walked one
  float* sD = sm + 64;
  float* sn = sD + 64;
  const float* rm = reinterpret_cast<const float*>(state + 2);
  const float* rD = rm + Na;
  const float* rn = rD + Na;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, rt = w >> 1, ct = w & 1;
  const long long o0 = (long long)blockIdx.x * 64;
  const long long tw = (Nwalk + 63) / 64;
  const long long t0 = (long long)blockIdx.y * tiles_per_split;
  const long long t1 = t0 + tiles_per_split < tw ? t0 + tiles_per_split : tw;

  sc_stage(Os, own, o0, Nown, F, LD);
  sc_stage_labels(los, lown, o0, Nown);
  if (SIDE == 0 && tid < 64) {
    const bool in = o0 + tid < Na;
    sm[tid] = in ? rm[o0 + tid] : 0.f;
    sD[tid] = in ? rD[o0 + tid] : 0.f;
    sn[tid] = in ? rn[o0 + tid] : 0.f;
  }
  __syncthreads();
  long long lor[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) lor[r] = los[rt * 32 + sc_row(r, lane)];

  // second product: wave w owns rows (w & 1) * 32 .. of the tile and the 32-column blocks (w >> 1) and (w >> 1) + 2 of F
  const int rh = w & 1, nfb = (F + 31) >> 5;
  const int fb0 = w >> 1, fb1 = (w >> 1) + 2;
  const int f0 = min(fb0 * 32 + (lane & 31), Fp - 1), f1 = min(fb1 * 32 + (lane & 31), Fp - 1);   // clamped: such columns are not stored
  sc_f16v acc0, acc1, tot0, tot1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; tot0[r] = 0.f; tot1[r] = 0.f; }

  int since = 0;
  for (long long t = t0; t < t1; ++t) {
    const long long q0 = t * 64;
    __syncthreads();
    sc_stage(Ws, walk, q0, Nwalk, F, LD);
    sc_stage_labels(lws, lwalk, q0, Nwalk);
    if (SIDE == 1 && tid < 64) {
      const bool in = q0 + tid < Na;
      sm[tid] = in ? rm[q0 + tid] : 0.f;
      sD[tid] = in ? rD[q0 + tid] : 0.f;
      sn[tid] = in ? rn[q0 + tid] : 0.f;
    }
    __syncthreads();
    const sc_f16v acc = sc_s_tile(Os, Ws, LD, Fp, rt, ct, lane);
    const int cj = ct * 32 + (lane & 31);
    const bool cvalid = q0 + cj < Nwalk;
    const long long lwj = lws[cj];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ri = rt * 32 + sc_row(r, lane);
      const int ai = SIDE == 0 ? ri : cj;                     // the anchor of the pair, as an index of sm / sD / sn
      const float s = acc[r] / T;
      const float wv = lor[r] == lwj ? sn[ai] : -expf(s - sm[ai]) * sD[ai];
      Wt[ri * 65 + cj] = cvalid ? wv : 0.f;
    }
    __syncthreads();
    if (fb0 < nfb) {
      const float* a = Wt + (rh * 32 + (lane & 31)) * 65 + (lane >> 5);
      const float* b0 = Ws + (lane >> 5) * LD + f0;
      const float* b1 = Ws + (lane >> 5) * LD + f1;
      if (fb1 < nfb) {
        for (int k = 0; k < 64; k += 2) {
          const float av = a[k];
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0[k * LD], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1[k * LD], acc1, 0, 0, 0);
        }
      } else {
        for (int k = 0; k < 64; k += 2) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b0[k * LD], acc0, 0, 0, 0);
      }
    }
    if (++since == SC_FLUSH) {
      since = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) { tot0[r] += acc0[r]; tot1[r] += acc1[r]; acc0[r] = 0.f; acc1[r] = 0.f; }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) { tot0[r] += acc0[r]; tot1[r] += acc1[r]; }

  const double c = -(double)*g * state[1] / (double)T;
  float* dst = splits > 1 ? slab + (size_t)blockIdx.y * (size_t)Nown * F : dx;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long row = o0 + rh * 32 + sc_row(r, lane);
    if (row >= Nown) continue;
    const int fa = fb0 * 32 + (lane & 31), fb = fb1 * 32 + (lane & 31);
    if (fa < F) dst[row * F + fa] = splits > 1 ? tot0[r] : (float)((double)tot0[r] * c);
    if (fb < F) dst[row * F + fb] = splits > 1 ? tot1[r] : (float)((double)tot1[r] * c);
  }
}

__global__ __launch_bounds__(SC_THREADS) void k_supcon_sum(const float* __restrict__ slab, long long n, int splits, const double* __restrict__ state,
                                                            float T, const float* __restrict__ g, float* __restrict__ dx) {
  const double c = -(double)*g * state[1] / (double)T;
  for (long long e = (long long)blockIdx.x * SC_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * SC_THREADS) {
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += (double)slab[(size_t)k * (size_t)n + (size_t)e];
    dx[e] = (float)(s * c);
  }
}

// -------------------------------------------------------------------------------------------------------------------------- l2 norm
__global__ __launch_bounds__(SC_THREADS) void k_l2norm_fwd(const float* __restrict__ x, long long N, int F, float* __restrict__ y,
                                                            float* __restrict__ norm) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (SC_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= N) return;
  const float x0 = lane < F ? x[row * F + lane] : 0.f, x1 = lane + 64 < F ? x[row * F + lane + 64] : 0.f;
  const double ss = wave_sum_d(fma((double)x1, (double)x1, (double)x0 * (double)x0));
  const float nrm = (float)sqrt(ss);
  const float den = nrm > L2_EPS ? nrm : L2_EPS;
  if (lane < F) y[row * F + lane] = x0 / den;
  if (lane + 64 < F) y[row * F + lane + 64] = x1 / den;
  if (lane == 0) norm[row] = nrm;
}

// dx = (g - y (y . g)) / norm where norm > eps, g / eps where not (autograd through the reference's torch.where); y . g in float64 in the
// order of the forward's sum
__global__ __launch_bounds__(SC_THREADS) void k_l2norm_bwd(const float* __restrict__ y, const float* __restrict__ norm, const float* __restrict__ g,
                                                            long long N, int F, float* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (SC_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= N) return;
  const bool h0 = lane < F, h1 = lane + 64 < F;
  const float y0 = h0 ? y[row * F + lane] : 0.f, y1 = h1 ? y[row * F + lane + 64] : 0.f;
  const float g0 = h0 ? g[row * F + lane] : 0.f, g1 = h1 ? g[row * F + lane + 64] : 0.f;
  const double dot = wave_sum_d(fma((double)y1, (double)g1, (double)y0 * (double)g0));
  const float nrm = norm[row];
  if (nrm > L2_EPS) {
    if (h0) dx[row * F + lane] = (float)(((double)g0 - (double)y0 * dot) / (double)nrm);
    if (h1) dx[row * F + lane + 64] = (float)(((double)g1 - (double)y1 * dot) / (double)nrm);
  } else {
    if (h0) dx[row * F + lane] = g0 / L2_EPS;
    if (h1) dx[row * F + lane + 64] = g1 / L2_EPS;
  }
}

// --------------------------------------------------------------------------------------------------------------------- entry points
static int sc_lds_attr(const void* kern, size_t bytes, int slot) {
  static std::atomic<bool> attr[64][3];   // per device: the attribute belongs to the device's code object
  const int dev = mopa_device_index();
  if (dev < 0) return MOPA_ERR_LAUNCH;
  if (!attr[dev][slot].load(std::memory_order_acquire)) {
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return MOPA_ERR_LAUNCH;
    attr[dev][slot].store(true, std::memory_order_release);
  }
  return MOPA_OK;
}

static inline size_t sc_slab_bytes(int64_t Nown, int64_t Nwalk, int F) {
  const ScPlan p = sc_plan(cdiv64(Nown, 64), cdiv64(Nwalk, 64), SC_MAX_SPLIT);
  return p.parts > 1 ? (size_t)p.parts * (size_t)Nown * F * sizeof(float) : 0;
}

// Bytes of `ws` for mopa_supcon_fwd and mopa_supcon_bwd at this shape; 0 for a refused shape.
MOPA_API size_t mopa_supcon_workspace_bytes(int64_t Na, int64_t Nq, int F) {
  if (!sc_shape_ok(Na, Nq, F)) return 0;
  size_t b = sc_parts_bytes(Na, sc_plan(cdiv64(Na, SC_TA), cdiv64(Nq, SC_TQ), SC_MAX_CHUNKS).parts);
  const size_t s0 = sc_slab_bytes(Na, Nq, F), s1 = sc_slab_bytes(Nq, Na, F);
  if (s0 > b) b = s0;
  if (s1 > b) b = s1;
  return align_up(b, 256);
}

MOPA_API size_t mopa_supcon_state_bytes(int64_t Na) {
  if (Na < 1 || Na > SC_MAX_ROWS) return 0;
  return 16 + (size_t)Na * 12;
}

// The forward's number of pool chunks (a function of the two row counts alone); 0 for a refused shape.
MOPA_API int mopa_supcon_pool_chunks(int64_t Na, int64_t Nq) {
  if (!sc_shape_ok(Na, Nq, 1)) return 0;
  return sc_plan(cdiv64(Na, SC_TA), cdiv64(Nq, SC_TQ), SC_MAX_CHUNKS).parts;
}

// Rows per tile of the kernels: side 0 = anchors (SC_TA), side 1 = pool (SC_TQ); 0 for another side.  The tile-edge tests read it.
MOPA_API int mopa_supcon_tile_rows(int side) { return side == 0 ? SC_TA : side == 1 ? SC_TQ : 0; }

// labels_anchor (Na) int64, anchor (Na, F), pool (Nq, F) float32 row-major, labels_pool (Nq) int64 (anchor and pool may be the same
// memory); T > 0; skip_invalid: 0 = an anchor without a positive or without a negative makes the loss NaN, 1 = such anchors are left
// out.  loss: one float32; state: mopa_supcon_state_bytes(Na), 8-byte aligned, read by mopa_supcon_bwd; status: one int32, rewritten.
MOPA_API int mopa_supcon_fwd(const int64_t* labels_anchor, const float* anchor, int64_t Na, const float* pool, const int64_t* labels_pool,
                             int64_t Nq, int F, float T, int skip_invalid, float* loss, void* state, int* status, void* ws, size_t ws_bytes,
                             void* stream) {
  if (!sc_shape_ok(Na, Nq, F) || !(T > 0.f) || !(T <= FLT_MAX) || skip_invalid < 0 || skip_invalid > 1) return MOPA_ERR_ARG;
  if (!labels_anchor || !anchor || !pool || !labels_pool || !loss || !state || !status || !ws) return MOPA_ERR_ARG;
  if (((uintptr_t)state & 7) || ((uintptr_t)ws & 7)) return MOPA_ERR_ARG;
  const int64_t ta = cdiv64(Na, SC_TA);
  const ScPlan p = sc_plan(ta, cdiv64(Nq, SC_TQ), SC_MAX_CHUNKS);
  if (ws_bytes < sc_parts_bytes(Na, p.parts)) return MOPA_ERR_WORKSPACE;
  const int rc = sc_lds_attr(reinterpret_cast<const void*>(k_supcon_fwd), sc_fwd_lds(SC_MAX_F), 0);
  if (rc != MOPA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const ScParts parts = sc_parts(ws, Na, p.parts);
  k_supcon_fwd<<<dim3((unsigned)ta, (unsigned)p.parts), SC_THREADS, sc_fwd_lds(F), st>>>(
      (const long long*)labels_anchor, anchor, (long long)Na, pool, (const long long*)labels_pool, (long long)Nq, F, T, p.tiles_per_part, parts);
  MOPA_CHECK_LAUNCH();
  k_supcon_finalize<<<1, SC_FIN_THREADS, 0, st>>>(parts, (long long)Na, p.parts, skip_invalid, loss, (double*)state, status);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// dx = g * d loss / d anchor (side 0, (Na, F)) or g * d loss / d pool (side 1, (Nq, F)) of the forward call that wrote `state`, on the
// same inputs and T; g: one float32 on the device.  ws: mopa_supcon_workspace_bytes (its content after the forward is not needed).
MOPA_API int mopa_supcon_bwd(const int64_t* labels_anchor, const float* anchor, int64_t Na, const float* pool, const int64_t* labels_pool,
                             int64_t Nq, int F, float T, int side, const void* state, const float* g, float* dx, void* ws, size_t ws_bytes,
                             void* stream) {
  if (!sc_shape_ok(Na, Nq, F) || !(T > 0.f) || !(T <= FLT_MAX) || side < 0 || side > 1) return MOPA_ERR_ARG;
  if (!labels_anchor || !anchor || !pool || !labels_pool || !state || !g || !dx) return MOPA_ERR_ARG;
  if ((uintptr_t)state & 7) return MOPA_ERR_ARG;
  const int64_t Nown = side == 0 ? Na : Nq, Nwalk = side == 0 ? Nq : Na;
  const int64_t to = cdiv64(Nown, 64);
  const ScPlan p = sc_plan(to, cdiv64(Nwalk, 64), SC_MAX_SPLIT);
  if (p.parts > 1 && (!ws || ((uintptr_t)ws & 3) || ws_bytes < sc_slab_bytes(Nown, Nwalk, F))) return MOPA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)to, (unsigned)p.parts);
  const size_t lds = sc_bwd_lds(F);
  if (side == 0) {
    const int rc = sc_lds_attr(reinterpret_cast<const void*>(k_supcon_bwd<0>), sc_bwd_lds(SC_MAX_F), 1);
    if (rc != MOPA_OK) return rc;
    k_supcon_bwd<0><<<grid, SC_THREADS, lds, st>>>(anchor, (const long long*)labels_anchor, (long long)Na, pool, (const long long*)labels_pool,
                                                   (long long)Nq, F, T, p.tiles_per_part, p.parts, (const double*)state, (long long)Na, g, dx,
                                                   (float*)ws);
  } else {
    const int rc = sc_lds_attr(reinterpret_cast<const void*>(k_supcon_bwd<1>), sc_bwd_lds(SC_MAX_F), 2);
    if (rc != MOPA_OK) return rc;
    k_supcon_bwd<1><<<grid, SC_THREADS, lds, st>>>(pool, (const long long*)labels_pool, (long long)Nq, anchor, (const long long*)labels_anchor,
                                                   (long long)Na, F, T, p.tiles_per_part, p.parts, (const double*)state, (long long)Na, g, dx,
                                                   (float*)ws);
  }
  MOPA_CHECK_LAUNCH();
  if (p.parts > 1) {
    const long long n = (long long)Nown * F;
    k_supcon_sum<<<stream_grid(n, SC_THREADS), SC_THREADS, 0, st>>>((const float*)ws, n, p.parts, (const double*)state, T, g, dx);
    MOPA_CHECK_LAUNCH();
  }
  return MOPA_OK;
}

// y (N, F) = x / max'(|x|_2, 1e-8) per row, norm (N) = |x|_2 rounded to float32 (kept for the backward); 1 <= F <= 128.
MOPA_API int mopa_l2norm_rows_fwd(const float* x, int64_t N, int F, float* y, float* norm, void* stream) {
  if (F < 1 || F > SC_MAX_F || N < 1 || N > SC_MAX_ROWS || !x || !y || !norm) return MOPA_ERR_ARG;
  k_l2norm_fwd<<<(unsigned)cdiv64(N, SC_THREADS / 64), SC_THREADS, 0, (hipStream_t)stream>>>(x, (long long)N, F, y, norm);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

MOPA_API int mopa_l2norm_rows_bwd(const float* y, const float* norm, const float* g, int64_t N, int F, float* dx, void* stream) {
  if (F < 1 || F > SC_MAX_F || N < 1 || N > SC_MAX_ROWS || !y || !norm || !g || !dx) return MOPA_ERR_ARG;
  k_l2norm_bwd<<<(unsigned)cdiv64(N, SC_THREADS / 64), SC_THREADS, 0, (hipStream_t)stream>>>(y, norm, g, (long long)N, F, dx);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
