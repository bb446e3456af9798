// Lovasz-softmax loss (mopa/common/utils/loss.py:107-199) on the device: per (row segment, class) a stable segmented LSD radix sort of
// the errors, integer running counts of the foreground along the sorted order, float64 Jaccard weights.  No host synchronisation, no
// floating-point atomics, a launch count that depends on neither P, C nor the classes present.
//
//   forward   k_lov_count     per segment: valid rows V, rows with a label outside [0, C), rows per class (integer LDS + global atomics);
//                             the logits form also stores the rows' log-sum-exp
//             per pass (LOV_PASSES of LOV_BITS bits; pass 0 forms the keys from the inputs, no key plane is written first)
//               k_lov_hist    per (block, class) the digit histogram of the block's tile (integer LDS atomics) -> tab[class][block][digit]
//               k_lov_rowscan per (digit, class, segment) the exclusive scan of the counts over the segment's blocks, in place, and the
//                             digit's total
//               k_lov_scatter per (block, class): rank of every pair among the pairs of its digit in tile order (wave match, per-wave
//                             counters: no arrival order), position = digit base + block offset + rank
//             k_lov_fgcount   foreground per scan block of the sorted order
//             k_lov_weights   running counts -> I, U, J = 1 - I / U, w_k = J_k - J_{k-1} (float64); per-block float64 sums of e w in a
//                             fixed order; sign w into the coefficient plane
//             k_lov_final     per segment the selected classes, their mean; the mean over segments; loss, status, state
//   backward  k_lov_bwd       dp = g coef / n_selected / S per entry; k_lov_bwd_logits continues to dz = p (dp - sum dp p) in float64 from
//                             float64 coefficients, rounded once
//
// A pair is (key, row | foreground << 31).  key = 0x3F800000 - bits(e) for e = |fg - p| in [0, 1] (ascending key = descending e; the
// stable sort keeps equal keys in ascending row order), 0x3F800001 for an ignored row: 30 bits vary.  A class that is not selected
// costs a read of the segment's counts per block and nothing else.  The arithmetic is stated in DESIGN.md section 4; yardstick
// tests/_lovasz_reference.py.
//
// state (8-byte slots): [0] loss (double), [1 + s] 1 / (n_selected(s) S) or 0 (double), [33 + s] the segment's selected classes (bits).
// status (int32): bit 0 a label outside [0, C) that is not the ignore value.
#include "common.h"
#include "softmax_row.h"

#define LOV_MAX_C 64
#define LOV_MAX_S 32
#ifndef LOV_BITS
#define LOV_BITS 10           // digit width: three passes over the 30 key bits; profiles/r34_lovasz.md has the widths that lost
#endif
#define LOV_KEY_BITS 30
#define LOV_PASSES ((LOV_KEY_BITS + LOV_BITS - 1) / LOV_BITS)
#define LOV_R (1 << LOV_BITS)
#define LOV_THREADS 256
#define LOV_WAVES (LOV_THREADS / 64)
#define LOV_ITEMS 16
#define LOV_SORT_TILE (LOV_THREADS * LOV_ITEMS)   // 4096 pairs per sort block
#define LOV_SCAN_ROUNDS 8
#define LOV_SCAN_TILE (LOV_THREADS * LOV_SCAN_ROUNDS)   // 2048 ranks per scan block
#define LOV_SCAN_WAVES 16     // waves of a k_lov_rowscan block: each takes a sixteenth of the segment's blocks
#define LOV_ONE 0x3F800000u
#define LOV_IGNORED 0x3F800001u
#define LOV_HDR (2 + LOV_MAX_C)   // ints per segment: V, rows with a bad label, rows per class
#define LOV_STATE_SLOTS (1 + 2 * LOV_MAX_S)

struct LovSeg {
  int S;
  int sblk0[LOV_MAX_S + 1];       // first sort block of the segment
  int cblk0[LOV_MAX_S + 1];       // first scan block of the segment
  long long off[LOV_MAX_S + 1];   // first row of the segment
};
struct LovSrc {
  const float* x;             // (P, C) probabilities, or logits with lse
  const float* lse;           // per row, logits form only
  const long long* y;
  long long ignore;
  int has_ignore, C;
};
struct LovSel {
  int mode;                   // 0 'present', 1 'all', 2 a list (mask)
  unsigned long long mask;
};

__device__ __forceinline__ int lov_seg_of(const int* __restrict__ blk0, int S, int blk) {
  int s = 0;
  for (int k = 1; k < S; ++k) s = blk0[k] <= blk ? k : s;   // non-decreasing table: the last segment that starts at or before blk
  return s;
}
__device__ __forceinline__ bool lov_selected(const int* __restrict__ hdr, int s, int c, LovSel sel) {
  const int* h = hdr + s * LOV_HDR;
  if (h[0] == 0) return false;
  if (sel.mode == 1) return true;
  if (sel.mode == 2) return (sel.mask >> c) & 1ull;
  return h[2 + c] > 0;
}
__device__ __forceinline__ bool lov_valid(const LovSrc& src, long long y) { return !(src.has_ignore && y == src.ignore); }

// the pair of row i for class c, from the inputs
__device__ __forceinline__ uint2 lov_first(const LovSrc& src, long long i, int c) {
  const long long y = src.y[i];
  const bool valid = lov_valid(src, y), fg = valid && y == (long long)c;
  float v = src.x[i * src.C + c];
  if (src.lse) v = row_softmax_at(v, src.lse[i]);
  const float e = fabsf((fg ? 1.f : 0.f) - v);
  const unsigned bits = __float_as_uint(e);
  uint2 pr;
  pr.x = valid ? (bits > LOV_ONE ? 0u : LOV_ONE - bits) : LOV_IGNORED;   // p outside [0, 1] (or NaN) sorts first, as e = 1
  pr.y = (unsigned)i | (fg ? 0x80000000u : 0u);
  return pr;
}

// exclusive prefix of v over the block's threads in thread order, and the total.  lds: blockDim.x / 64 ints; two barriers.
__device__ __forceinline__ int lov_block_scan(int v, int* lds, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  int pre = 0, tot = 0;
  for (int k = 0; k < nw; ++k) { const int c = lds[k]; pre += k < w ? c : 0; tot += c; }
  __syncthreads();
  total = tot;
  return pre + inc - v;
}

// ------------------------------------------------------------------------------------------------------------------------ counts
__global__ __launch_bounds__(LOV_THREADS) void k_lov_count(LovSrc src, LovSeg seg, int* __restrict__ hdr, float* __restrict__ lse_out) {
  __shared__ int h[LOV_HDR];
  const int s = blockIdx.y, tid = threadIdx.x, C = src.C;
  if (tid < LOV_HDR) h[tid] = 0;
  __syncthreads();
  const long long n1 = seg.off[s + 1];
  for (long long i = seg.off[s] + (long long)blockIdx.x * LOV_THREADS + tid; i < n1; i += (long long)gridDim.x * LOV_THREADS) {
    if (lse_out) lse_out[i] = row_lse(src.x + i * C, C);
    const long long y = src.y[i];
    if (!lov_valid(src, y)) continue;
    atomicAdd(&h[0], 1);
    if (y >= 0 && y < C) atomicAdd(&h[2 + (int)y], 1); else atomicAdd(&h[1], 1);
  }
  __syncthreads();
  if (tid < LOV_HDR && h[tid]) atomicAdd(&hdr[s * LOV_HDR + tid], h[tid]);
}

// -------------------------------------------------------------------------------------------------------------------- radix sort
template <bool FIRST>
__global__ __launch_bounds__(LOV_THREADS) void k_lov_hist(LovSrc src, LovSeg seg, LovSel sel, const int* __restrict__ hdr,
                                                           const uint2* __restrict__ in, long long P, int shift, int nbmax,
                                                           int* __restrict__ tab) {
  __shared__ int h[LOV_R];
  const int gb = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int s = lov_seg_of(seg.sblk0, seg.S, gb);
  if (!lov_selected(hdr, s, c, sel)) return;
  for (int d = tid; d < LOV_R; d += LOV_THREADS) h[d] = 0;
  __syncthreads();
  const long long n1 = seg.off[s + 1], base = seg.off[s] + (long long)(gb - seg.sblk0[s]) * LOV_SORT_TILE;
#pragma unroll 4
  for (int j = 0; j < LOV_ITEMS; ++j) {
    const long long i = base + j * LOV_THREADS + tid;
    if (i < n1) {
      const unsigned key = FIRST ? lov_first(src, i, c).x : in[(size_t)c * P + i].x;
      atomicAdd(&h[(key >> shift) & (LOV_R - 1)], 1);
    }
  }
  __syncthreads();
  int* out = tab + ((size_t)c * nbmax + gb) * LOV_R;
  for (int d = tid; d < LOV_R; d += LOV_THREADS) out[d] = h[d];
}

// lane = digit, wave w = the w-th sixteenth of the segment's blocks: sums, the waves' sums in index order, then the prefixes in place
__global__ __launch_bounds__(LOV_SCAN_WAVES * 64) void k_lov_rowscan(LovSeg seg, LovSel sel, const int* __restrict__ hdr, int nbmax,
                                                                      int* __restrict__ tab, int* __restrict__ tot) {
  __shared__ int sums[LOV_SCAN_WAVES][64];
  const int c = blockIdx.y, s = blockIdx.z, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (!lov_selected(hdr, s, c, sel)) return;
  const int d = blockIdx.x * 64 + lane;
  const bool live = d < LOV_R;
  const int b0 = seg.sblk0[s], b1 = seg.sblk0[s + 1], q = (b1 - b0 + LOV_SCAN_WAVES - 1) / LOV_SCAN_WAVES;
  const int lo = b0 + w * q < b1 ? b0 + w * q : b1, hi = lo + q < b1 ? lo + q : b1;
  int* col = tab + (size_t)c * nbmax * LOV_R + d;
  int sum = 0;
  if (live)
    for (int b = lo; b < hi; ++b) sum += col[(size_t)b * LOV_R];
  sums[w][lane] = sum;
  __syncthreads();
  int run = 0, total = 0;
  for (int k = 0; k < LOV_SCAN_WAVES; ++k) { const int v = sums[k][lane]; run += k < w ? v : 0; total += v; }
  if (live) {
    for (int b = lo; b < hi; ++b) {
      const int v = col[(size_t)b * LOV_R];
      col[(size_t)b * LOV_R] = run;
      run += v;
    }
    if (w == 0) tot[((size_t)c * seg.S + s) * LOV_R + d] = total;
  }
}

template <bool FIRST>
__global__ __launch_bounds__(LOV_THREADS) void k_lov_scatter(LovSrc src, LovSeg seg, LovSel sel, const int* __restrict__ hdr,
                                                              const uint2* __restrict__ in, uint2* __restrict__ out, long long P,
                                                              int shift, int nbmax, const int* __restrict__ tab,
                                                              const int* __restrict__ tot) {
  __shared__ int cnt[LOV_WAVES][LOV_R];    // pairs of the digit in the wave's span so far; then the waves' exclusive prefixes
  __shared__ int dbase[LOV_R];             // first position of the block's pairs of the digit within the segment
  __shared__ int red[LOV_WAVES];
  const int gb = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int s = lov_seg_of(seg.sblk0, seg.S, gb);
  if (!lov_selected(hdr, s, c, sel)) return;
  const long long n0 = seg.off[s], n1 = seg.off[s + 1];
  const long long base = n0 + (long long)(gb - seg.sblk0[s]) * LOV_SORT_TILE + (long long)w * (64 * LOV_ITEMS) + lane;
  for (int d = tid; d < LOV_WAVES * LOV_R; d += LOV_THREADS) (&cnt[0][0])[d] = 0;
  uint2 pr[LOV_ITEMS];
#pragma unroll
  for (int r = 0; r < LOV_ITEMS; ++r) {
    const long long i = base + r * 64;
    pr[r] = make_uint2(0u, 0u);
    if (i < n1) pr[r] = FIRST ? lov_first(src, i, c) : in[(size_t)c * P + i];
  }
  __syncthreads();
  // a wave owns 16 x 64 consecutive pairs and walks them 64 at a time: the rank of a pair among the equal digits of its wave.  Per
  // round the lanes of one digit find each other by ballots; their lowest lane alone reads and advances the wave's counter (no
  // atomics: the counters are the wave's own, and its LDS operations issue in program order) and hands the old value to the others
  volatile int* mine = cnt[w];
  int rank[LOV_ITEMS];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < LOV_ITEMS; ++r) {
    const bool valid = base + r * 64 < n1;
    const int d = (pr[r].x >> shift) & (LOV_R - 1);
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < LOV_BITS; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long bal = __ballot(valid && bit);
      m &= bit ? bal : ~bal;
    }
    const int leader = valid ? __ffsll((long long)m) - 1 : lane;
    int old = 0;
    if (valid && lane == leader) {
      old = mine[d];
      mine[d] = old + __popcll(m);
    }
    old = __shfl(old, leader, 64);
    rank[r] = old + __popcll(m & below);
  }
  __syncthreads();
  // digit bases: exclusive scan over the digits of the segment's totals, plus the block's offset within the digit
  {
    constexpr int PER = LOV_R >= LOV_THREADS ? LOV_R / LOV_THREADS : 1;
    const int* t = tot + ((size_t)c * seg.S + s) * LOV_R;
    int v[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int d = tid * PER + k;
      v[k] = d < LOV_R ? t[d] : 0;
      sum += v[k];
    }
    int total;
    int run = lov_block_scan(sum, red, total);
    const int* mine_tab = tab + ((size_t)c * nbmax + gb) * LOV_R;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int d = tid * PER + k;
      if (d < LOV_R) dbase[d] = run + mine_tab[d];
      run += v[k];
    }
    for (int d = tid; d < LOV_R; d += LOV_THREADS) {
      int acc = 0;
#pragma unroll
      for (int k = 0; k < LOV_WAVES; ++k) { const int a = cnt[k][d]; cnt[k][d] = acc; acc += a; }
    }
  }
  __syncthreads();
  const long long n = n1 - n0;
  uint2* dst = out + (size_t)c * P + n0;
#pragma unroll
  for (int r = 0; r < LOV_ITEMS; ++r) {
    if (base + r * 64 < n1) {
      const int d = (pr[r].x >> shift) & (LOV_R - 1);
      const long long pos = (long long)dbase[d] + cnt[w][d] + rank[r];
      if (pos >= 0 && pos < n) dst[pos] = pr[r];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- scan and weights
__global__ __launch_bounds__(LOV_THREADS) void k_lov_fgcount(LovSeg seg, LovSel sel, const int* __restrict__ hdr,
                                                              const uint2* __restrict__ sorted, long long P, int ncmax,
                                                              int* __restrict__ fgc) {
  __shared__ int red[LOV_WAVES];
  const int gb = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int s = lov_seg_of(seg.cblk0, seg.S, gb);
  if (!lov_selected(hdr, s, c, sel)) return;
  const long long V = hdr[s * LOV_HDR], k0 = (long long)(gb - seg.cblk0[s]) * LOV_SCAN_TILE;
  const uint2* src = sorted + (size_t)c * P + seg.off[s];
  int n = 0;
#pragma unroll
  for (int j = 0; j < LOV_SCAN_ROUNDS; ++j) {
    const long long k = k0 + j * LOV_THREADS + tid;
    if (k < V) n += (int)(src[k].y >> 31);
  }
  int total;
  lov_block_scan(n, red, total);
  if (tid == 0) fgc[(size_t)c * ncmax + gb] = total;
}

__global__ __launch_bounds__(LOV_THREADS) void k_lov_weights(LovSeg seg, LovSel sel, const int* __restrict__ hdr,
                                                              const uint2* __restrict__ sorted, long long P, int C, int ncmax,
                                                              const int* __restrict__ fgc, double* __restrict__ part,
                                                              float* __restrict__ coef32, double* __restrict__ coef64) {
  __shared__ int red[LOV_WAVES];
  __shared__ double redd[LOV_WAVES];
  const int gb = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int s = lov_seg_of(seg.cblk0, seg.S, gb);
  if (!lov_selected(hdr, s, c, sel)) return;
  const long long n = seg.off[s + 1] - seg.off[s], V = hdr[s * LOV_HDR], G = hdr[s * LOV_HDR + 2 + c];
  const long long k0 = (long long)(gb - seg.cblk0[s]) * LOV_SCAN_TILE;
  const uint2* src = sorted + (size_t)c * P + seg.off[s];
  // foreground in the scan blocks before this one (integers: any order)
  int before = 0;
  for (int b = seg.cblk0[s] + tid; b < gb; b += LOV_THREADS) before += fgc[(size_t)c * ncmax + b];
  int total;
  lov_block_scan(before, red, total);
  long long running = total;
  double acc = 0.0;
  for (int j = 0; j < LOV_SCAN_ROUNDS; ++j) {
    const long long k = k0 + j * LOV_THREADS + tid;
    uint2 pr = make_uint2(0u, 0u);
    if (k < n) pr = src[k];
    const int fg = k < V ? (int)(pr.y >> 31) : 0;
    int round_total;
    const int ex = lov_block_scan(fg, red, round_total);
    if (k < n && (long long)(pr.y & 0x7FFFFFFFu) < P) {
      const size_t at = (size_t)(pr.y & 0x7FFFFFFFu) * C + c;
      double sw = 0.0;
      if (k < V) {
        const long long cum = running + ex + fg, cum1 = cum - fg;   // foreground among ranks 0..k, and among 0..k-1
        const double J = 1.0 - (double)(G - cum) / (double)(G + (k + 1 - cum));
        const double w = k == 0 ? J : J - (1.0 - (double)(G - cum1) / (double)(G + (k - cum1)));
        const float e = __uint_as_float(LOV_ONE - pr.x);
        acc += (double)e * w;
        sw = e == 0.f ? 0.0 : (fg ? -w : w);   // sign(p - fg) w
      }
      if (coef64) coef64[at] = sw; else coef32[at] = (float)sw;
    }
    running += round_total;
  }
  // fixed order: the thread's rounds, the wave's butterfly, the waves in index order
  acc = wave_sum_d(acc);
  if ((tid & 63) == 0) redd[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int k = 0; k < LOV_WAVES; ++k) t += redd[k];
    part[(size_t)c * ncmax + gb] = t;
  }
}

__global__ __launch_bounds__(64) void k_lov_final(LovSeg seg, LovSel sel, const int* __restrict__ hdr, int C, int ncmax,
                                                   const double* __restrict__ part, void* __restrict__ state, float* __restrict__ loss,
                                                   int* __restrict__ status) {
  __shared__ double Lc[LOV_MAX_C];
  const int c = threadIdx.x;
  double total = 0.0;
  int bad = 0;
  double* st = (double*)state;
  unsigned long long* stm = (unsigned long long*)state;
  for (int s = 0; s < seg.S; ++s) {
    const bool on = c < C && lov_selected(hdr, s, c, sel);
    double L = 0.0;
    if (on) {   // the blocks' sums in index order; sixteen loads in flight per batch of adds (one load per add chains the latencies)
      const double* q = part + (size_t)c * ncmax;
      int b = seg.cblk0[s];
      const int b1 = seg.cblk0[s + 1];
      for (; b + 16 <= b1; b += 16) {
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = q[b + k];
#pragma unroll
        for (int k = 0; k < 16; ++k) L += v[k];
      }
      for (; b < b1; ++b) L += q[b];
    }
    Lc[c] = L;
    const unsigned long long mask = __ballot(on);
    __syncthreads();
    if (c == 0) {
      const int nsel = __popcll(mask);
      double sum = 0.0;
      for (int k = 0; k < C; ++k)
        if ((mask >> k) & 1ull) sum += Lc[k];
      if (nsel) total += sum / (double)nsel;
      st[1 + s] = nsel ? 1.0 / ((double)nsel * (double)seg.S) : 0.0;
      stm[1 + LOV_MAX_S + s] = mask;
      bad |= hdr[s * LOV_HDR + 1];
    }
    __syncthreads();
  }
  if (c == 0) {
    const double l = total / (double)seg.S;
    st[0] = l;
    *loss = (float)l;
    *status = bad ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------- backward
// Both forms are element-wise (thread = one (row, class) entry: every access is coalesced).  f = g / (n_selected(s) S) of the row's
// segment, 0 for an ignored row and for a class that was not selected (its coefficients were never written).
__device__ __forceinline__ double lov_bwd_factor(const LovSrc& src, const LovSeg& seg, const void* __restrict__ state, double g, long long i,
                                                 int c) {
  int s = 0;
  for (int k = 1; k < seg.S; ++k) s = seg.off[k] <= i ? k : s;
  const unsigned long long mask = lov_valid(src, src.y[i]) ? ((const unsigned long long*)state)[1 + LOV_MAX_S + s] : 0ull;
  return (mask >> c) & 1ull ? g * ((const double*)state)[1 + s] : 0.0;
}

__global__ __launch_bounds__(LOV_THREADS) void k_lov_bwd(LovSrc src, LovSeg seg, const float* __restrict__ coef, const void* __restrict__ state,
                                                          const float* __restrict__ gout, long long P, float* __restrict__ dx) {
  const double g = (double)*gout;
  const long long n = P * src.C;
  for (long long e = (long long)blockIdx.x * LOV_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * LOV_THREADS) {
    const long long i = e / src.C;
    const double f = lov_bwd_factor(src, seg, state, g, i, (int)(e - i * src.C));
    dx[e] = f != 0.0 ? (float)(f * (double)coef[e]) : 0.f;
  }
}

// logits form: a block takes tiles of LOV_BWD_ELEMS / C whole rows; dp p of every entry goes through LDS, a thread per row sums it over
// the classes in index order, and dz = p (dp - sum) is rounded once
#define LOV_BWD_K 4
#define LOV_BWD_ELEMS (LOV_THREADS * LOV_BWD_K)
__global__ __launch_bounds__(LOV_THREADS) void k_lov_bwd_logits(LovSrc src, LovSeg seg, const double* __restrict__ coef,
                                                                 const void* __restrict__ state, const float* __restrict__ gout,
                                                                 long long P, float* __restrict__ dx) {
  __shared__ double prod[LOV_BWD_ELEMS];
  __shared__ double dot[LOV_BWD_ELEMS / 2];
  const double g = (double)*gout;
  const int C = src.C, RT = LOV_BWD_ELEMS / C, tid = threadIdx.x;
  for (long long r0 = (long long)blockIdx.x * RT; r0 < P; r0 += (long long)gridDim.x * RT) {
    const int rows = P - r0 < RT ? (int)(P - r0) : RT, ne = rows * C;
    float pv[LOV_BWD_K];
    double dpv[LOV_BWD_K];
#pragma unroll
    for (int k = 0; k < LOV_BWD_K; ++k) {
      const int e = k * LOV_THREADS + tid;
      pv[k] = 0.f;
      dpv[k] = 0.0;
      if (e < ne) {
        const int r = e / C;
        const long long i = r0 + r, at = r0 * C + e;
        const double f = lov_bwd_factor(src, seg, state, g, i, e - r * C);
        dpv[k] = f != 0.0 ? f * coef[at] : 0.0;
        pv[k] = row_softmax_at(src.x[at], src.lse[i]);
        prod[e] = dpv[k] * (double)pv[k];
      }
    }
    __syncthreads();
    for (int r = tid; r < rows; r += LOV_THREADS) {
      double d = 0.0;
      for (int c = 0; c < C; ++c) d += prod[r * C + c];
      dot[r] = d;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LOV_BWD_K; ++k) {
      const int e = k * LOV_THREADS + tid;
      if (e < ne) dx[r0 * C + e] = (float)((double)pv[k] * (dpv[k] - dot[e / C]));
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------ entry points
struct LovWs {   // byte offsets
  size_t hdr, tab, tot, fgc, part, buf0, buf1, total;
  int nbmax, ncmax;
};
static inline LovWs lov_ws(int64_t P, int C, int S) {
  LovWs w;
  w.nbmax = (int)(cdiv64(P, LOV_SORT_TILE) + S);
  w.ncmax = (int)(cdiv64(P, LOV_SCAN_TILE) + S);
  w.hdr = 0;
  w.tab = align_up((size_t)LOV_MAX_S * LOV_HDR * sizeof(int), 256);
  w.tot = w.tab + align_up((size_t)C * w.nbmax * LOV_R * sizeof(int), 256);
  w.fgc = w.tot + align_up((size_t)C * S * LOV_R * sizeof(int), 256);
  w.part = w.fgc + align_up((size_t)C * w.ncmax * sizeof(int), 256);
  w.buf0 = w.part + align_up((size_t)C * w.ncmax * sizeof(double), 256);
  w.buf1 = w.buf0 + align_up((size_t)C * P * sizeof(uint2), 256);
  w.total = w.buf1 + align_up((size_t)C * P * sizeof(uint2), 256);
  return w;
}
static inline bool lov_shape_ok(int64_t P, int C, int S) {
  return P >= 1 && P < ((int64_t)1 << 31) && C >= 2 && C <= LOV_MAX_C && S >= 1 && S <= LOV_MAX_S;
}
// off_host: S + 1 non-decreasing row offsets, off[0] = 0, off[S] = P
static inline bool lov_seg_fill(LovSeg& seg, const int64_t* off_host, int S, int64_t P) {
  if (!off_host || off_host[0] != 0 || off_host[S] != P) return false;
  seg.S = S;
  int64_t sb = 0, cb = 0;
  for (int s = 0; s <= LOV_MAX_S; ++s) {
    const int k = s < S ? s : S;
    if (s < S && off_host[s + 1] < off_host[s]) return false;
    seg.off[s] = off_host[k];
    seg.sblk0[s] = (int)sb;
    seg.cblk0[s] = (int)cb;
    if (s < S) {
      sb += cdiv64(off_host[s + 1] - off_host[s], LOV_SORT_TILE);
      cb += cdiv64(off_host[s + 1] - off_host[s], LOV_SCAN_TILE);
    }
  }
  return true;
}

MOPA_API size_t mopa_lovasz_workspace_bytes(int64_t P, int32_t C, int32_t S) {
  if (!lov_shape_ok(P, C, S)) return 0;
  return lov_ws(P, C, S).total;
}

MOPA_API size_t mopa_lovasz_state_bytes(void) { return (size_t)LOV_STATE_SLOTS * 8; }

// x (P, C) float32: probabilities, or logits with from_logits != 0 (then lse, P floats, is written and p = softmax(x) is formed on the
// fly with mopa_softmax_fwd's bits).  labels (P,) int64; rows with label == ignore are skipped when has_ignore != 0.  off_host: S + 1
// row offsets of the segments (host).  class_mode 0 'present', 1 'all', 2 the classes of class_mask.  coef: (P, C) float32, or float64
// in the logits form; the entries of selected classes are written.  loss: one float32; state: mopa_lovasz_state_bytes(); status: one
// int32, rewritten by every call.
MOPA_API int mopa_lovasz_fwd(const float* x, int32_t from_logits, const int64_t* labels, int64_t P, int32_t C, const int64_t* off_host,
                             int32_t S, int64_t ignore, int32_t has_ignore, int32_t class_mode, uint64_t class_mask, float* loss,
                             void* coef, float* lse, void* state, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!lov_shape_ok(P, C, S) || !x || !labels || !loss || !coef || !state || !status || !ws || (from_logits && !lse)) return MOPA_ERR_ARG;
  if (class_mode < 0 || class_mode > 2 || ((uintptr_t)state & 7) || ((uintptr_t)ws & 255) || ((uintptr_t)coef & 7)) return MOPA_ERR_ARG;
  if (class_mode == 2 && C < 64 && (class_mask >> C)) return MOPA_ERR_ARG;
  LovSeg seg;
  if (!lov_seg_fill(seg, off_host, S, P)) return MOPA_ERR_ARG;
  const LovWs w = lov_ws(P, C, S);
  if (ws_bytes < w.total) return MOPA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* b = (char*)ws;
  int* hdr = (int*)(b + w.hdr);
  int* tab = (int*)(b + w.tab);
  int* tot = (int*)(b + w.tot);
  int* fgc = (int*)(b + w.fgc);
  double* part = (double*)(b + w.part);
  uint2* buf[2] = {(uint2*)(b + w.buf0), (uint2*)(b + w.buf1)};
  LovSrc src;
  src.x = x; src.lse = from_logits ? lse : nullptr; src.y = (const long long*)labels; src.ignore = ignore; src.has_ignore = has_ignore; src.C = C;
  LovSel sel;
  sel.mode = class_mode; sel.mask = class_mask;
  const int nb = seg.sblk0[S], nc = seg.cblk0[S];
  int64_t longest = 1;
  for (int s = 0; s < S; ++s) longest = seg.off[s + 1] - seg.off[s] > longest ? seg.off[s + 1] - seg.off[s] : longest;
  if (hipMemsetAsync(hdr, 0, (size_t)S * LOV_HDR * sizeof(int), st) != hipSuccess) return MOPA_ERR_LAUNCH;
  k_lov_count<<<dim3(stream_grid(longest, LOV_THREADS), S), LOV_THREADS, 0, st>>>(src, seg, hdr, from_logits ? lse : nullptr);
  MOPA_CHECK_LAUNCH();
  const uint2* in = nullptr;
  for (int p = 0; p < LOV_PASSES; ++p) {
    uint2* out = buf[p & 1];
    const int shift = p * LOV_BITS;
    if (p == 0) k_lov_hist<true><<<dim3(nb, C), LOV_THREADS, 0, st>>>(src, seg, sel, hdr, in, P, shift, w.nbmax, tab);
    else k_lov_hist<false><<<dim3(nb, C), LOV_THREADS, 0, st>>>(src, seg, sel, hdr, in, P, shift, w.nbmax, tab);
    MOPA_CHECK_LAUNCH();
    k_lov_rowscan<<<dim3((LOV_R + 63) / 64, C, S), LOV_SCAN_WAVES * 64, 0, st>>>(seg, sel, hdr, w.nbmax, tab, tot);
    MOPA_CHECK_LAUNCH();
    if (p == 0) k_lov_scatter<true><<<dim3(nb, C), LOV_THREADS, 0, st>>>(src, seg, sel, hdr, in, out, P, shift, w.nbmax, tab, tot);
    else k_lov_scatter<false><<<dim3(nb, C), LOV_THREADS, 0, st>>>(src, seg, sel, hdr, in, out, P, shift, w.nbmax, tab, tot);
    MOPA_CHECK_LAUNCH();
    in = out;
  }
  k_lov_fgcount<<<dim3(nc, C), LOV_THREADS, 0, st>>>(seg, sel, hdr, in, P, w.ncmax, fgc);
  MOPA_CHECK_LAUNCH();
  k_lov_weights<<<dim3(nc, C), LOV_THREADS, 0, st>>>(seg, sel, hdr, in, P, C, w.ncmax, fgc, part, from_logits ? nullptr : (float*)coef,
                                                      from_logits ? (double*)coef : nullptr);
  MOPA_CHECK_LAUNCH();
  k_lov_final<<<1, 64, 0, st>>>(seg, sel, hdr, C, w.ncmax, part, state, loss, status);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// dx (P, C) float32 of the forward call that wrote coef, lse and state: d loss / d probabilities, or d loss / d logits in the logits
// form (x = the logits).  g: one float32 on the device, the upstream gradient of the loss.
MOPA_API int mopa_lovasz_bwd(const void* coef, int32_t from_logits, const float* x, const float* lse, const int64_t* labels, int64_t P,
                             int32_t C, const int64_t* off_host, int32_t S, int64_t ignore, int32_t has_ignore, const void* state,
                             const float* g, float* dx, void* stream) {
  if (!lov_shape_ok(P, C, S) || !coef || !labels || !state || !g || !dx || (from_logits && (!x || !lse))) return MOPA_ERR_ARG;
  if (((uintptr_t)state & 7) || ((uintptr_t)coef & 7)) return MOPA_ERR_ARG;
  LovSeg seg;
  if (!lov_seg_fill(seg, off_host, S, P)) return MOPA_ERR_ARG;
  LovSrc src;
  src.x = x; src.lse = lse; src.y = (const long long*)labels; src.ignore = ignore; src.has_ignore = has_ignore; src.C = C;
  if (from_logits)
    k_lov_bwd_logits<<<stream_grid(cdiv64(P, LOV_BWD_ELEMS / C), 1), LOV_THREADS, 0, (hipStream_t)stream>>>(src, seg, (const double*)coef, state,
                                                                                                          g, P, dx);
  else
    k_lov_bwd<<<stream_grid(P * C, LOV_THREADS), LOV_THREADS, 0, (hipStream_t)stream>>>(src, seg, (const float*)coef, state, g, P, dx);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
