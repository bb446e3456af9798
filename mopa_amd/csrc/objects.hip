// Object bank on the device: the DBSCAN instances of the labelled scans of a call, for the bank of object point clouds that Valid
// Ground-based Insertion (vgi.hip) draws from -- what mopa/data/waymo/obj_point_extract.py makes offline with
// sklearn.cluster.DBSCAN(eps, min_samples).fit_predict per (scan, class) and np.unique over the labels.  The labels are sklearn's,
// exactly: clusters numbered by their lowest-index CORE point, a border point in its lowest-numbered adjacent cluster, d == eps a
// neighbour, min_samples counting the point itself.  The yardstick is the numpy restatement tests/_objects_reference.py.
//
// A fixed number of launches (mopa_objects_launches) whatever B and C are: every kernel covers all scans and all classes.  A
// SEGMENT is one (scan, class position) pair, seg = scan * C + class position; nothing links points of different segments.  The
// scans are the segments of ONE (sum N, cols) float32 array with the row0 / blk0 table of ground.hip.  No read-back here, no
// allocation, no float atomics; integer atomics only where the result does not depend on their order.
//   1. k_ob_bin      class position per row (-1: no requested class, or rejected: non-finite or |coordinate| / eps >= 2^20, counted),
//                    labels preset to -2, per block the count of every class
//   2. ordered exclusive scan of the counts laid out [scan][class][block]: where every (class, block) run starts
//   3. k_ob_order    POSITIONS: the class rows sorted by (scan, class), stable in row order -- inside a segment a smaller position is
//                    a smaller row, so "lowest index" is "lowest position" from here on.  Per position: row, cell (floor(x / eps) in
//                    float64) + segment, x y z and the float32 range
//   4. k_ob_insert   uniform grid of side eps: open-addressed table of (cell, segment) -> slot, keyed through the owner position
//                    (the first to claim a slot; who that is changes nothing but the slot's place), points per slot counted
//   5. scan of the slot counts, k_ob_fill: the points of a slot behind each other (x, y, z, position); their order inside a slot
//                    is arbitrary and no output depends on it (counts, minima and a union-find fixed point only)
//   6. k_ob_core     core[p] = #{q in the 27 cells : d2(p, q) <= eps^2} >= min_samples (stops counting there); parent[p] = p
//   7. k_ob_union    lock-free union-find over core-core edges: hook the larger root under the smaller with atomicMin, paths
//                    flattened with atomicMin; fixed point: root = smallest position of the component's core points.  An edge whose
//                    ends already show one root is skipped on a plain load (profiles/r22_objects.md)
//   8. k_ob_rootflag every parent flattened to its root, root flags; ordered scan of the flags: rank of every root
//   9. k_ob_label    cluster id = rank(root) - rank at the segment's start; a border point takes the smallest root among its core
//                    neighbours; none: -1, and the segment is marked as having noise
//  10. k_ob_segscan  instances per segment (clusters + the noise group if kept and present), exclusive scan over the segments
//  11. k_ob_count    instance of every position, points per instance, first / last position of an instance
//  12. scan of the instance counts: the offsets of the grouped points
//  13. k_ob_group    one workgroup per instance (grid-stride): its points copied out in position order, the float64 sum of the
//                    ranges in a fixed order (per thread in position order, a fixed shuffle tree, the waves in order), the table row
// d2 = (dx dx + dy dy) + dz dz in float64 from the float32 inputs, evaluated as written (no contraction).
#include "common.h"
#include "segbatch.h"

#pragma clang fp contract(off)

#define OB_ROWS 1024           // rows per block of passes 1 and 3
#ifndef OB_THREADS
#define OB_THREADS 256         // every kernel; measured against 64 and 128, profiles/r22_objects.md (-D for its A/B builds)
#endif
#ifndef OB_UNROLL
#define OB_UNROLL 4            // candidates of a cell list loaded together; measured against 1 and 8, same note
#endif
#ifndef OB_CELL_DIV
#define OB_CELL_DIV 1          // cell side eps / OB_CELL_DIV, (2 OB_CELL_DIV + 1)^3 cells searched; measured against 2, same note
#endif
#define OB_MAXC 32
#define OB_SCAN_MIN 8193       // every scan is at least this long (tail zero): always the three-launch form of mopa_scan_exclusive_i32
#define OB_LAUNCHES 25         // 2 fills + 11 kernels + 4 scans of 3
#define OB_NPARAM 4

struct ObParams {
  double eps, eps2, cell, max_distance;                // cell: the side of a grid cell
  int min_samples, include_noise, C;
  int cls[OB_MAXC];
};

__device__ __forceinline__ int ob_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ------------------------------------------------------------------------------------------ 1. class positions + block counts
// cnt[C blk0[s] + c nb_s + (blk - blk0[s])] = rows of class position c in the block (nb_s = blocks of scan s)
__global__ __launch_bounds__(OB_THREADS) void k_ob_bin(const float* __restrict__ pts, int cols, const void* __restrict__ labels, int lbytes,
                                                       const int32_t* __restrict__ tab, int B, int64_t total, const ObParams P,
                                                       int8_t* __restrict__ cls, int32_t* __restrict__ out_labels, int* __restrict__ cnt,
                                                       int* __restrict__ counters) {
  __shared__ int hist[OB_MAXC];
  const int32_t* row0 = tab;
  const int32_t* blk0 = tab + B + 1;
  const int C = P.C;
  const int s = seg_of_block(blk0, B, blockIdx.x);
  const int n = row0[s + 1] - row0[s];
  const int lb = blockIdx.x - blk0[s];
  const int nb = blk0[s + 1] <= (int)gridDim.x ? blk0[s + 1] - blk0[s] : 0;      // a table that names blocks past the grid is refused
  if (threadIdx.x < OB_MAXC) hist[threadIdx.x] = 0;
  __syncthreads();
  if (lb < nb) {
#pragma unroll
    for (int t = 0; t < OB_ROWS / OB_THREADS; ++t) {
      const int i = lb * OB_ROWS + t * OB_THREADS + threadIdx.x;
      const int64_t row = (int64_t)row0[s] + i;
      if (i < n && row >= 0 && row < total) {
        const int64_t lab = lbytes == 1 ? (int64_t)((const uint8_t*)labels)[row]
                          : lbytes == 4 ? (int64_t)((const int32_t*)labels)[row] : ((const int64_t*)labels)[row];
        int c = -1;
        for (int k = 0; k < C; ++k)
          if (lab == (int64_t)P.cls[k]) c = k;
        if (c >= 0) {
          const float* q = pts + row * cols;
          const float x = q[0], y = q[1], z = q[2];
          const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && fabs((double)x / P.eps) < 1048576.0 &&
                          fabs((double)y / P.eps) < 1048576.0 && fabs((double)z / P.eps) < 1048576.0;
          if (!ok) {
            atomicAdd(&counters[0], 1);                // integer count: the result does not depend on the order
            c = -1;
          }
        }
        cls[row] = (int8_t)c;
        out_labels[row] = -2;
        if (c >= 0) atomicAdd(&hist[c], 1);
      }
    }
  }
  __syncthreads();
  if (lb < nb && (int)threadIdx.x < C) cnt[(int64_t)C * blk0[s] + (int64_t)threadIdx.x * nb + lb] = hist[threadIdx.x];
}

// ------------------------------------------------------------------------------------------ 3. the positions
// The waves of a block take their OB_ROWS / 4 rows one after the other; ranks by ballot inside a wave (the form of k_gr_order).
__global__ __launch_bounds__(OB_THREADS) void k_ob_order(const float* __restrict__ pts, int cols, const int32_t* __restrict__ tab, int B,
                                                         int64_t total, const ObParams P, const int8_t* __restrict__ cls,
                                                         const int* __restrict__ scan, int* __restrict__ order, int4* __restrict__ cell4,
                                                         float4* __restrict__ pos4) {
  __shared__ int run[OB_MAXC];
  const int32_t* row0 = tab;
  const int32_t* blk0 = tab + B + 1;
  const int C = P.C;
  const int s = seg_of_block(blk0, B, blockIdx.x);
  const int n = row0[s + 1] - row0[s];
  const int lb = blockIdx.x - blk0[s];
  const int nb = blk0[s + 1] <= (int)gridDim.x ? blk0[s + 1] - blk0[s] : 0;
  if (lb >= nb) return;                                // uniform over the block
  if ((int)threadIdx.x < C) run[threadIdx.x] = scan[(int64_t)C * blk0[s] + (int64_t)threadIdx.x * nb + lb];
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  constexpr int WROWS = OB_ROWS / (OB_THREADS / 64);   // consecutive rows of one wave
  for (int turn = 0; turn < OB_THREADS / 64; ++turn) {
    if (w == turn) {
      for (int t = 0; t < WROWS / 64; ++t) {
        const int i = lb * OB_ROWS + w * WROWS + t * 64 + lane;
        const int64_t row = (int64_t)row0[s] + i;
        const int c = (i < n && row >= 0 && row < total) ? (int)cls[row] : -1;
        bool todo = c >= 0 && c < C;
        unsigned long long act = __ballot(todo);
        while (act) {                                  // uniform over the wave: one round per distinct class among the 64 rows
          const int k = __shfl(c, __ffsll((long long)act) - 1);
          const bool mine = todo && c == k;
          const unsigned long long m = __ballot(mine);
          const int at = run[k];
          if (mine) {
            const int64_t dst = (int64_t)at + __popcll(m & below);
            if (dst >= 0 && dst < total) {
              const float* q = pts + row * cols;
              const float x = q[0], y = q[1], z = q[2];
              order[dst] = (int)row;
              cell4[dst] = make_int4((int)floor((double)x / P.cell), (int)floor((double)y / P.cell), (int)floor((double)z / P.cell), s * C + c);
              const float r2 = ((x * x + y * y) + z * z) + 0.00001f;
              pos4[dst] = make_float4(x, y, z, (float)sqrt((double)r2));   // float32 sqrt, correctly rounded (53 >= 2 * 24 + 2 bits)
            }
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

// ------------------------------------------------------------------------------------------ 4. / 5. the grid
__device__ __forceinline__ uint32_t ob_hash(int cx, int cy, int cz, int seg) {
  uint32_t h = (uint32_t)cx * 73856093u ^ (uint32_t)cy * 19349663u ^ (uint32_t)cz * 83492791u ^ (uint32_t)seg * 0x9E3779B1u;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
  return h;
}
__device__ __forceinline__ bool ob_same(const int4 a, const int4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// table[slot] = owner position or -1.  At most half of the hmask + 1 slots are ever taken (hmask + 1 >= 2 total rows): a probe ends.
__global__ __launch_bounds__(OB_THREADS) void k_ob_insert(const int* __restrict__ pT, int64_t total, const int4* __restrict__ cell4, int hmask,
                                                          int* __restrict__ table, int* __restrict__ slotof, int* __restrict__ ccount) {
  const int64_t p = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
  const int T = *pT;
  if (p >= T || p >= total) return;
  const int4 key = cell4[p];
  uint32_t h = ob_hash(key.x, key.y, key.z, key.w) & (uint32_t)hmask;
  for (int probe = 0; probe <= hmask; ++probe) {
    int q = ob_ld(&table[h]);
    if (q < 0) {
      q = atomicCAS(&table[h], -1, (int)p);
      if (q < 0) q = (int)p;
    }
    if (q == (int)p || (q < total && ob_same(cell4[q], key))) {
      slotof[p] = (int)h;
      atomicAdd(&ccount[h], 1);
      return;
    }
    h = (h + 1) & (uint32_t)hmask;
  }
}

__global__ __launch_bounds__(OB_THREADS) void k_ob_fill(const int* __restrict__ pT, int64_t total, const float4* __restrict__ pos4,
                                                        const int* __restrict__ slotof, const int* __restrict__ cstart, int* __restrict__ ccount,
                                                        float4* __restrict__ cellpts, int* __restrict__ cellidx) {
  const int64_t p = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
  const int T = *pT;
  if (p >= T || p >= total) return;
  const int slot = slotof[p];
  const int64_t at = (int64_t)cstart[slot] + atomicSub(&ccount[slot], 1) - 1;
  if (at < 0 || at >= total) return;
  const float4 v = pos4[p];
  cellpts[at] = make_float4(v.x, v.y, v.z, __int_as_float((int)p));
  cellidx[p] = (int)at;
}

// the slot of a cell of a segment, -1 if it holds no point
__device__ __forceinline__ int ob_lookup(const int* __restrict__ table, const int4* __restrict__ cell4, int hmask, const int4 key) {
  uint32_t h = ob_hash(key.x, key.y, key.z, key.w) & (uint32_t)hmask;
  for (int probe = 0; probe <= hmask; ++probe) {
    const int q = table[h];
    if (q < 0) return -1;
    if (ob_same(cell4[q], key)) return (int)h;
    h = (h + 1) & (uint32_t)hmask;
  }
  return -1;
}

struct ObGrid {
  const int* table;
  const int4* cell4;
  const int* cstart;
  const float4* cellpts;
  int hmask;
};

__device__ __forceinline__ double ob_d2(const float4 a, const float4 b) {
  const double ex = (double)a.x - (double)b.x, ey = (double)a.y - (double)b.y, ez = (double)a.z - (double)b.z;
  return (ex * ex + ey * ey) + ez * ez;
}

// f(position of the neighbour, its place in the cell lists) for every q (p itself included) of p's segment with d2(p, q) <= eps2;
// f returns false to stop
template <typename F>
__device__ __forceinline__ void ob_neighbours(const ObGrid& G, const int4 key, const float4 me, double eps2, F f) {
  for (int dz = -OB_CELL_DIV; dz <= OB_CELL_DIV; ++dz)
    for (int dy = -OB_CELL_DIV; dy <= OB_CELL_DIV; ++dy)
      for (int dx = -OB_CELL_DIV; dx <= OB_CELL_DIV; ++dx) {
        const int slot = ob_lookup(G.table, G.cell4, G.hmask, make_int4(key.x + dx, key.y + dy, key.z + dz, key.w));
        if (slot < 0) continue;
        const int end = G.cstart[slot + 1];
        int k = G.cstart[slot];
        for (; k + OB_UNROLL <= end; k += OB_UNROLL) {    // the loads of OB_UNROLL candidates in flight together
          float4 q[OB_UNROLL];
#pragma unroll
          for (int u = 0; u < OB_UNROLL; ++u) q[u] = G.cellpts[k + u];
#pragma unroll
          for (int u = 0; u < OB_UNROLL; ++u)
            if (ob_d2(me, q[u]) <= eps2)
              if (!f(__float_as_int(q[u].w), k + u)) return;
        }
        for (; k < end; ++k) {
          const float4 q = G.cellpts[k];
          if (ob_d2(me, q) <= eps2)
            if (!f(__float_as_int(q.w), k)) return;
        }
      }
}

// ------------------------------------------------------------------------------------------ 6. core flags
__global__ __launch_bounds__(OB_THREADS) void k_ob_core(const int* __restrict__ pT, int64_t total, const ObGrid G, const float4* __restrict__ pos4,
                                                        const ObParams P, const int* __restrict__ cellidx, uint8_t* __restrict__ core,
                                                        uint8_t* __restrict__ ccore, int* __restrict__ parent) {
  const int64_t p = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
  const int T = *pT;
  if (p >= T || p >= total) return;
  int n = 0;
  const int need = P.min_samples;
  ob_neighbours(G, G.cell4[p], pos4[p], P.eps2, [&](int, int) { return ++n < need; });
  core[p] = n >= need;
  const int at = cellidx[p];
  if (at >= 0 && at < total) ccore[at] = n >= need;    // the same flag in cell-list order: read along with the cell's points
  parent[p] = (int)p;
}

// ------------------------------------------------------------------------------------------ 7. components
// parent[x] <= x always and only ever decreases; every value it takes is a member of x's component.
__device__ __forceinline__ int ob_find(int* parent, int x) {
  int p = ob_ld(&parent[x]);
  while (p != x) {
    const int g = ob_ld(&parent[p]);
    if (g != p) atomicMin(&parent[x], g);              // flattening
    x = p;
    p = g;
  }
  return x;
}
__device__ __forceinline__ void ob_unite(int* parent, int a, int b) {
  for (;;) {
    a = ob_find(parent, a);
    b = ob_find(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicMin(&parent[hi], lo);
    if (old == hi) return;                             // hi was a root and hangs under lo now
    a = old;                                           // somebody hooked hi under `old` first: old and lo are still to be joined
    b = lo;
  }
}

__global__ __launch_bounds__(OB_THREADS) void k_ob_union(const int* __restrict__ pT, int64_t total, const ObGrid G, const float4* __restrict__ pos4,
                                                         const ObParams P, const uint8_t* __restrict__ core, const uint8_t* __restrict__ ccore,
                                                         int* parent) {
  const int64_t p = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
  const int T = *pT;
  if (p >= T || p >= total || !core[p]) return;
  // Every edge once, from its larger end.  Most edges join what is joined already: rp is a root p's tree had, parent[q] (a plain
  // load, possibly an old value) a member of q's tree; trees only ever merge, so equal values mean one tree and the edge is done.
  int rp = ob_find(parent, (int)p);
  ob_neighbours(G, G.cell4[p], pos4[p], P.eps2, [&](int q, int k) {
    if (q < (int)p && ccore[k] && parent[q] != rp) {
      ob_unite(parent, (int)p, q);
      rp = ob_find(parent, (int)p);
    }
    return true;
  });
}

// ------------------------------------------------------------------------------------------ 8. roots
// flag[i] for every i < nflag (the scan's padded length); parent[i] = its root for every core point
__global__ __launch_bounds__(OB_THREADS) void k_ob_rootflag(const int* __restrict__ pT, int64_t total, int nflag, const uint8_t* __restrict__ core,
                                                            int* __restrict__ parent, int* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
  if (i >= nflag) return;
  const int T = *pT;
  int f = 0;
  if (i < T && i < total && core[i]) {
    int x = (int)i, p = ob_ld(&parent[x]);
    while (p != x) { x = p; p = ob_ld(&parent[x]); }   // read only: other threads walk through the same links
    atomicMin(&parent[i], x);
    f = x == (int)i;
  }
  flag[i] = f;
}

// ------------------------------------------------------------------------------------------ 9. labels
// first position of segment seg in the ordering, and one past its last
__device__ __forceinline__ void ob_seg_range(const int32_t* __restrict__ tab, int B, int C, const int* __restrict__ scan, int seg, int nblk,
                                             int& start, int& end) {
  const int32_t* blk0 = tab + B + 1;
  const int s = seg / C, c = seg - s * C;
  start = end = 0;
  if (s < 0 || s >= B || blk0[s] < 0 || blk0[s + 1] < blk0[s] || blk0[s + 1] > nblk) return;
  const int nb = blk0[s + 1] - blk0[s];
  const int64_t at = (int64_t)C * blk0[s] + (int64_t)c * nb;
  start = scan[at];
  end = scan[at + nb];                                 // at + nb: the next class, the next scan or the grand total
}

__global__ __launch_bounds__(OB_THREADS) void k_ob_label(const int* __restrict__ pT, int64_t total, const ObGrid G, const float4* __restrict__ pos4,
                                                         const ObParams P, const int32_t* __restrict__ tab, int B, int nblk,
                                                         const int* __restrict__ scan, const uint8_t* __restrict__ core,
                                                         const uint8_t* __restrict__ ccore, const int* __restrict__ parent, const int* __restrict__ rscan,
                                                         const int* __restrict__ order, int* __restrict__ lab, int32_t* __restrict__ out_labels,
                                                         int* __restrict__ noiseflag) {
  const int64_t p = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
  const int T = *pT;
  if (p >= T || p >= total) return;
  const int4 key = G.cell4[p];
  int root = 0x7fffffff;
  if (core[p]) root = parent[p];
  else
    ob_neighbours(G, key, pos4[p], P.eps2, [&](int q, int k) {
      if (ccore[k]) { const int r = parent[q]; root = r < root ? r : root; }
      return true;
    });
  int id = -1;
  if (root != 0x7fffffff) {
    int start, end;
    ob_seg_range(tab, B, P.C, scan, key.w, nblk, start, end);
    id = rscan[root] - rscan[start];
  } else noiseflag[key.w] = 1;                          // every writer writes the same value
  lab[p] = id;
  const int row = order[p];
  if (row >= 0 && row < total) out_labels[row] = id;
}

// ------------------------------------------------------------------------------------------ 10. instances per segment
__global__ __launch_bounds__(OB_THREADS) void k_ob_segscan(const int32_t* __restrict__ tab, int B, int nblk, const ObParams P,
                                                           const int* __restrict__ scan, const int* __restrict__ rscan,
                                                           const int* __restrict__ noiseflag, int* __restrict__ instbase, int* __restrict__ counters) {
  __shared__ int wsum[OB_THREADS / 64];
  __shared__ int carry_s;
  const int S = B * P.C;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < S; base += OB_THREADS) {
    const int seg = base + threadIdx.x;
    int v = 0;
    if (seg < S) {
      int start, end;
      ob_seg_range(tab, B, P.C, scan, seg, nblk, start, end);
      v = (rscan[end] - rscan[start]) + ((P.include_noise && noiseflag[seg]) ? 1 : 0);
    }
    int inc = v;                                       // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int before = carry_s;
    for (int k = 0; k < w; ++k) before += wsum[k];
    if (seg < S) instbase[seg] = before + inc - v;
    __syncthreads();
    if (threadIdx.x == OB_THREADS - 1) carry_s = before + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    instbase[S] = carry_s;
    counters[1] = carry_s;
  }
}

// ------------------------------------------------------------------------------------------ 11. points per instance
// span[2 i] = max(total - first position), span[2 i + 1] = max(last position + 1): zero-initialised maxima
__global__ __launch_bounds__(OB_THREADS) void k_ob_count(const int* __restrict__ pT, int64_t total, int64_t maxinst, const ObParams P,
                                                         const int4* __restrict__ cell4, const int* __restrict__ lab,
                                                         const int* __restrict__ noiseflag, const int* __restrict__ instbase,
                                                         int* __restrict__ instof, int* __restrict__ icount, int* __restrict__ span) {
  const int64_t p = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
  const int T = *pT;
  if (p >= T || p >= total) return;
  const int seg = cell4[p].w, id = lab[p];
  const int nz = (P.include_noise && noiseflag[seg]) ? 1 : 0;
  int64_t inst = -1;
  if (id >= 0 || P.include_noise) inst = (int64_t)instbase[seg] + id + nz;     // the noise group (id -1) is the segment's first
  if (inst < 0 || inst >= maxinst) inst = -1;
  instof[p] = (int)inst;
  if (inst >= 0) {
    atomicAdd(&icount[inst], 1);
    atomicMax(&span[2 * inst], (int)(total - p));
    atomicMax(&span[2 * inst + 1], (int)p + 1);
  }
}

// ------------------------------------------------------------------------------------------ 13. table + grouped points
__global__ __launch_bounds__(OB_THREADS) void k_ob_group(const float* __restrict__ pts, int cols, int64_t total, int B, const ObParams P,
                                                         const int* __restrict__ order, const float4* __restrict__ pos4,
                                                         const int* __restrict__ noiseflag, const int* __restrict__ instbase,
                                                         const int* __restrict__ instof, const int* __restrict__ ioffs, const int* __restrict__ span,
                                                         int32_t* __restrict__ table, int32_t* __restrict__ offsets, double* __restrict__ mean_range,
                                                         uint8_t* __restrict__ keep, float* __restrict__ out_points, const int* __restrict__ cws,
                                                         int32_t* __restrict__ counters) {
  __shared__ int wcnt[OB_THREADS / 64];
  __shared__ double wred[OB_THREADS / 64];
  const int S = B * P.C;
  const int M = instbase[S];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    offsets[M] = ioffs[M];
    counters[0] = cws[0];
    counters[1] = M;
    counters[2] = ioffs[M];
  }
  for (int inst = blockIdx.x; inst < M; inst += gridDim.x) {
    int lo = 0, hi = S;                                // the segment: the last one with instbase[seg] <= inst < instbase[seg + 1]
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (instbase[mid] <= inst) lo = mid + 1; else hi = mid;
    }
    const int seg = lo - 1;
    const int first = (int)(total - span[2 * inst]), last = span[2 * inst + 1];
    const int64_t out0 = ioffs[inst];
    const int n = ioffs[inst + 1] - ioffs[inst];
    int done = 0;
    double sum = 0;
    for (int b0 = first; b0 < last; b0 += OB_THREADS) {
      const int p = b0 + threadIdx.x;
      const bool mine = p < last && p >= 0 && p < total && instof[p] == inst;
      const unsigned long long m = __ballot(mine);
      if (lane == 0) wcnt[w] = __popcll(m);
      __syncthreads();
      int before = done, all = 0;
#pragma unroll
      for (int k = 0; k < OB_THREADS / 64; ++k) {
        if (k < w) before += wcnt[k];
        all += wcnt[k];
      }
      if (mine) {
        const int64_t dst = out0 + before + __popcll(m & below);
        const int row = order[p];
        if (dst >= 0 && dst < total && row >= 0 && row < total) {
          const float* q = pts + (int64_t)row * cols;
          float* o = out_points + dst * cols;
          for (int k = 0; k < cols; ++k) o[k] = q[k];
        }
        sum += (double)pos4[p].w;
      }
      done += all;
      __syncthreads();
    }
    sum = wave_sum_d(sum);
    if (lane == 0) wred[w] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = wred[0];
#pragma unroll
      for (int k = 1; k < OB_THREADS / 64; ++k) t = t + wred[k];
      const double mean = t / (double)n;
      const int nz = (P.include_noise && noiseflag[seg]) ? 1 : 0;
      table[4 * inst + 0] = seg / P.C;
      table[4 * inst + 1] = seg % P.C;
      table[4 * inst + 2] = inst - instbase[seg] - nz;
      table[4 * inst + 3] = n;
      offsets[inst] = (int)out0;
      mean_range[inst] = mean;
      keep[inst] = mean <= P.max_distance;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------ entry points
MOPA_API int mopa_objects_rows_per_block(void) { return OB_ROWS; }
MOPA_API int mopa_objects_max_classes(void) { return OB_MAXC; }
MOPA_API int mopa_objects_num_params(void) { return OB_NPARAM; }
// kernel launches and device fills of one mopa_objects_extract with points: the same for every B, C and size
MOPA_API int mopa_objects_launches(void) { return OB_LAUNCHES; }
// rows of `table` / `mean_range` / `keep` (and, plus one, of `offsets`) a call may write: a cluster has at least one point, a
// segment at most one noise group
MOPA_API size_t mopa_objects_max_instances(int64_t total_rows, int32_t B, int32_t C) {
  if (total_rows < 0 || B < 1 || C < 1) return 0;
  return (size_t)total_rows + (size_t)B * (size_t)C;
}

// workspace: [zeroed: cnt | ccount | noiseflag | icount | span | counters] [set to -1: table] scan | order | cell4 | pos4 | slotof |
// cstart | cellpts | cellidx | core | ccore | parent | rflag | rscan | lab | instbase | instof | ioffs | cls | totals | scratch of the scans
struct ObLay {
  int64_t nA, H, nH, nF, MI, nI;
  size_t cnt, ccount, noiseflag, icount, span, counters, zero_end, table, table_end, scan, order, cell4, pos4, slotof, cstart, cellpts, cellidx, core,
         ccore, parent, rflag, rscan, lab, instbase, instof, ioffs, cls, tot, sws, end;
};
static ObLay ob_layout(int64_t R, int64_t NB, int64_t S, int64_t C) {
  ObLay L;
  L.nA = C * NB + 1 > OB_SCAN_MIN ? C * NB + 1 : OB_SCAN_MIN;
  L.H = 1024;
  while (L.H < 2 * R) L.H <<= 1;
  L.nH = L.H + 1 > OB_SCAN_MIN ? L.H + 1 : OB_SCAN_MIN;
  L.nF = R + 1 > OB_SCAN_MIN ? R + 1 : OB_SCAN_MIN;
  L.MI = R + S;
  L.nI = L.MI + 1 > OB_SCAN_MIN ? L.MI + 1 : OB_SCAN_MIN;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += align_up(bytes, 256); return o; };
  L.cnt = take(L.nA * 4);
  L.ccount = take(L.nH * 4);
  L.noiseflag = take(S * 4);
  L.icount = take(L.nI * 4);
  L.span = take(2 * L.MI * 4);
  L.counters = take(16);
  L.zero_end = at;
  L.table = take(L.H * 4);
  L.table_end = at;
  L.scan = take(L.nA * 4);
  L.order = take(R * 4);
  L.cell4 = take(R * 16);
  L.pos4 = take(R * 16);
  L.slotof = take(R * 4);
  L.cstart = take(L.nH * 4);
  L.cellpts = take(R * 16);
  L.cellidx = take(R * 4);
  L.core = take(R);
  L.ccore = take(R);
  L.parent = take(R * 4);
  L.rflag = take(L.nF * 4);
  L.rscan = take(L.nF * 4);
  L.lab = take(R * 4);
  L.instbase = take((S + 1) * 4);
  L.instof = take(R * 4);
  L.ioffs = take(L.nI * 4);
  L.cls = take(R);
  L.tot = take(16);
  L.sws = at;
  int64_t nmax = L.nA;
  if (L.nH > nmax) nmax = L.nH;
  if (L.nF > nmax) nmax = L.nF;
  if (L.nI > nmax) nmax = L.nI;
  at += mopa_scan_workspace_bytes(nmax);
  L.end = at;
  return L;
}
static bool ob_sizes_ok(int64_t total_rows, int64_t total_blocks, int32_t B, int32_t C) {
  if (B < 1 || C < 1 || C > OB_MAXC || (int64_t)B * C > 65535 || total_rows < 0 || total_rows >= (int64_t)1 << 28 || total_blocks < 0) return false;
  if (total_blocks > total_rows || total_blocks * OB_ROWS < total_rows || total_blocks > total_rows / OB_ROWS + B) return false;
  return true;
}
MOPA_API size_t mopa_objects_workspace_bytes(int64_t total_rows, int64_t total_blocks, int32_t B, int32_t C) {
  if (!ob_sizes_ok(total_rows, total_blocks, B, C)) return 0;
  return ob_layout(total_rows, total_blocks, (int64_t)B * C, C).end;
}

// The DBSCAN instances of C classes in B labelled scans that lie behind each other in points (total_rows, cols) float32 (cols >= 3,
// the first three columns are x, y, z) with labels (total_rows) of label_bytes = 1 (uint8), 4 (int32) or 8 (int64) each.  tab
// (device, 2 (B + 1) int32): row0[B + 1] then blk0[B + 1] as mopa_ground_estimate takes them, a scan of n rows having
// ceil(n / mopa_objects_rows_per_block()) blocks.  class_ids_host: C distinct class ids (C <= mopa_objects_max_classes(), B C <=
// 65535).  params_host: mopa_objects_num_params() doubles -- eps, min_samples, max_distance, include_noise.  Outputs (device):
//   out_labels (total_rows) int32: -2 = no requested class or rejected, -1 = noise, >= 0 = the cluster id inside its segment
//   table (M, 4) int32: scan, class position, instance id (-1 = the segment's noise group, which comes first), points
//   offsets (M + 1) int32, mean_range (M) float64, keep (M) uint8 = mean_range <= max_distance,
//   out_points (total, cols) float32: the points of instance i are rows offsets[i] .. offsets[i + 1], in row order,
//   counters (3) int32: rejected rows, M, total.
// table / mean_range / keep hold mopa_objects_max_instances() rows, offsets one more, out_points total_rows rows.
MOPA_API int mopa_objects_extract(const float* points, int32_t cols, const void* labels, int32_t label_bytes, const int32_t* tab, int32_t B,
                                  int64_t total_rows, int64_t total_blocks, const int32_t* class_ids_host, int32_t C, const double* params_host,
                                  int32_t* out_labels, int32_t* table, int32_t* offsets, double* mean_range, uint8_t* keep, float* out_points,
                                  int32_t* counters, void* ws, size_t ws_bytes, void* stream) {
  if (!ob_sizes_ok(total_rows, total_blocks, B, C) || cols < 3 || !params_host || !class_ids_host || !tab || !counters || !offsets) return MOPA_ERR_ARG;
  if (label_bytes != 1 && label_bytes != 4 && label_bytes != 8) return MOPA_ERR_ARG;
  ObParams P;
  P.eps = params_host[0];
  P.eps2 = P.eps * P.eps;
  P.cell = P.eps / OB_CELL_DIV;
  P.max_distance = params_host[2];
  P.min_samples = (int)params_host[1];
  P.include_noise = params_host[3] != 0.0;
  P.C = C;
  if (!(P.eps > 0 && P.eps <= 1e18) || P.min_samples < 1 || !(params_host[1] <= 1 << 30) || P.max_distance != P.max_distance) return MOPA_ERR_ARG;
  for (int k = 0; k < OB_MAXC; ++k) P.cls[k] = k < C ? class_ids_host[k] : 0;
  for (int k = 0; k < C; ++k)
    for (int j = 0; j < k; ++j)
      if (P.cls[j] == P.cls[k]) return MOPA_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (total_rows == 0) {
    if (hipMemsetAsync(counters, 0, 3 * sizeof(int32_t), st) != hipSuccess || hipMemsetAsync(offsets, 0, sizeof(int32_t), st) != hipSuccess) return MOPA_ERR_LAUNCH;
    return MOPA_OK;
  }
  if (!points || !labels || !out_labels || !table || !mean_range || !keep || !out_points || !ws) return MOPA_ERR_ARG;
  const int S = B * C;
  const ObLay L = ob_layout(total_rows, total_blocks, S, C);
  if (ws_bytes < L.end) return MOPA_ERR_WORKSPACE;
  char* w = (char*)ws;
  int* cnt = (int*)(w + L.cnt);
  int* ccount = (int*)(w + L.ccount);
  int* noiseflag = (int*)(w + L.noiseflag);
  int* icount = (int*)(w + L.icount);
  int* span = (int*)(w + L.span);
  int* cws = (int*)(w + L.counters);
  int* tbl = (int*)(w + L.table);
  int* scan = (int*)(w + L.scan);
  int* order = (int*)(w + L.order);
  int4* cell4 = (int4*)(w + L.cell4);
  float4* pos4 = (float4*)(w + L.pos4);
  int* slotof = (int*)(w + L.slotof);
  int* cstart = (int*)(w + L.cstart);
  float4* cellpts = (float4*)(w + L.cellpts);
  int* cellidx = (int*)(w + L.cellidx);
  uint8_t* core = (uint8_t*)(w + L.core);
  uint8_t* ccore = (uint8_t*)(w + L.ccore);
  int* parent = (int*)(w + L.parent);
  int* rflag = (int*)(w + L.rflag);
  int* rscan = (int*)(w + L.rscan);
  int* lab = (int*)(w + L.lab);
  int* instbase = (int*)(w + L.instbase);
  int* instof = (int*)(w + L.instof);
  int* ioffs = (int*)(w + L.ioffs);
  int8_t* cls = (int8_t*)(w + L.cls);
  int* tot = (int*)(w + L.tot);
  void* sws = w + L.sws;
  const size_t sws_bytes = L.end - L.sws;
  const int nblk = (int)total_blocks;
  const int hmask = (int)(L.H - 1);
  const int* pT = scan + (int64_t)C * nblk;            // the grand total of the first scan: the number of positions
  const int gp = (int)cdiv64(total_rows, OB_THREADS);
  const ObGrid G = {tbl, cell4, cstart, cellpts, hmask};
  if (hipMemsetAsync(w, 0, L.zero_end, st) != hipSuccess || hipMemsetAsync(tbl, 0xFF, L.table_end - L.table, st) != hipSuccess) return MOPA_ERR_LAUNCH;
  k_ob_bin<<<nblk, OB_THREADS, 0, st>>>(points, cols, labels, label_bytes, tab, B, total_rows, P, cls, out_labels, cnt, cws);
  MOPA_CHECK_LAUNCH();
  int rc = mopa_scan_exclusive_i32(cnt, scan, (int)L.nA, tot, sws, sws_bytes, stream);
  if (rc) return rc;
  k_ob_order<<<nblk, OB_THREADS, 0, st>>>(points, cols, tab, B, total_rows, P, cls, scan, order, cell4, pos4);
  k_ob_insert<<<gp, OB_THREADS, 0, st>>>(pT, total_rows, cell4, hmask, tbl, slotof, ccount);
  MOPA_CHECK_LAUNCH();
  rc = mopa_scan_exclusive_i32(ccount, cstart, (int)L.nH, tot + 1, sws, sws_bytes, stream);
  if (rc) return rc;
  k_ob_fill<<<gp, OB_THREADS, 0, st>>>(pT, total_rows, pos4, slotof, cstart, ccount, cellpts, cellidx);
  k_ob_core<<<gp, OB_THREADS, 0, st>>>(pT, total_rows, G, pos4, P, cellidx, core, ccore, parent);
  k_ob_union<<<gp, OB_THREADS, 0, st>>>(pT, total_rows, G, pos4, P, core, ccore, parent);
  k_ob_rootflag<<<(int)cdiv64(L.nF, OB_THREADS), OB_THREADS, 0, st>>>(pT, total_rows, (int)L.nF, core, parent, rflag);
  MOPA_CHECK_LAUNCH();
  rc = mopa_scan_exclusive_i32(rflag, rscan, (int)L.nF, tot + 2, sws, sws_bytes, stream);
  if (rc) return rc;
  k_ob_label<<<gp, OB_THREADS, 0, st>>>(pT, total_rows, G, pos4, P, tab, B, nblk, scan, core, ccore, parent, rscan, order, lab, out_labels, noiseflag);
  k_ob_segscan<<<1, OB_THREADS, 0, st>>>(tab, B, nblk, P, scan, rscan, noiseflag, instbase, cws);
  k_ob_count<<<gp, OB_THREADS, 0, st>>>(pT, total_rows, L.MI, P, cell4, lab, noiseflag, instbase, instof, icount, span);
  MOPA_CHECK_LAUNCH();
  rc = mopa_scan_exclusive_i32(icount, ioffs, (int)L.nI, tot + 3, sws, sws_bytes, stream);
  if (rc) return rc;
  const int gg = L.MI < 2048 ? (int)L.MI : 2048;
  k_ob_group<<<gg, OB_THREADS, 0, st>>>(points, cols, total_rows, B, P, order, pos4, noiseflag, instbase, instof, ioffs, span, table, offsets,
                                        mean_range, keep, out_points, cws, counters);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
