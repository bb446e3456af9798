// The skeleton the input-pipeline stages share (scanprep, kittiprep, nuscprep, a2d2prep; ground and objects use the lookup): a
// call's scans ("segments") are processed by a fixed number of launches whatever their number is.
//
// A segment of n rows is cut into blocks of `rows_per_block` rows, a block never spans two segments.  The host builds the block
// table (SegTable: blk0[s] = first block of segment s, row0[s] = its first row in the call's flat row numbering; both have one
// entry more, the totals) and hands it to the kernels by value; a block finds its segment with seg_of_block.  A flags pass
// leaves per block P integer counts, plane after plane (cnt[p * nblk + blk], block_counts); ONE ordered exclusive scan over all
// planes (SegCounts, seg_counts_scan) turns them into the first output row of every block, and the compaction places a row at
// its block's offset + its rank among the block's rows (block_rank).  Integer counts and an ordered scan: deterministic.
//
// Included after common.h.  One translation unit per .hip, no RDC: everything here is static inline / __forceinline__.
#pragma once

extern "C" int mopa_scan_exclusive_i32(const int32_t* in, int32_t* out, int32_t n, int32_t* total, void* ws, size_t ws_bytes, void* stream);
extern "C" size_t mopa_scan_workspace_bytes(int64_t n);

// ------------------------------------------------------------------------------------------ device
// the segment of a block: the last s < S with blk0[s] <= blk, for a non-decreasing table with blk0[0] == 0 (empty segments share
// their successor's first block and are never returned for a block that exists)
__device__ __forceinline__ int seg_of_block(const int32_t* __restrict__ blk0, int S, int blk) {
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (blk0[mid] <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// rank of the thread among the block's threads with p, in thread order, and their number.  lds: THREADS / 64 ints; two barriers.
template <int THREADS>
__device__ __forceinline__ int block_rank(bool p, int* lds, int& total) {
  const unsigned long long m = __ballot(p);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) lds[w] = __popcll(m);
  __syncthreads();
  int pre = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < THREADS / 64; ++k) { const int c = lds[k]; pre += k < w ? c : 0; tot += c; }
  __syncthreads();
  total = tot;
  return pre + r;
}
// cnt[k * nblk + blockIdx.x] = the sum of c[k] over the block's 256 threads, for the planes k < K whose bit is set in `planes`
template <int K>
__device__ __forceinline__ void block_counts(const int (&c)[K], int* __restrict__ cnt, int nblk, unsigned planes = ~0u) {
  __shared__ int red[4][K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int v = wave_sum_i(c[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < K && (planes >> k & 1u)) cnt[(K > 1 ? k * nblk : 0) + blockIdx.x] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
}

// ------------------------------------------------------------------------------------------ host: the block table
template <int MAXS>
struct SegTable {
  int32_t n[MAXS];
  int32_t row0[MAXS + 1];           // first row of the segment in the call's flat row numbering; row0[S] = all rows
  int32_t blk0[MAXS + 1];           // first block of the segment; blk0[S] = all blocks
};
// -> the number of blocks, or -1 (no table, S outside 1 .. MAXS, a negative n, 2^30 rows or more in all)
template <int MAXS>
static inline int seg_table_fill(SegTable<MAXS>& t, const int32_t* n_host, int S, int rows_per_block) {
  if (!n_host || S < 1 || S > MAXS) return -1;
  int64_t blk = 0, row = 0;
  for (int s = 0; s < S; ++s) {
    if (n_host[s] < 0) return -1;
    t.n[s] = n_host[s];
    t.row0[s] = (int32_t)row;
    t.blk0[s] = (int32_t)blk;
    blk += cdiv64(n_host[s], rows_per_block);
    row += n_host[s];
    if (row >= (int64_t)1 << 30) return -1;
  }
  t.row0[S] = (int32_t)row;
  t.blk0[S] = (int32_t)blk;
  return (int)blk;
}

// ------------------------------------------------------------------------------------------ host: counts, scan, workspace
// P count planes of nblk blocks behind `prefix` ints of the caller's own:
//   prefix | cnt [P nblk + 1] | scan [P nblk + 1] | total | (spare, 16 ints with the three above) | scratch of the scan
// One more (zero) item than counts, so that scan[P nblk], the grand total, exists for every lookup of blk0[S].
struct SegCounts {
  int items;                        // P nblk + 1
  int *cnt, *scan, *total;
  void* sws;
  size_t sws_bytes;
};
static inline size_t seg_counts_head(int P, int64_t nblk, int prefix) { return align_up((size_t)(prefix + 2 * P * nblk + 16) * sizeof(int), 256); }
static inline size_t seg_counts_bytes(int P, int64_t nblk, int prefix = 0) {
  return seg_counts_head(P, nblk, prefix) + mopa_scan_workspace_bytes(P * nblk + 1);
}
static inline SegCounts seg_counts(void* ws, int P, int nblk, int prefix = 0) {
  SegCounts c;
  c.items = P * nblk + 1;
  c.cnt = (int*)ws + prefix;
  c.scan = c.cnt + c.items;
  c.total = c.scan + c.items;
  c.sws = (char*)ws + seg_counts_head(P, nblk, prefix);
  c.sws_bytes = mopa_scan_workspace_bytes(c.items);
  return c;
}
// scan = exclusive scan of cnt; `clear`: the extra item is zeroed first (not needed again when the same counts are scanned twice)
static inline int seg_counts_scan(const SegCounts& c, void* stream, bool clear = true) {
  if (clear && hipMemsetAsync(c.cnt + c.items - 1, 0, sizeof(int), (hipStream_t)stream) != hipSuccess) return MOPA_ERR_LAUNCH;
  return mopa_scan_exclusive_i32(c.cnt, c.scan, c.items, c.total, c.sws, c.sws_bytes, stream);
}
