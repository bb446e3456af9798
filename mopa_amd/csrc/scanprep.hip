// The 3D half of the input pipeline on the device: for the B scans of an iteration (plus, for the EMA teacher, their
// un-augmented copies as B more segments) rotation, voxel coordinates, the in-field filter, ONE stable compaction of every
// per-point array and the per-scan median refinement of the loaded pseudo labels -- what Dataset.__getitem__ +
// collate_scn_base do per sample on the host (mopa/data/nuscenes/nuscenes_dataloader.py:339-340,410-465,
// mopa/data/semantic_kitti/semantic_kitti_dataloader.py:583-585,632-676, mopa/data/collate.py:182-264,
// mopa/data/utils/augmentation_3d.py:48-59, mopa/data/utils/refine_pseudo_labels.py:5-22).
//
// A fixed number of launches whatever B is: every kernel covers all segments of the call, cut into blocks of SP_ROWS rows
// (segbatch.h: the block table, the counts and their scan).  Per-segment pointers and draws travel as kernel arguments (at most
// SP_MAXS segments per call; the binding splits larger batches).  The arithmetic is k_vox_minmax / k_vox_coords / k_rotate_f32 of hash3d.hip, restated per segment: same bits.
// The rotated points are written once and read by every later pass.  No float atomics: min / max go through integer
// atomics on the ordered bit pattern, counts and histograms are integers, the compaction is ordered -> deterministic.
#include "common.h"
#include "segbatch.h"

#define SP_MAXS 64             // segments per call: 32 scans, each with an optional un-augmented copy
#define SP_MAXB 32             // scans per call
#define SP_ROWS 1024           // rows per block (256 threads x 4 tiles)
#define SP_MAXC 32             // classes of the refinement (pseudo.hip PS_MAXC)

struct SpSeg {
  const float* src[SP_MAXS];        // (n, 3) float32: the rotated points (or the points as loaded)
  const uint8_t* keep_in[SP_MAXS];  // (n,) 0/1 or null: rows removed before the minimum is taken
  SegTable<SP_MAXS> seg;
};
struct SpTr {
  double u[SP_MAXB][3];             // the translation's rand(3) draws (scans only; copies are never translated)
  uint8_t on[SP_MAXB];
};
struct SpRot {
  const float* src[SP_MAXB];
  float* dst[SP_MAXB];
  SegTable<SP_MAXB> seg;
  float r[SP_MAXB][9];
};
struct SpSide {
  const void* label[SP_MAXB];       // (n,) raw class ids or null
  const int64_t* img[SP_MAXB];      // (n, 2) or null
  const float* src[SP_MAXB];        // (n, 3) rotated points
  SegTable<SP_MAXB> seg;
};

__device__ __forceinline__ int sp_f2ord(float f) { int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7FFFFFFF; }
__device__ __forceinline__ float sp_ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7FFFFFFF); }
__device__ __forceinline__ int64_t sp_label(const void* p, int dtype, int64_t i) {
  switch (dtype) {
    case 0: return ((const uint8_t*)p)[i];
    case 1: return ((const int16_t*)p)[i];
    case 2: return ((const int32_t*)p)[i];
    default: return ((const int64_t*)p)[i];
  }
}

// ------------------------------------------------------------------------------------------ 1. rotation
// out = points @ R per scan, float32 as fma(z, r2j, fma(y, r1j, x * r0j)) (k_rotate_f32).
__global__ __launch_bounds__(256) void k_sp_rotate(const SpRot a, int S) {
  const int s = seg_of_block(a.seg.blk0, S, blockIdx.x);
  const int n = a.seg.n[s];
  const float* __restrict__ p = a.src[s];
  float* __restrict__ o = a.dst[s];
  float r[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) r[k] = a.r[s][k];
  const int base = (blockIdx.x - a.seg.blk0[s]) * SP_ROWS;
#pragma unroll
  for (int t = 0; t < SP_ROWS / 256; ++t) {
    const int i = base + t * 256 + threadIdx.x;
    if (i >= n) break;
    const float x = p[3 * (int64_t)i], y = p[3 * (int64_t)i + 1], z = p[3 * (int64_t)i + 2];
    o[3 * (int64_t)i] = fmaf(z, r[6], fmaf(y, r[3], __fmul_rn(x, r[0])));
    o[3 * (int64_t)i + 1] = fmaf(z, r[7], fmaf(y, r[4], __fmul_rn(x, r[1])));
    o[3 * (int64_t)i + 2] = fmaf(z, r[8], fmaf(y, r[5], __fmul_rn(x, r[2])));
  }
}

// ------------------------------------------------------------------------------------------ 2. min / max
__global__ void k_sp_init(int* __restrict__ mm, int S) {
  for (int i = threadIdx.x; i < S * 6; i += blockDim.x) mm[i] = (i % 6) < 3 ? 0x7FFFFFFF : (int)0x80000000;
}
__global__ __launch_bounds__(256) void k_sp_minmax(const SpSeg a, int S, float scale, int* __restrict__ mm) {
  __shared__ int red[4][6];
  const int s = seg_of_block(a.seg.blk0, S, blockIdx.x);
  const int n = a.seg.n[s];
  const float* __restrict__ p = a.src[s];
  const uint8_t* __restrict__ kin = a.keep_in[s];
  const int base = (blockIdx.x - a.seg.blk0[s]) * SP_ROWS;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int t = 0; t < SP_ROWS / 256; ++t) {
    const int i = base + t * 256 + threadIdx.x;
    if (i < n && (!kin || kin[i])) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float r = rintf(p[3 * (int64_t)i + c] * scale);
        lo[c] = fminf(lo[c], r);
        hi[c] = fmaxf(hi[c], r);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    for (int o = 32; o > 0; o >>= 1) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], o, 64));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o, 64));
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][c] = sp_f2ord(lo[c]); red[threadIdx.x >> 6][3 + c] = sp_f2ord(hi[c]); }
  }
  __syncthreads();
  if (threadIdx.x < 6) {  // min / max do not depend on arrival order: integer atomics on the ordered bit pattern
    const int c = threadIdx.x;
    int v = red[0][c];
    for (int w = 1; w < 4; ++w) v = c < 3 ? min(v, red[w][c]) : max(v, red[w][c]);
    if (c < 3) { if (v != 0x7FFFFFFF) atomicMin(&mm[s * 6 + c], v); }
    else if (v != (int)0x80000000) atomicMax(&mm[s * 6 + c], v);
  }
}

// coordinates of one row (k_vox_coords): c = rint(p * scale) - min; with translation float32(double(c) + off)
struct SpField { float mn[3]; double off[3]; bool transl; };
__device__ __forceinline__ SpField sp_field(const int* __restrict__ mm, int s, int B, const SpTr& tr, int full_scale) {
  SpField f;
  f.transl = s < B && tr.on[s];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f.mn[c] = sp_ord2f(mm[s * 6 + c]);
    const float mx = sp_ord2f(mm[s * 6 + 3 + c]) - f.mn[c];
    float t = (float)full_scale - mx;
    t = t - 0.001f;
    t = fmaxf(t, 0.f);
    f.off[c] = f.transl ? (double)t * tr.u[s < B ? s : 0][c] : 0.0;
  }
  return f;
}
__device__ __forceinline__ bool sp_coords(const float* __restrict__ p, int64_t i, float scale, int full_scale, const SpField& f, int64_t* ci) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = rintf(p[3 * i + c] * scale) - f.mn[c];
    if (f.transl) v = (float)((double)v + f.off[c]);
    ci[c] = (int64_t)v;
    ok = ok && ci[c] >= 0 && ci[c] < full_scale;
  }
  return ok;
}

// ------------------------------------------------------------------------------------------ 3. keep flags + block counts
// flags[row] bit 0 = the row is emitted (survives keep_in and lies inside the field), bit 1 = it survives a keep_in that is given
// (without keep_in the byte is 0 / 1: the reference's idxs as it stands).
// cnt[blk] = emitted rows of the block, cnt[nblk + blk] = rows of the block that survive keep_in.
__global__ __launch_bounds__(256) void k_sp_flags(const SpSeg a, const SpTr tr, int S, int B, float scale, int full_scale,
                                                  const int* __restrict__ mm, uint8_t* __restrict__ flags, int* __restrict__ cnt, int nblk) {
  const int s = seg_of_block(a.seg.blk0, S, blockIdx.x);
  const int n = a.seg.n[s];
  const float* __restrict__ p = a.src[s];
  const uint8_t* __restrict__ kin = a.keep_in[s];
  const SpField f = sp_field(mm, s, B, tr, full_scale);
  const int base = (blockIdx.x - a.seg.blk0[s]) * SP_ROWS;
  int c[2] = {0, 0};                // emitted rows, rows that survive keep_in
#pragma unroll
  for (int t = 0; t < SP_ROWS / 256; ++t) {
    const int i = base + t * 256 + threadIdx.x;
    if (i < n) {
      const bool k1 = !kin || kin[i];
      bool ok = false;
      if (k1) { int64_t ci[3]; ok = sp_coords(p, i, scale, full_scale, f, ci); }
      flags[(int64_t)a.seg.row0[s] + i] = (uint8_t)((ok ? 1 : 0) | ((kin && k1) ? 2 : 0));
      c[0] += ok;
      c[1] += k1;
    }
  }
  block_counts(c, cnt, nblk);
}
// offsets[s] = first output row of segment s (s <= S; the copies count from offsets[B] on), offsets[S + 1 + b] = first row of
// scan b among the rows that survive keep_in (b <= B).  scan = exclusive scan of cnt.
__global__ void k_sp_offsets(const SpSeg a, int S, int B, const int* __restrict__ scan, int nblk, int64_t* __restrict__ offsets) {
  const int i = threadIdx.x;   // blk0[S] = nblk, and the scan has one item more than counts: scan[2 nblk] is the grand total
  if (i <= S) offsets[i] = scan[a.seg.blk0[i]];
  if (i <= B) offsets[S + 1 + i] = scan[nblk + a.seg.blk0[i]] - scan[nblk];
}

// ------------------------------------------------------------------------------------------ 4. compaction
struct __attribute__((aligned(32))) SpLoc { int64_t x, y, z, b; };
// identity != 0 (nothing is removed): row i of segment s goes to row0[s] + i, rows outside the field are counted in n_outside.
// Otherwise the rows with flag bit 0 go, in order, to scan[blk] + rank; rows with bit 1 write their bit 0 to mask1 (the
// reference's idxs of a cropped scan) and their point index to gather1.  locs / gather receive the scans, ori_locs the copies (segments >= B).
__global__ __launch_bounds__(256) void k_sp_compact(const SpSeg a, const SpTr tr, int S, int B, int batch0, float scale, int full_scale,
                                                    int identity, const int* __restrict__ mm, const uint8_t* __restrict__ flags,
                                                    const int* __restrict__ scan, int nblk, SpLoc* __restrict__ locs,
                                                    SpLoc* __restrict__ ori_locs, int64_t* __restrict__ gather, int64_t gather_base,
                                                    uint8_t* __restrict__ mask1, int64_t* __restrict__ gather1, int* __restrict__ n_outside) {
  __shared__ int lds[4];
  const int s = seg_of_block(a.seg.blk0, S, blockIdx.x);
  const int n = a.seg.n[s];
  const float* __restrict__ p = a.src[s];
  const SpField f = sp_field(mm, s, B, tr, full_scale);
  const int base = (blockIdx.x - a.seg.blk0[s]) * SP_ROWS;
  const bool copy = s >= B;
  SpLoc* __restrict__ dst = copy ? ori_locs : locs;
  int64_t run2, run1 = 0;
  if (identity) {
    run2 = (int64_t)a.seg.row0[s] - (copy ? a.seg.row0[B] : 0) + base;
  } else {
    run2 = (int64_t)scan[blockIdx.x] - (copy ? scan[a.seg.blk0[B]] : 0);
    run1 = (int64_t)scan[nblk + blockIdx.x] - scan[nblk];
  }
  int outside = 0;
#pragma unroll
  for (int t = 0; t < SP_ROWS / 256; ++t) {
    const int i = base + t * 256 + threadIdx.x;
    const bool valid = i < n;
    if (identity) {
      if (valid) {
        int64_t ci[3];
        outside += !sp_coords(p, i, scale, full_scale, f, ci);
        const int64_t o = run2 + t * 256 + threadIdx.x;
        dst[o] = SpLoc{ci[0], ci[1], ci[2], (int64_t)(batch0 + (copy ? s - B : s))};
        if (!copy) gather[o] = gather_base + a.seg.row0[s] + i;
      }
      continue;
    }
    const uint8_t fl = valid ? flags[(int64_t)a.seg.row0[s] + i] : 0;
    int tot2, tot1 = 0;
    const int r2 = block_rank<256>(fl & 1, lds, tot2);
    if (fl & 1) {
      int64_t ci[3];
      sp_coords(p, i, scale, full_scale, f, ci);
      dst[run2 + r2] = SpLoc{ci[0], ci[1], ci[2], (int64_t)(batch0 + (copy ? s - B : s))};
      if (!copy) gather[run2 + r2] = gather_base + a.seg.row0[s] + i;
    }
    run2 += tot2;
    if (mask1 && !copy) {
      const bool k1 = valid && (a.keep_in[s] ? (fl & 2) != 0 : true);
      const int r1 = block_rank<256>(k1, lds, tot1);
      if (k1) { mask1[run1 + r1] = fl & 1; gather1[run1 + r1] = gather_base + a.seg.row0[s] + i; }
      run1 += tot1;
    }
  }
  if (identity) {
    outside = wave_sum_i(outside);
    if ((threadIdx.x & 63) == 0 && outside) atomicAdd(n_outside, outside);
  }
}

// ------------------------------------------------------------------------------------------ 5. side arrays through the gather
// out row m takes point g = gather[m] - gather_base (m itself when gather is null) of the call's flat numbering.
struct __attribute__((aligned(16))) SpPair { int64_t r, c; };
__global__ __launch_bounds__(256) void k_sp_take(const SpSide a, int B, const int64_t* __restrict__ gather, int64_t gather_base, int64_t M,
                                                 int label_dtype, const int64_t* __restrict__ label_map, int64_t map_len, int64_t ignore,
                                                 const int64_t* __restrict__ ps2, const int64_t* __restrict__ ps3,
                                                 int64_t* __restrict__ label_out, SpPair* __restrict__ img_out, float* __restrict__ pts_out,
                                                 int64_t* __restrict__ ps2_out, int64_t* __restrict__ ps3_out) {
  __shared__ int row0[SP_MAXB + 1];
  if (threadIdx.x <= B) row0[threadIdx.x] = a.seg.row0[threadIdx.x];
  __syncthreads();
  for (int64_t m = blockIdx.x * (int64_t)256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const int64_t g = gather ? gather[m] - gather_base : m;
    int lo = 0, hi = B - 1;               // the scan that holds row g: row0[b] <= g < row0[b + 1] (empty scans are skipped)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (row0[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const int64_t i = g - row0[lo];
    if (label_out) {
      int64_t v = sp_label(a.label[lo], label_dtype, i);
      if (label_map) v = (v >= 0 && v < map_len) ? label_map[v] : ignore;
      label_out[m] = v;
    }
    if (img_out) img_out[m] = reinterpret_cast<const SpPair*>(a.img[lo])[i];
    if (pts_out) {
      const float* __restrict__ p = a.src[lo] + 3 * i;
      pts_out[3 * m] = p[0]; pts_out[3 * m + 1] = p[1]; pts_out[3 * m + 2] = p[2];
    }
    if (ps2_out) ps2_out[m] = ps2[g];
    if (ps3_out) ps3_out[m] = ps3[g];
  }
}

MOPA_API int mopa_scanprep_rotate(const void* const* src_host, void* const* dst_host, const int32_t* n_host, const float* rot_host /*[S][9]*/,
                                  int32_t S, void* stream) {
  SpRot a = {};
  const int nblk = seg_table_fill(a.seg, n_host, S, SP_ROWS);
  if (nblk < 0 || !src_host || !dst_host || !rot_host) return MOPA_ERR_ARG;
  for (int s = 0; s < S; ++s) {
    if (n_host[s] > 0 && (!src_host[s] || !dst_host[s])) return MOPA_ERR_ARG;
    a.src[s] = (const float*)src_host[s];
    a.dst[s] = (float*)dst_host[s];
    for (int k = 0; k < 9; ++k) a.r[s][k] = rot_host[s * 9 + k];
  }
  if (nblk == 0) return MOPA_OK;
  k_sp_rotate<<<nblk, 256, 0, (hipStream_t)stream>>>(a, S);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// workspace: mm [SP_MAXS][6], then the two count planes (emitted, surviving keep_in) of segbatch.h's SegCounts
MOPA_API size_t mopa_scanprep_workspace_bytes(int64_t total_blocks) {
  if (total_blocks < 0) return 0;
  return seg_counts_bytes(2, total_blocks, SP_MAXS * 6);
}
MOPA_API int mopa_scanprep_rows_per_block(void) { return SP_ROWS; }

static int sp_fill(SpSeg& a, SpTr& tr, const void* const* src_host, const void* const* keep_in_host, const int32_t* n_host,
                   const double* u_host, const int32_t* transl_host, int S, int B) {
  if (!src_host || B < 1 || B > SP_MAXB || (S != B && S != 2 * B)) return -1;
  const int nblk = seg_table_fill(a.seg, n_host, S, SP_ROWS);
  if (nblk < 0) return -1;
  for (int s = 0; s < S; ++s) {
    if (n_host[s] > 0 && !src_host[s]) return -1;
    a.src[s] = (const float*)src_host[s];
    a.keep_in[s] = keep_in_host ? (const uint8_t*)keep_in_host[s] : nullptr;
  }
  for (int b = 0; b < B; ++b) {
    tr.on[b] = transl_host && transl_host[b];
    if (tr.on[b] && !u_host) return -1;
    for (int c = 0; c < 3; ++c) tr.u[b][c] = tr.on[b] ? u_host[3 * b + c] : 0.0;
  }
  return nblk;
}

// Stages 2 + 3 for S segments (the B scans first, then -- S == 2 B -- their un-augmented copies): per-segment min / max into the
// workspace; with count != 0 also flags (sum n bytes), the ordered scan of the per-block counts and offsets (S + 1 + B + 1 int64,
// see k_sp_offsets), which the caller reads back to size the outputs.  The workspace carries min / max and the scan to
// mopa_scanprep_compact and must not be touched in between.
MOPA_API int mopa_scanprep_count(const void* const* src_host, const void* const* keep_in_host, const int32_t* n_host, const double* u_host,
                                 const int32_t* transl_host, int32_t S, int32_t B, float scale, int32_t full_scale, int32_t count,
                                 uint8_t* flags, int64_t* offsets, void* ws, size_t ws_bytes, void* stream) {
  SpSeg a = {};
  SpTr tr = {};
  const int nblk = sp_fill(a, tr, src_host, keep_in_host, n_host, u_host, transl_host, S, B);
  if (nblk < 0 || full_scale <= 0 || !ws || (count && (!flags || !offsets))) return MOPA_ERR_ARG;
  if (ws_bytes < mopa_scanprep_workspace_bytes(nblk)) return MOPA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int* mm = (int*)ws;
  const SegCounts c = seg_counts(ws, 2, nblk, SP_MAXS * 6);
  k_sp_init<<<1, 256, 0, st>>>(mm, S);
  if (nblk > 0) k_sp_minmax<<<nblk, 256, 0, st>>>(a, S, scale, mm);
  if (count) {
    if (nblk > 0) k_sp_flags<<<nblk, 256, 0, st>>>(a, tr, S, B, scale, full_scale, mm, flags, c.cnt, nblk);
    const int rc = seg_counts_scan(c, stream);
    if (rc) return rc;
    k_sp_offsets<<<1, 128, 0, st>>>(a, S, B, c.scan, nblk, offsets);
  }
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// Stage 4.  identity != 0: nothing is removed (flags may be null).  locs / gather point at the first row of this call's scans,
// ori_locs at the first row of its copies; gather values are gather_base + the point's row in this call's flat numbering.
MOPA_API int mopa_scanprep_compact(const void* const* src_host, const void* const* keep_in_host, const int32_t* n_host, const double* u_host,
                                   const int32_t* transl_host, int32_t S, int32_t B, int32_t batch0, float scale, int32_t full_scale,
                                   int32_t identity, const uint8_t* flags, int64_t* locs, int64_t* ori_locs, int64_t* gather,
                                   int64_t gather_base, uint8_t* mask1, int64_t* gather1, int32_t* n_outside, void* ws, size_t ws_bytes, void* stream) {
  SpSeg a = {};
  SpTr tr = {};
  const int nblk = sp_fill(a, tr, src_host, keep_in_host, n_host, u_host, transl_host, S, B);
  if (nblk < 0 || full_scale <= 0 || !ws || !locs || !gather || (S > B && !ori_locs) || (identity ? !n_outside : !flags) || batch0 < 0 ||
      (mask1 && !gather1))
    return MOPA_ERR_ARG;
  if ((((uintptr_t)locs | (uintptr_t)ori_locs) & 31)) return MOPA_ERR_ARG;
  if (ws_bytes < mopa_scanprep_workspace_bytes(nblk)) return MOPA_ERR_WORKSPACE;
  if (nblk == 0) return MOPA_OK;
  const int* mm = (const int*)ws;
  const int* scan = seg_counts(ws, 2, nblk, SP_MAXS * 6).scan;
  k_sp_compact<<<nblk, 256, 0, (hipStream_t)stream>>>(a, tr, S, B, batch0, scale, full_scale, identity, mm, flags, scan, nblk, (SpLoc*)locs,
                                                      (SpLoc*)ori_locs, gather, gather_base, mask1, gather1, n_outside);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// Stage 5: every per-point side array of the B scans through one gather (null: all rows in order, M = sum n).  label_dtype:
// 0 uint8, 1 int16, 2 int32, 3 int64; label_map (map_len entries) or null; ids outside the table give `ignore`.  ps2 / ps3:
// flat (sum n) int64 arrays in the call's row numbering.  Outputs that are null are not produced.
MOPA_API int mopa_scanprep_take(const int64_t* gather, int64_t gather_base, int64_t M, const int32_t* n_host, int32_t B,
                                const void* const* label_host, int32_t label_dtype, const int64_t* label_map, int64_t map_len,
                                int64_t ignore_label, const void* const* img_host, const void* const* src_host, const int64_t* ps2,
                                const int64_t* ps3, int64_t* label_out, int64_t* img_out, float* pts_out, int64_t* ps2_out,
                                int64_t* ps3_out, void* stream) {
  if (M < 0 || label_dtype < 0 || label_dtype > 3 || (label_map && map_len <= 0)) return MOPA_ERR_ARG;
  if ((label_out && !label_host) || (img_out && !img_host) || (pts_out && !src_host) || (ps2_out && !ps2) || (ps3_out && !ps3))
    return MOPA_ERR_ARG;
  if (((uintptr_t)img_out & 15)) return MOPA_ERR_ARG;
  SpSide a = {};
  if (seg_table_fill(a.seg, n_host, B, SP_ROWS) < 0) return MOPA_ERR_ARG;
  if (!gather && M != a.seg.row0[B]) return MOPA_ERR_ARG;
  for (int b = 0; b < B; ++b) {
    a.label[b] = label_host ? label_host[b] : nullptr;
    a.img[b] = img_host ? (const int64_t*)img_host[b] : nullptr;
    a.src[b] = src_host ? (const float*)src_host[b] : nullptr;
    if (n_host[b] > 0 && ((label_out && !a.label[b]) || (img_out && (!a.img[b] || ((uintptr_t)a.img[b] & 15))) || (pts_out && !a.src[b])))
      return MOPA_ERR_ARG;
  }
  if (M == 0) return MOPA_OK;
  k_sp_take<<<stream_grid(M, 256), 256, 0, (hipStream_t)stream>>>(a, B, gather, gather_base, M, label_dtype, label_map, map_len, ignore_label,
                                                                  ps2, ps3, label_out, (SpPair*)img_out, pts_out, ps2_out, ps3_out);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}

// ------------------------------------------------------------------------------------------ segmented pseudo-label refinement
// mopa_refine_pseudo_labels (pseudo.hip) for S independent segments in one set of launches: per segment and class the exact
// lower median sorted[(n - 1) / 2] by a four-pass 8-bit radix select, threshold min(median, 0.9).  state [S][3 C], hist [S][C][256].
struct SrSeg {
  const float* prob[SP_MAXS];     // null: the labels pass through unrefined (cast to int64)
  const void* label[SP_MAXS];
  int64_t* out[SP_MAXS];
  int32_t n[SP_MAXS];
};
#define SR_BLOCKS 64              // blocks per segment of the histogram pass
__global__ __launch_bounds__(256) void k_sr_hist(const SrSeg a, int dtype, int C, int pass, const unsigned* __restrict__ state,
                                                 unsigned* __restrict__ hist) {
  extern __shared__ unsigned lh[];  // [C][256]
  const int s = blockIdx.y;
  const int n = a.n[s];
  const float* __restrict__ prob = a.prob[s];
  if (!prob || (int64_t)blockIdx.x * 256 >= n) return;
  const void* label = a.label[s];
  const unsigned* st = state + (size_t)s * 3 * C;
  for (int i = threadIdx.x; i < C * 256; i += 256) lh[i] = 0;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int64_t c = sp_label(label, dtype, i);
    if (c < 0 || c >= C) continue;
    const unsigned bits = __float_as_uint(prob[i]);
    if ((bits & himask) == (st[c] & himask)) atomicAdd(&lh[c * 256 + ((bits >> shift) & 255u)], 1u);
  }
  __syncthreads();
  unsigned* h = hist + (size_t)s * C * 256;
  for (int i = threadIdx.x; i < C * 256; i += 256)
    if (lh[i]) atomicAdd(&h[i], lh[i]);
}
// one wave per (class, segment): k_ps_select
__global__ __launch_bounds__(64) void k_sr_select(int C, int pass, unsigned* __restrict__ state_all, unsigned* __restrict__ hist_all) {
  const int c = blockIdx.x, lane = threadIdx.x;
  unsigned* state = state_all + (size_t)blockIdx.y * 3 * C;
  unsigned* hist = hist_all + (size_t)blockIdx.y * C * 256;
  unsigned h[4], tot = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { h[j] = hist[c * 256 + lane * 4 + j]; tot += h[j]; }
  unsigned incl = tot;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  const unsigned n = __shfl(incl, 63, 64);
  unsigned k;
  if (pass == 0) {
    k = n ? (n - 1) / 2 : 0;
    if (lane == 0) state[2 * C + c] = n;
  } else {
    k = state[C + c];
  }
  const unsigned excl = incl - tot;
  const bool mine = n > 0 && k >= excl && k < incl;
  if (mine) {
    unsigned run = excl;
    int b = 3;
    bool found = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!found) {
        if (k < run + h[j]) { found = true; b = j; }
        else run += h[j];
      }
    }
    const int shift = 24 - 8 * pass;
    state[c] = (pass == 0 ? 0u : state[c]) | ((unsigned)(lane * 4 + b) << shift);
    state[C + c] = k - run;
  }
  if (n == 0 && lane == 0 && pass == 0) { state[c] = 0; state[C + c] = 0; }
#pragma unroll
  for (int j = 0; j < 4; ++j) hist[c * 256 + lane * 4 + j] = 0;
}
__global__ __launch_bounds__(256) void k_sr_apply(const SrSeg a, int dtype, int C, const unsigned* __restrict__ state, int64_t ignore) {
  const int s = blockIdx.y;
  const int n = a.n[s];
  const float* __restrict__ prob = a.prob[s];
  const void* label = a.label[s];
  int64_t* __restrict__ out = a.out[s];
  const unsigned* st = state + (size_t)s * 3 * C;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int64_t c = sp_label(label, dtype, i);
    int64_t o = c;
    if (prob && c >= 0 && c < C) {
      const float thresh = fminf(__uint_as_float(st[c]), 0.9f);
      if (prob[i] < thresh) o = ignore;
    }
    out[i] = o;
  }
}

MOPA_API size_t mopa_refine_pseudo_labels_segmented_workspace_bytes(int32_t S, int32_t C) {
  if (S < 1 || C < 1) return 0;
  return align_up((size_t)S * (3 * C + C * 256) * sizeof(unsigned), 256);
}

// S segments: prob_host[s] (n_s) fp32 >= 0 or null (no refinement: the labels are only cast), label_host[s] (n_s) integers of
// label_dtype (0 uint8, 1 int16, 2 int32, 3 int64), out_host[s] (n_s) int64.  Equal to S calls of mopa_refine_pseudo_labels.
MOPA_API int mopa_refine_pseudo_labels_segmented(const void* const* prob_host, const void* const* label_host, int32_t label_dtype,
                                                 const int32_t* n_host, void* const* out_host, int32_t S, int32_t C, int64_t ignore_label,
                                                 void* ws, size_t ws_bytes, void* stream) {
  if (!label_host || !n_host || !out_host || S < 1 || S > SP_MAXS || C <= 0 || C > SP_MAXC || label_dtype < 0 || label_dtype > 3 || !ws)
    return MOPA_ERR_ARG;
  if (ws_bytes < mopa_refine_pseudo_labels_segmented_workspace_bytes(S, C)) return MOPA_ERR_WORKSPACE;
  SrSeg a = {};
  int nmax = 0;
  bool any = false;
  for (int s = 0; s < S; ++s) {
    if (n_host[s] < 0 || (n_host[s] > 0 && (!label_host[s] || !out_host[s]))) return MOPA_ERR_ARG;
    a.prob[s] = prob_host ? (const float*)prob_host[s] : nullptr;
    a.label[s] = label_host[s];
    a.out[s] = (int64_t*)out_host[s];
    a.n[s] = n_host[s];
    nmax = n_host[s] > nmax ? n_host[s] : nmax;
    any = any || (a.prob[s] && n_host[s] > 0);
  }
  if (nmax == 0) return MOPA_OK;
  hipStream_t st = (hipStream_t)stream;
  unsigned* state = (unsigned*)ws;
  unsigned* hist = state + (size_t)S * 3 * C;
  const int gx = (int)(cdiv64(nmax, 256) < SR_BLOCKS ? cdiv64(nmax, 256) : SR_BLOCKS);
  if (any) {
    if (hipMemsetAsync(ws, 0, (size_t)S * (3 * C + C * 256) * sizeof(unsigned), st) != hipSuccess) return MOPA_ERR_LAUNCH;
    for (int pass = 0; pass < 4; ++pass) {
      k_sr_hist<<<dim3(gx, S), 256, (size_t)C * 256 * sizeof(unsigned), st>>>(a, label_dtype, C, pass, state, hist);
      k_sr_select<<<dim3(C, S), 64, 0, st>>>(C, pass, state, hist);
    }
  }
  k_sr_apply<<<dim3(gx, S), 256, 0, st>>>(a, label_dtype, C, state, ignore_label);
  MOPA_CHECK_LAUNCH();
  return MOPA_OK;
}
