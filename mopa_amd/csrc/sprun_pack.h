// Shared by sprun.hip and spconv.hip (the batched weight-form refresh): the weight layout of k_spconv_run.
#pragma once
#include <stdint.h>
// Weights for k_spconv_run: per (offset, column group of NT 16-column tiles) one contiguous slice in LDS-image order,
//   wr[o][cg][kc][t][lane][s] = Wc[o][16 kc + 4 (lane >> 4) + s][(cg NT + t) 16 + (lane & 15)]
// (Wc = w [K][cin][cout], or its per-offset transpose for backward-data): a lane's MFMA operand of (chunk kc, tile t) is one
// conflict-free ds_read_b128 at (kc NT + t) 1024 + 16 lane, and staging a slice is a straight copy.
__device__ __forceinline__ void run_pack_elem(const float* __restrict__ w, float* __restrict__ wr, int i, int K, int cin_w, int cout_w,
                                              int transpose, int nt) {
  const int cin_c = transpose ? cout_w : cin_w, cout_c = transpose ? cin_w : cout_w;
  const int nkc = cin_c >> 4, ncg = (cout_c >> 4) / nt;
  int rem = i;
  const int s = rem & 3; rem >>= 2;
  const int lane = rem & 63; rem >>= 6;
  const int t = rem % nt; rem /= nt;
  const int kc = rem % nkc; rem /= nkc;
  const int cg = rem % ncg;
  const int o = rem / ncg;
  const int k = kc * 16 + (lane >> 4) * 4 + s, c = (cg * nt + t) * 16 + (lane & 15);
  wr[i] = transpose ? w[((int64_t)o * cin_w + c) * cout_w + k] : w[((int64_t)o * cin_w + k) * cout_w + c];
}
// Column-group width (16-column tiles per block) of the run kernel for cout output channels: all of them up to 7 tiles,
// else the largest divisor <= 7 (128 -> 4, 160 -> 5, 192 -> 6, 224 -> 7, 144 -> 3).  0 = shape not supported.
static inline int run_nt(int cin, int cout) {
  if (cin % 16 || cout % 16 || cin < 16 || cin > 224 || cout < 16 || cout > 224) return 0;
  const int tiles = cout / 16;
  if (tiles <= 7) return tiles;
  for (int c = 7; c >= 2; --c)
    if (tiles % c == 0) return c;
  return 0;
}

// ---- which kernel a forward launch runs (mopa_spconv_fwd, mopa_spconv_fwd_grouped, mopa_spconv_fwd_run), as ONE value: each entry
// point computes it in one host function (pick_fwd / pick_grouped / pick_run), its launcher is a switch over it, and
// mopa_spconv_fwd_kernel returns it to a caller that only asks.  Fields:
//   bits 0-3   family (SPK_*)
//   bits 4-7   NTW: 16-column tiles per column group (k_spconv_run: NT; k_spconv_stem: CIN)
//   bits 8-11  NA (k_spconv_fwd, k_spconv_blk), NKU (k_spconv_t4), COUT / 16 (k_spconv_stem)
//   bits 12-15 D: depth of the load ring (k_spconv_pipe, k_spconv_t4)
//   bits 16-18 NWV: waves per tile (k_spconv_t4)
//   bit  19    ALIGNED (k_spconv_fwd, k_spconv_blk), PART (k_spconv_t4), SCATTER (k_spconv_run)
//   bits 20-23 osplit (k_spconv_blk: blocks over the filter offsets, 1 = no partial copies)
//   bits 24-25 RG (k_spconv_run)
enum { SPK_STEM = 1, SPK_FWD = 2, SPK_BLK = 3, SPK_PIPE = 4, SPK_T4 = 5, SPK_RUN = 6, SPK_RING = 7 };
#define SPK(fam, ntw, nk, d, nwv) ((fam) | (ntw) << 4 | (nk) << 8 | (d) << 12 | (nwv) << 16)
#define SPK_KERNEL(p) ((p) & 0x7ffff)        // what the launcher switches over: the template arguments that are not a bool
#define SPK_FAMILY(p) ((p) & 15)
#define SPK_NTW(p) (((p) >> 4) & 15)
#define SPK_FLAG (1 << 19)
#define SPK_OSPLIT(p) (((p) >> 20) & 15)
#define SPK_RG(p) (((p) >> 24) & 3)
// w_flip of the three entry points: bit 0 mirrored offsets, bit 1 packed weights (grouped call), bits 8-30 "decide as if the table
// had this many 64-row tiles" (0: the real row count).  The kernel runs on the real table; only the choice above uses the stated size.
static inline int64_t spk_stated_rows(int w_flip, int64_t num_out) {
  const int64_t tiles = (w_flip >> 8) & 0x7fffff;
  return tiles ? tiles * 64 : num_out;
}
// Which k_spconv_run mopa_spconv_fwd_run launches on a table of `rows` rows (-1: shape not supported).  Items of 128 slots (two row
// groups per wave) unless the table is so short that they would leave CUs idle: the rule count is not known on the host (no
// synchronisation), ~9 rules per row on the deep 27-offset tables, rows_in <= 8 rows_out otherwise.
static inline int spk_pick_run(int K, int64_t rows, int cin, int cout, int one_rule_per_row) {
  const int nt = run_nt(cin, cout);
  if (nt == 0) return -1;
  const int64_t rules_est = K == 27 ? 9 * rows : one_rule_per_row ? rows : 5 * rows / 2;
  const int rg = rules_est / 128 < 1024 ? 1 : 2;   // (fewer than ~4 items of 128 per CU: level 5 at 8 scans 27 -> 17 us with 64-slot items)
  return SPK(SPK_RUN, nt, 0, 0, 0) | (one_rule_per_row ? SPK_FLAG : 0) | rg << 24;
}

// ---- which kernel a weight-gradient launch runs (mopa_spconv_bwd_weight, mopa_spconv_bwd_weight_run), as ONE value: each entry point
// computes it in one host function (pick_wgrad in spconv.hip / wgr_pick in sprun.hip) together with everything else of the launch
// (chunks or pieces, workspace bytes, LDS bytes), launches through a switch over it, and mopa_spconv_wgrad_kernel returns it to a
// caller that only asks.  Fields:
//   bits 0-3   family (WGK_*)
//   bits 4-7   MU: 16-channel blocks of Cin per wave (0: k_spconv_stem_wgrad)
//   bits 8-11  NT: 16-column tiles of Cout
//   bits 12-15 D: depth of the load ring (k_spconv_wgrad2)
//   bits 16-18 NWV: waves per (offset, chunk) (k_spconv_wgrad2)
enum { WGK_STEM = 1, WGK_SIMPLE = 2, WGK_PIPE = 3, WGK_RUN = 4 };
#define WGK(fam, mu, nt, d, nwv) ((fam) | (mu) << 4 | (nt) << 8 | (d) << 12 | (nwv) << 16)
// `accumulate` of the two entry points: bit 0 add to dweight, bits 8-30 "decide as if the table had this many 64-row tiles" (0: the
// real row count) -- the convention of w_flip above (spk_stated_rows reads both).  The stated size moves the decisions that follow
// the table's size alone (the wave target and the four-waves-per-block form of k_spconv_wgrad2, the piece size of k_wgrad_run); every
// clamp and check (rows per chunk, slab caps, the bound on the slots, 32-bit row offsets, the workspace) stays on the real table.
// What mopa_spconv_wgrad_kernel writes to its host array (int64): the plan behind the value above.
enum { WGI_CHUNKS = 0, WGI_ROWS_PER_CHUNK = 1, WGI_S = 2, WGI_PIECES = 3, WGI_WS_BYTES = 4, WGI_LDS_BYTES = 5, WGI_BLOCKS = 6, WGI_N = 8 };
// (sprun.hip) the run entry's decision for spconv.hip's query: the value above or the entry's error code; ptr_low as in the query
int mopa_wgr_pick_for_query(int K, int64_t num_out, int64_t stated, int cin, int cout, int one_rule_per_row, int ld_in, int ld_dout,
                            unsigned ptr_low, int64_t* info);
