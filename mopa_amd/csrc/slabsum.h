// The ordered slab sums of the split-K weight gradients: the ONE place where their summation order is written down.
//
// A weight-gradient GEMM writes one partial result ("slab") per split into the workspace; a reduction kernel adds the slabs in a
// fixed order into the parameter gradient.  The order is part of the library's results (training is bit-reproducible, and the
// "same bits as ..." tests compare entry points that share it; tests/test_gpu_slab_sums.py restates it in numpy), so a change here
// changes every weight gradient at once -- and must keep all of the following:
//
//  1. slab_lane_sums<EW>: a block is 256 threads = EW consecutive elements x NL = 256 / EW slab lanes, thread = (el, cl) =
//     (threadIdx.x % EW, threadIdx.x / EW).  Thread (el, cl) adds slabs cl, cl + NL, cl + 2 NL, ... of its element in ascending
//     order, starting from +0 (a thread that is not `live` leaves +0), stores the sum in red[cl][el], and the block meets at a barrier.
//  2. slab_combine<EW>: t += red[k][el] for k = 0 ... NL - 1, in that order, starting from the value the caller passes.  Two
//     associations exist and each kernel keeps its own:  "dw first"  (dw + r0) + r1 + ...   the caller passes accumulate ? dw : +0
//                                                         "dw last"   dw + (0 + r0 + r1 + ...)   the caller passes +0 and adds dw
//     (k_reduce_slabs2, k_reduce_slabs: first; k_reduce_slabs_convt, k_reduce_slabs_stem: last -- the bits of the re-layout kernels
//     that used to add a summed temporary into the parameter gradient).
//  3. slab_point_sum<NP>: the Winograd weight gradients' slabs hold NP transform points per split; point p of an element is the sum
//     of its splits c = 0 ... nsplit - 1 in order, starting from +0, by ONE thread (no lanes, no combine).
//  4. slab_dw_3x3 / slab_store_row: the 3x3 result dW = G^T dU G of both Winograd forms, row by row: the kernel computes row a of
//     (.) G, the routine owns where it goes (igemm layout [tap][ci][co] or torch's OIHW [co][ci][tap]) and the accumulate read in
//     front of the row's three writes.
//
// Every reduction kernel is these calls plus its own index map or transform; each kernel reads dw where its association has it.
// k_wgrad_run_reduce (sprun.hip) follows 1 and 2, "dw first", with EW = 16 on float4 elements over one offset's pieces, in its own
// text: folded into these helpers the compiler gave it another instruction mix (profiles/r35_slab_sums.md).
// Included after common.h.
#pragma once

template <int EW>
__device__ __forceinline__ void slab_lane_sums(float (&red)[256 / EW][EW + 1], const float* __restrict__ slabs, int nsplit, int64_t n,
                                               int64_t i, bool live) {
  constexpr int NL = 256 / EW;
  const int el = threadIdx.x % EW, cl = threadIdx.x / EW;
  float s = 0.f;
  if (live)
#pragma unroll 8
    for (int c = cl; c < nsplit; c += NL) s += slabs[(int64_t)c * n + i];
  red[cl][el] = s;
  __syncthreads();
}

template <int EW>
__device__ __forceinline__ float slab_combine(const float (&red)[256 / EW][EW + 1], int el, float t) {
#pragma unroll
  for (int k = 0; k < 256 / EW; ++k) t += red[k][el];
  return t;
}

template <int NP>
__device__ __forceinline__ float slab_point_sum(const float* __restrict__ slabs, int nsplit, int64_t n, int64_t i, int p, bool live) {
  float s = 0.f;
  if (live)
#pragma unroll 8
    for (int c = 0; c < nsplit; ++c) s += slabs[((int64_t)c * NP + p) * n + i];
  return s;
}

// Where the 3x3 result of element i = ci * Cout + co (of n = Cin * Cout) goes: tap (a, b) is dw[base + (3 a + b) * step].
__device__ __forceinline__ void slab_dw_3x3(int64_t i, int64_t n, int oihw, int Cin, int Cout, int64_t& base, int64_t& step) {
  const int co = (int)(i % Cout), ci = (int)(i / Cout);
  base = oihw ? ((int64_t)co * Cin + ci) * 9 : i, step = oihw ? 1 : n;
}
// row a: d = dw + base + 3 a * step
__device__ __forceinline__ void slab_store_row(float* d, int64_t step, int accumulate, float g0, float g1, float g2) {
  if (accumulate) { g0 += d[0]; g1 += d[step]; g2 += d[2 * step]; }
  d[0] = g0; d[step] = g1; d[2 * step] = g2;
}
