// The two small steps behind a pass's big kernels -- the fixed-order sum of the workgroups' diag(W^T W) partials and the
// column selection on the sums -- as device functions, so that the stand-alone kernels (figh_linalg.hip) and the extra
// workgroup of the streamed merge launch (figh_tsqr_stream.hip) run ONE copy of each: same additions in the same order,
// same bits.  __noinline__: a caller's own register allocation does not see their bodies.
#pragma once

#include "figh_internal.h"

namespace figh {

constexpr int kReduceCols = 8;      // columns one group of 256 threads sums per call

// part[b][c0 + j], b < nblocks -> sm[256 j] for j < count <= kReduceCols, by one group of 256 threads (t = 0 .. 255; sm:
// 256 count doubles of LDS of the group's own).  Thread t sums the partials b = t, t + 256, ... in that order, then the
// halving tree sm[t] += sm[t + w], w = 128 .. 1.  Every thread of the WORKGROUP must call it (it holds workgroup barriers;
// count = 0 only takes part in them); the sums are visible to the whole group on return.
static __device__ __noinline__ void reduce_partials_cols(const double *__restrict__ part, const int nblocks, const int ncols,
                                                  const int c0, const int count, double *sm, const int t) {
    double s[kReduceCols];
#pragma unroll
    for (int j = 0; j < kReduceCols; ++j) s[j] = 0.0;
    for (int b = t; b < nblocks; b += 256) {
        const double *row = part + (long)b * ncols + c0;
#pragma unroll
        for (int j = 0; j < kReduceCols; ++j)
            if (j < count) s[j] += row[j];
    }
#pragma unroll
    for (int j = 0; j < kReduceCols; ++j)
        if (j < count) sm[256 * j + t] = s[j];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int j = 0; j < kReduceCols; ++j)
                if (j < count) sm[256 * j + t] += sm[256 * j + t + w];
        }
        __syncthreads();
    }
}

// select_columns_kernel behind its kept flags (kept[c] = 0 / 1, LDS, complete): the selection words sel (layout at the
// kernel), written by the threads tid of nthreads.  No word is written twice.
static __device__ __noinline__ void select_columns_write(const int *kept, const int ncols, const int link_stride,
                                                  const int *__restrict__ link_pos, int *__restrict__ sel, const int tid,
                                                  const int nthreads) {
    int total = 0;
    for (int c = 0; c < ncols; ++c) total += kept[c];
    for (int c = tid; c < ncols; c += nthreads) {
        int pos = 0;
        for (int e = 0; e < c; ++e) pos += kept[e];
        // (link_pos: the link-compact layout of figh_regressor_build_padded + FIGH_FLAG_LINK_COMPACT -- a kept column's link
        // always has a segment there: columns of links without one have norm exactly 0)
        if (kept[c]) sel[2 + pos] = (link_pos ? max(link_pos[c / 14], 0) : c / 14) * link_stride + c % 14;
        if (c >= total) sel[2 + c] = 0;
        sel[2 + ncols + c] = kept[c];
    }
    if (tid == 0) {
        sel[0] = total;
        sel[1] = ncols;
    }
}

}  // namespace figh
