// The host decisions of the streamed regressor TSQR (figh_regressor_tsqr, _tsqr_norms, _gram: figh_stream.hip) as a value:
// stream_plan() computes them all from plain facts of the call, before anything is allocated or launched, and the chunk
// loop only executes what the plan says.  Plain C++17 without a device: tools/stream_plan_host.cpp prints the plan of calls
// given as text, and tests/test_streamed_plan_host.py holds it against the Python mirror (tests/stream_common.py) with it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "figh.h"

namespace figh {

inline int64_t default_chunk(int rps, int ncols) {
    // ~2 GB of W per chunk: large enough to fill the chip (2048 waves x >= 8 tiles), small next to 288 GB
    int64_t c = (int64_t)(2.0e9 / (8.0 * rps * ncols));
    c = (c / 64) * 64;
    return c < 64 ? 64 : c;
}

// samples per chunk of a streamed pass over N >= 1 samples (chunk_samples == 0: the default), and of the chunk at `lo`
inline int64_t chunk_size(int64_t N, int64_t chunk_samples, int rps, int ncols) {
    if (chunk_samples == 0) chunk_samples = default_chunk(rps, ncols);
    return chunk_samples < N ? chunk_samples : N;
}
inline int64_t chunk_samples_at(int64_t lo, int64_t cs, int64_t N) { return (lo + cs <= N) ? cs : N - lo; }

// the chunk's W is a private workspace: tree models get the link-padded layout (16 columns per link, every row
// segment one 128-byte line) and the caller's column list is translated to it
inline bool chunk_w_padded(bool is_chain, int mode, int flags) {
    return !(is_chain && mode == FIGH_MODE_JOINT_TORQUE) && !(flags & FIGH_FLAG_TX40);
}
// its leading dimension; nlive > 0: the link-compact layout with that many link segments
inline int64_t chunk_w_ld(bool padded, int nlive, int nlinks, int ncols) {
    return padded ? 16 * (int64_t)(nlive > 0 ? nlive : nlinks) : ncols;
}

// What stream_plan needs to know of a call.
struct StreamCall {
    int rps = 0, ncols = 0;            // figh_regressor_shape
    int nlinks = 0, nv = 0, njoints = 0;
    bool is_chain = false;             // the chain kernel's models
    bool free_flyer = false;           // joint 1 is a free-flyer
    int mode = 0, flags = 0;
    bool with_tau = false, weighted = false;
    int64_t N = 0, chunk_samples = 0;  // N >= 1
    const int32_t *cols = nullptr;     // the caller's column list on the host, n entries (all columns: 0 .. n - 1)
    int n = 0;
    const int *link_pos = nullptr;     // tree_link_positions and its return value; nullptr / -1: does not apply
    int nlive = -1;
    int64_t chain_capacity = 0;        // the device's part: workgroups a chained launch can have (tsqr_level0_capacity - 1)
};

struct StreamPlan {
    int rps = 0, ncols = 0;             // the call's
    int n = 0, nc = 0;                  // kept columns, + tau
    int64_t cs = 0, nchunks = 0, last = 0;  // samples per chunk, chunks, samples of the last one
    bool padded = false;                // link-padded chunk W
    bool compact_applies = false;       // the link-compact layout exists for the call ...
    bool compact = false;               // ... and is used (not: the link-padded fallback)
    int nlive = -1;                     // its link segments when used, else -1
    int64_t ldc = 0;                    // leading dimension of the chunk's W
    std::vector<int32_t> first;         // structure hint: first possibly non-zero kept column per row block; empty = none
    bool chained = false;               // every workgroup keeps one running triangle across the chunks
    bool split = false;                 // force rows factored apart, over nf columns (ncf with tau)
    int nf = 0, ncf = 0;
    long chain_wgs = 0;                 // workgroups of a chained launch (0: not chained)
    int64_t level0_launches = 0;        // over all chunks
    int64_t pieces = 0;                 // row blocks of all chunks (rps x nchunks)

    // a chunk of nc_ samples runs with the hint
    bool hinted(int64_t nc_) const { return !first.empty() && nc_ >= 64; }
};

inline StreamPlan stream_plan(const StreamCall &c) {
    StreamPlan p;
    p.rps = c.rps, p.ncols = c.ncols;
    p.n = c.n;
    p.nc = c.n + (c.with_tau ? 1 : 0);
    const int n = p.n, nc = p.nc;
    p.cs = chunk_size(c.N, c.chunk_samples, c.rps, c.ncols);
    const int64_t cs = p.cs;
    p.nchunks = (c.N + cs - 1) / cs;
    p.last = c.N - (p.nchunks - 1) * cs;
    p.padded = chunk_w_padded(c.is_chain, c.mode, c.flags);
    // external wrench on a free-flyer root: links without entries (massless bodies) get no columns in the chunk's W
    // (FIGH_FLAG_LINK_COMPACT; the caller's column list can only name them if it keeps columns that are identically zero)
    p.nlive = p.padded && c.link_pos ? c.nlive : -1;
    if (p.nlive <= 0 || p.nlive >= c.nlinks) p.nlive = -1;
    p.compact_applies = p.nlive > 0;
    // a caller may list columns of links without entries (identically zero columns: the SIP program passes the inertial
    // columns of EVERY link, identification_tools.py:528-531): those exist in the link-padded layout only
    for (int k = 0; k < n && p.nlive > 0; ++k)
        if (c.cols[k] < 0 || c.cols[k] / 14 >= c.nlinks || c.link_pos[c.cols[k] / 14] < 0) p.nlive = -1;
    p.compact = p.nlive > 0;
    p.ldc = chunk_w_ld(p.padded, p.nlive, c.nlinks, c.ncols);
    // joint-torque regressor of single-dof joints: the rows of joint j only involve the links from j on, so the kept
    // columns in front of 14 j are exact zeros in row block j -- the structure hint of figh_tsqr_structured
    if (c.mode == FIGH_MODE_JOINT_TORQUE && c.nv == c.njoints - 1 && nc <= 80 && cs >= 64) {
        bool sorted = true;
        for (int k = 1; k < n; ++k) sorted = sorted && c.cols[k - 1] < c.cols[k];
        if (sorted) {
            p.first.resize(c.rps);
            for (int j = 0; j < c.rps; ++j) {
                int f = 0;
                while (f < n && c.cols[f] < 14 * j) ++f;
                p.first[j] = f;
            }
        }
    }
    // More than 80 columns and several chunks: CHAINED launches -- every workgroup of the blocked kernel keeps ONE running
    // triangle across the chunks (same workgroup count in every launch; a launch starts from the triangle the previous one
    // wrote), so the stack to merge holds one launch's triangles instead of nchunks times as many (human model, 20 chunks:
    // 512 instead of 10 240 triangles, merges 8.3 -> 1.8 ms).
    p.chained = nc > 80 && p.nchunks > 1;
    // External wrench on a free-flyer root: per chunk the three force row blocks are factored over the nf columns that can
    // be non-zero there (rotational-inertia columns are exact zeros in force rows, figh_tsqr_selected_wrench) and reduced to
    // one triangle per chunk; the torque row blocks go through the (chained) launches over all columns.
    if (c.mode == FIGH_MODE_EXT_WRENCH && c.rps == 6 && c.free_flyer && !(c.flags & FIGH_FLAG_TX40) && !c.weighted && nc > 80 &&
        3 * cs >= 16L * nc) {
        for (int k = 0; k < n; ++k) p.nf += (c.cols[k] % 14) >= 6;
        if (p.nf >= n) p.nf = 0;
    }
    p.split = p.nf > 0;
    p.ncf = p.nf + (c.with_tau ? 1 : 0);
    const long rsplit = p.split ? 2 : 1;  // the torque rows are half of a chunk
    if (p.chained) p.chain_wgs = std::min<long>(c.chain_capacity, std::max<long>(1, (long)c.rps * cs / rsplit / (8L * nc)));
    p.level0_launches = p.nchunks * (p.split ? 2 : 1);
    p.pieces = c.rps * p.nchunks;
    return p;
}

}  // namespace figh
