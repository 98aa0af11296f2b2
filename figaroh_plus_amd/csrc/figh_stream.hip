// Streamed ("fused" in SURVEY.md section 8b) entry points: the stacked regressor is never materialised in full.
// The samples are cut into chunks; each chunk's W lives in a library workspace just long enough for the next kernel
// (column norms, or the level-0 Householder TSQR) and is then overwritten by the next chunk.  This is what makes the
// human model at 1e7 samples (269 GB of W) or any W beyond HBM tractable, and it is the C-ABI form of
// IdentificationPipeline(chunk_samples=...).
//
//   figh_regressor_colsq  : diag(W^T W) of build_regressor_basic's W               (regressor.py:243,271)
//   figh_regressor_tsqr   : R of np.linalg.qr(W[:, col_idx] | tau), optionally row-block weighted
//                                                                                   (qrdecomposition.py:105,205,238)
//   figh_regressor_gram   : W_e^T W_e, W_e^T tau, tau^T tau from that R (host, O(n^3)) -- the normal-equation
//                           quantities of the SIP QP (identification_tools.py:528-531) and of collective (1) in
//                           SURVEY.md section 8e, without squaring the condition number on the way.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "figh_internal.h"
#include "figh_stream_plan.h"

using namespace figh;

namespace {

__global__ __launch_bounds__(256) void vec_add_kernel(double *__restrict__ acc, const double *__restrict__ x, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) acc[i] += x[i];
}

// reference column 14 l + s -> link-padded column 16 l + s (a NULL list = all columns)
// (link_pos: the link-compact layout, FIGH_FLAG_LINK_COMPACT -- a link without a segment only has eliminated columns, which
// no caller lists; should one be listed all the same it reads segment 0: values of another column, never out of range)
__global__ __launch_bounds__(256) void pad_columns_kernel(const int32_t *__restrict__ in, int n, int32_t *__restrict__ out,
                                                          const int *__restrict__ link_pos) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int c = in ? in[i] : i;
        const int l = link_pos ? max(link_pos[c / 14], 0) : c / 14;
        out[i] = l * 16 + c % 14;
    }
}

// The W of a streamed chunk or of a whole batch, in a library workspace of the caller's: its layout (figh_stream_plan.h), the
// caller's column list in its numbering, and the regressor entry that writes it.
struct ChunkW {
    bool padded;
    int64_t ldc;
    int flags;                        // the caller's, + FIGH_FLAG_LINK_COMPACT once columns() got a link map
    const int32_t *d_cols = nullptr;  // columns(): the caller's list in W's numbering

    // nlive > 0: the link-compact layout with that many link segments
    ChunkW(figh_model_t model, int mode, int flags, int ncols, int nlive = -1)
        : padded(chunk_w_padded(model->is_chain, mode, flags)), ldc(chunk_w_ld(padded, nlive, model->host.nlinks, ncols)),
          flags(flags) {}

    // link_pos (host, one entry per link; nullptr: none) goes to the device, and a padded layout gets the translated list
    int columns(figh_model_t model, const int32_t *d_col_idx, int n, const int *link_pos) {
        int *d_link_pos = nullptr;
        if (link_pos) {
            d_link_pos = static_cast<int *>(workspace(sizeof(int) * kMaxJoints, kWsLinkPos));
            if (!d_link_pos) return FIGH_ERR_ALLOC;
            FIGH_HIP(hipMemcpyAsync(d_link_pos, link_pos, sizeof(int) * model->host.nlinks, hipMemcpyHostToDevice, stream()));
            FIGH_HIP(hipStreamSynchronize(stream()));  // (link_pos is the caller's memory)
            flags |= FIGH_FLAG_LINK_COMPACT;
        }
        d_cols = d_col_idx;
        if (!padded) return FIGH_OK;
        int32_t *out = static_cast<int32_t *>(workspace(sizeof(int32_t) * (size_t)n, kWsChunkNormsOrCols));
        if (!out) return FIGH_ERR_ALLOC;
        hipLaunchKernelGGL(pad_columns_kernel, dim3((n + 255) / 256), dim3(256), 0, stream(), d_col_idx, n, out,
                           (const int *)d_link_pos);
        FIGH_HIP(hipGetLastError());
        d_cols = out;
        return FIGH_OK;
    }

    // W of `ns` samples into Wc (rps * ns rows of ldc); d_colsq (nullable): diag(W^T W) of all columns
    int build(figh_model_t model, int mode, int ft_mask, int64_t ns, const double *d_q, const double *d_v, const double *d_a,
              double *Wc, double *d_colsq) const {
        return padded ? figh_regressor_build_padded(model, mode, flags, ft_mask, ns, d_q, d_v, d_a, Wc, ldc, d_colsq)
                      : figh_regressor_build(model, mode, flags, ft_mask, ns, d_q, d_v, d_a, Wc, ldc, d_colsq);
    }
};

// the caller's column list on the host (a NULL list = all n columns)
int host_column_list(const int32_t *d_col_idx, int n, std::vector<int32_t> &cols) {
    cols.resize(n);
    if (d_col_idx) return figh_memcpy_d2h(cols.data(), d_col_idx, sizeof(int32_t) * n);
    for (int c = 0; c < n; ++c) cols[c] = c;
    return FIGH_OK;
}

}  // namespace

extern "C" int figh_regressor_colsq(figh_model_t model, int mode, int flags, int ft_mask, int64_t N, const double *d_q,
                                    const double *d_v, const double *d_a, int64_t chunk_samples, double *d_colsq) {
    int rps = 0, ncols = 0;
    if (int rc = figh_regressor_shape(model, mode, flags, &rps, &ncols)) return rc;
    FIGH_REQUIRE(N >= 0 && chunk_samples >= 0, "negative size");
    FIGH_REQUIRE(d_q && d_v && d_a && d_colsq, "NULL device pointer");
    if (int rc = ensure_device()) return rc;
    FIGH_HIP(hipMemsetAsync(d_colsq, 0, sizeof(double) * ncols, stream()));
    if (N == 0) return FIGH_OK;
    if (!(model->is_chain && mode == FIGH_MODE_JOINT_TORQUE && !(flags & FIGH_FLAG_GENERIC)) && !(flags & FIGH_FLAG_TX40)) {
        // tree kernel: the norms are accumulated from the computed segments directly, W is never written (nor chunked)
        int done = 0;
        if (int rc = launch_regressor_tree(model, mode, flags, ft_mask, N, d_q, d_v, d_a, nullptr, 0, ncols, 16, d_colsq, &done))
            return rc;
        return FIGH_OK;
    }
    const int64_t cs = chunk_size(N, chunk_samples, rps, ncols);
    double *Wc = static_cast<double *>(workspace(sizeof(double) * (size_t)rps * cs * ncols, kWsChunkW));
    double *part = static_cast<double *>(workspace(sizeof(double) * ncols, kWsChunkNormsOrCols));
    if (!Wc || !part) return FIGH_ERR_ALLOC;
    const int nq = model->host.nq, nv = model->host.nv;
    for (int64_t lo = 0; lo < N; lo += cs) {
        if (int rc = figh_regressor_build(model, mode, flags, ft_mask, chunk_samples_at(lo, cs, N), d_q + lo * nq,
                                          d_v + lo * nv, d_a + lo * nv, Wc, ncols, part))
            return rc;
        hipLaunchKernelGGL(vec_add_kernel, dim3((ncols + 255) / 256), dim3(256), 0, stream(), d_colsq, part, ncols);
        FIGH_HIP(hipGetLastError());
    }
    return FIGH_OK;
}

// ---- The streamed TSQR (figh_regressor_tsqr, _tsqr_norms and, through the first, _gram) in phases: the argument checks,
// one fetch of the column list, the plan (figh_stream_plan.h: every decision, nothing launched), workspaces sized from it,
// the chunk loop that only executes it, the merge.
namespace {

struct StreamArgs {  // figh_regressor_tsqr_norms' arguments (d_colsq_out nullable)
    figh_model_t model;
    int mode, flags, ft_mask;
    int64_t N;
    const double *d_q, *d_v, *d_a;
    const int32_t *d_col_idx;
    int n;
    const double *d_tau, *h_block_weight;
    int nblocks;
    int64_t chunk_samples;
    double *d_R_out, *d_colsq_out;
};

// phase 1: refuse, or zero what the chunks accumulate into; *done: no samples, the outputs are final
int check_stream_args(const StreamArgs &a, int *rps, int *ncols, bool *done) {
    if (int rc = figh_regressor_shape(a.model, a.mode, a.flags, rps, ncols)) return rc;
    FIGH_REQUIRE(a.N >= 0 && a.chunk_samples >= 0, "negative size");
    FIGH_REQUIRE(a.d_q && a.d_v && a.d_a && a.d_R_out, "NULL device pointer");
    FIGH_REQUIRE(a.n >= 1 && (a.d_col_idx ? a.n <= *ncols : a.n == *ncols), "bad column count");
    if (a.h_block_weight)
        FIGH_REQUIRE(a.nblocks > 0 && *rps % a.nblocks == 0, "row-block weights must divide the rows of a sample");
    if (int rc = ensure_device()) return rc;
    if (a.d_colsq_out) FIGH_HIP(hipMemsetAsync(a.d_colsq_out, 0, sizeof(double) * *ncols, stream()));
    *done = a.N == 0;
    if (*done) {
        const int nc = a.n + (a.d_tau ? 1 : 0);
        FIGH_HIP(hipMemsetAsync(a.d_R_out, 0, sizeof(double) * (size_t)nc * nc, stream()));
        return FIGH_OK;
    }
    const int64_t cs = chunk_size(a.N, a.chunk_samples, *rps, *ncols);
    FIGH_REQUIRE(!(a.flags & FIGH_FLAG_BLOCKED_INPUTS) || cs >= a.N || cs % 64 == 0,
                 "tile-blocked inputs: chunk_samples must be a multiple of 64");
    return FIGH_OK;
}

// phase 3: the call as stream_plan sees it (cols: the caller's list on the host; link_pos: kMaxJoints entries, filled here)
StreamPlan plan_stream(const StreamArgs &a, int rps, int ncols, const std::vector<int32_t> &cols, int *link_pos) {
    const DevModel &h = a.model->host;
    StreamCall c;
    c.rps = rps, c.ncols = ncols;
    c.nlinks = h.nlinks, c.nv = h.nv, c.njoints = h.njoints;
    c.is_chain = a.model->is_chain;
    c.free_flyer = h.njoints > 1 && h.jtype[1] == FIGH_JT_FREEFLYER;
    c.mode = a.mode, c.flags = a.flags;
    c.with_tau = a.d_tau != nullptr, c.weighted = a.h_block_weight != nullptr;
    c.N = a.N, c.chunk_samples = a.chunk_samples;
    c.cols = cols.data(), c.n = a.n;
    c.link_pos = link_pos;
    c.nlive = tree_link_positions(a.model, a.mode, a.flags & 7, a.ft_mask, link_pos);
    c.chain_capacity = tsqr_level0_capacity(a.n + (a.d_tau ? 1 : 0)) - 1;
    return stream_plan(c);
}

// phase 4: the workspaces, sized from the plan
struct StreamWork {
    int64_t per_chunk = 0, cap_f = 0;  // level-0 triangles one launch can produce: all rows / torque rows, force rows
    double *Wc = nullptr, *tc = nullptr, *cs_part = nullptr, *stack = nullptr;
    int *fsel = nullptr;
    double *stack_f = nullptr, *Rf = nullptr;

    int allocate(const StreamArgs &a, const StreamPlan &p) {
        const int nc = p.nc, ncf = p.ncf;
        // diag(W^T W) of all columns fused into the regressor kernel of every chunk (the elimination's input, for a caller
        // that factors the columns it EXPECTS to be kept and verifies the set afterwards: no separate norms pass over the
        // samples)
        if (a.d_colsq_out) cs_part = static_cast<double *>(workspace(sizeof(double) * p.ncols, kWsChunkNormsFused));
        Wc = static_cast<double *>(workspace(sizeof(double) * (size_t)p.rps * p.cs * p.ldc, kWsChunkW));
        if (a.d_tau) tc = static_cast<double *>(workspace(sizeof(double) * (size_t)p.rps * p.cs, kWsChunkTau));
        // level-0 triangles of ALL chunks are stacked and the merge tree runs once (a merge is latency-bound: running it
        // per chunk cost 158 ms of the 1.24 s human pass)
        per_chunk = tsqr_level0_capacity(nc);
        stack = static_cast<double *>(workspace(sizeof(double) * (size_t)p.nchunks * per_chunk * nc * nc, kWsChunkStack));
        if ((a.d_colsq_out && !cs_part) || !Wc || (a.d_tau && !tc) || !stack) return FIGH_ERR_ALLOC;
        if (!p.split) return FIGH_OK;
        cap_f = tsqr_level0_capacity(ncf);
        fsel = static_cast<int *>(workspace(sizeof(int) * 2 * (size_t)p.n, kWsForceCols));
        // the force rows' level-0 triangles of ALL chunks are stacked and merged once (a merge per chunk cost 0.175 ms x 20
        // for the human model)
        stack_f = static_cast<double *>(workspace(sizeof(double) * (size_t)ncf * ncf * cap_f * p.nchunks, kWsChunkForceStack));
        Rf = static_cast<double *>(workspace(sizeof(double) * (size_t)ncf * ncf, kWsForceOrBlockR));
        return fsel && stack_f && Rf ? FIGH_OK : FIGH_ERR_ALLOC;
    }
};

// phase 5: the chunk of the samples from `lo` on -- W, the norms, tau, the level-0 launches the plan says; *have, *have_f:
// the triangles in w.stack and w.stack_f
int run_chunk(const StreamArgs &a, const StreamPlan &p, const ChunkW &cw, const StreamWork &w, int64_t lo, int64_t *have,
              int64_t *have_f) {
    const int rps = p.rps, n = p.n, nc = p.nc, nq = a.model->host.nq, nv = a.model->host.nv;
    const int64_t nc_ = chunk_samples_at(lo, p.cs, a.N), ldc = p.ldc;
    if (int rc = cw.build(a.model, a.mode, a.ft_mask, nc_, a.d_q + lo * nq, a.d_v + lo * nv, a.d_a + lo * nv, w.Wc, w.cs_part))
        return rc;
    if (w.cs_part) {
        hipLaunchKernelGGL(vec_add_kernel, dim3((p.ncols + 255) / 256), dim3(256), 0, stream(), a.d_colsq_out, w.cs_part,
                           p.ncols);
        FIGH_HIP(hipGetLastError());
    }
    if (a.d_tau)  // rows j*N + [lo, lo + nc_) of tau -> the chunk's joint-major vector (rows j*nc_ + i)
        FIGH_HIP(hipMemcpy2DAsync(w.tc, sizeof(double) * nc_, a.d_tau + lo, sizeof(double) * a.N, sizeof(double) * nc_, rps,
                                  hipMemcpyDeviceToDevice, stream()));
    Level0Options torque;  // (the torque rows: all of the chunk's rows unless it is split)
    if (p.hinted(nc_)) {
        if (int rc = tile_hint(p.first.data(), rps, (int64_t)rps * nc_, n, nc, &torque.hint)) return rc;
    }
    const int64_t rows_f = p.split ? 3 * nc_ : 0;  // the chunk's force rows (row blocks 0 .. 2 of its joint-major W)
    if (p.split) {
        int64_t cnt_f = 0;
        if (int rc = tsqr_level0(w.Wc, rows_f, ldc, w.fsel, p.nf, w.tc, nullptr, 0, w.stack_f + (size_t)*have_f * p.ncf * p.ncf,
                                 w.cap_f, &cnt_f, nullptr))
            return rc;
        *have_f += cnt_f;
    }
    if (p.chained) {
        torque.chain_wgs = p.chain_wgs;
        torque.chain_flags = lo > 0 ? 1 : 0;
    }
    int64_t got = 0;
    if (int rc = tsqr_level0(w.Wc + rows_f * ldc, (int64_t)rps * nc_ - rows_f, ldc, cw.d_cols, n, w.tc ? w.tc + rows_f : nullptr,
                             a.h_block_weight, a.nblocks, w.stack + (size_t)(p.chained ? 0 : *have) * nc * nc, w.per_chunk,
                             &got, nullptr, torque))
        return rc;
    *have = p.chained ? got : *have + got;
    return FIGH_OK;
}

int regressor_tsqr_impl(const StreamArgs &a) {
    int rps = 0, ncols = 0;
    bool done = false;
    if (int rc = check_stream_args(a, &rps, &ncols, &done)) return rc;
    if (done) return FIGH_OK;
    std::vector<int32_t> cols;
    if (int rc = host_column_list(a.d_col_idx, a.n, cols)) return rc;
    int link_pos[kMaxJoints];
    const StreamPlan p = plan_stream(a, rps, ncols, cols, link_pos);
    ChunkW cw(a.model, a.mode, a.flags, ncols, p.nlive);
    if (int rc = cw.columns(a.model, a.d_col_idx, a.n, p.compact ? link_pos : nullptr)) return rc;
    StreamWork w;
    if (int rc = w.allocate(a, p)) return rc;
    if (p.split)
        if (int rc = split_force_columns(cw.d_cols, p.n, cw.padded ? 16 : 14, w.fsel)) return rc;
    int64_t have = 0, have_f = 0;
    for (int64_t lo = 0; lo < a.N; lo += p.cs)
        if (int rc = run_chunk(a, p, cw, w, lo, &have, &have_f)) return rc;
    FIGH_REQUIRE(have < (1LL << 31), "too many level-0 triangles");
    if (p.split) {  // the force rows' triangle of all chunks, over all kept columns, as one more element of the stack
        FIGH_REQUIRE(have_f < (1LL << 31), "too many level-0 triangles");
        if (int rc = append_force_triangle(w.stack_f, have_f, p.ncf, p.nf, w.fsel + p.n, w.Rf, p.nc, p.n, w.stack, &have)) return rc;
    }
    return figh_tsqr_merge(w.stack, (int)have, p.nc, a.d_R_out);
}

}  // namespace

extern "C" int figh_regressor_tsqr(figh_model_t model, int mode, int flags, int ft_mask, int64_t N, const double *d_q,
                                   const double *d_v, const double *d_a, const int32_t *d_col_idx, int n,
                                   const double *d_tau, const double *h_block_weight, int nblocks, int64_t chunk_samples,
                                   double *d_R_out) {
    return regressor_tsqr_impl({model, mode, flags, ft_mask, N, d_q, d_v, d_a, d_col_idx, n, d_tau, h_block_weight, nblocks,
                                chunk_samples, d_R_out, nullptr});
}

extern "C" int figh_regressor_tsqr_norms(figh_model_t model, int mode, int flags, int ft_mask, int64_t N, const double *d_q,
                                         const double *d_v, const double *d_a, const int32_t *d_col_idx, int n,
                                         const double *d_tau, const double *h_block_weight, int nblocks,
                                         int64_t chunk_samples, double *d_R_out, double *d_colsq_out) {
    FIGH_REQUIRE(d_colsq_out, "NULL device pointer");
    return regressor_tsqr_impl({model, mode, flags, ft_mask, N, d_q, d_v, d_a, d_col_idx, n, d_tau, h_block_weight, nblocks,
                                chunk_samples, d_R_out, d_colsq_out});
}

// triangles of the previous trajectories (common) and of trajectory b, interleaved: the stack of the pair level that
// folds the first into every one of the B results
__global__ __launch_bounds__(256) void interleave_stack_kernel(const double *__restrict__ common,
                                                               const double *__restrict__ each, const long tri,
                                                               const long B, double *__restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= tri * B) return;
    const long b = e / tri, k = e - b * tri;
    out[2 * b * tri + k] = common[k];
    out[(2 * b + 1) * tri + k] = each[e];
}

extern "C" int figh_regressor_tsqr_batch(figh_model_t model, int mode, int flags, int ft_mask, int64_t B, int64_t n_per,
                                         const double *d_q, const double *d_v, const double *d_a,
                                         const int32_t *d_col_idx, int n, const double *d_R_stack, double *d_R_out) {
    int rps = 0, ncols = 0;
    if (int rc = figh_regressor_shape(model, mode, flags, &rps, &ncols)) return rc;
    FIGH_REQUIRE(B >= 1 && n_per >= 1, "figh_regressor_tsqr_batch: at least one trajectory of at least one sample");
    FIGH_REQUIRE(d_q && d_v && d_a && d_R_out, "NULL device pointer");
    FIGH_REQUIRE(n >= 1 && (d_col_idx ? n <= ncols : n == ncols) && n <= 512, "bad column count");
    if (int rc = ensure_device()) return rc;
    const int nc = n;
    const size_t tri = (size_t)nc * nc;
    const int nq = model->host.nq, nv = model->host.nv;
    const int64_t N_tot = B * n_per;
    if (nc <= 80 || (int64_t)rps * n_per < 8L * nc) {
        // register-tile kernel (or trajectories too short to be cut further): a launch pair per trajectory
        FIGH_REQUIRE(!(flags & FIGH_FLAG_BLOCKED_INPUTS) || n_per % 64 == 0,
                     "tile-blocked inputs: samples per trajectory must be a multiple of 64");
        double *pair = d_R_stack ? static_cast<double *>(workspace(sizeof(double) * 2 * tri, kWsBatchPair)) : nullptr;
        if (d_R_stack && !pair) return FIGH_ERR_ALLOC;
        if (d_R_stack) FIGH_HIP(hipMemcpyAsync(pair, d_R_stack, sizeof(double) * tri, hipMemcpyDeviceToDevice, stream()));
        for (int64_t b = 0; b < B; ++b) {
            double *dst = d_R_stack ? pair + tri : d_R_out + (size_t)b * tri;
            if (int rc = figh_regressor_tsqr(model, mode, flags, ft_mask, n_per, d_q + b * n_per * nq, d_v + b * n_per * nv,
                                             d_a + b * n_per * nv, d_col_idx, n, nullptr, nullptr, 0, n_per, dst))
                return rc;
            if (d_R_stack)
                if (int rc = figh_tsqr_merge(pair, 2, nc, d_R_out + (size_t)b * tri)) return rc;
        }
        return FIGH_OK;
    }
    // ---- blocked kernel: ONE K1 launch over all B * n_per samples (the standard joint-major regressor: trajectory b is the
    // rps row segments [j N_tot + b n_per, + n_per)), ONE batched level-0 launch (wgs workgroups per trajectory), then
    // pair levels over the whole stack -- wgs is a power of two, so a pair never straddles two trajectories
    ChunkW cw(model, mode, flags, ncols);
    const int64_t ldc = cw.ldc;
    FIGH_REQUIRE(ldc < (1L << 21), "figh_tsqr: more than 80 columns need a leading dimension below 2^21 elements");
    double *Wc = static_cast<double *>(workspace(sizeof(double) * (size_t)rps * N_tot * ldc, kWsChunkW));
    if (!Wc) return FIGH_ERR_ALLOC;
    if (int rc = cw.columns(model, d_col_idx, n, nullptr)) return rc;
    if (int rc = cw.build(model, mode, ft_mask, N_tot, d_q, d_v, d_a, Wc, nullptr)) return rc;
    const long M = tsqr_wide_tile_rows(nc);
    const long tiles = rps * ((n_per + M - 1) / M);
    // workgroups per trajectory: enough in total to fill the chip twice over, a leaf at least four tiles and 4 nc rows tall
    long cap = std::min<long>({tiles / 4, (long)(rps * n_per) / (4L * nc), std::max<long>(1, 1024 / B)});
    long wgs = 1;
    while (2 * wgs <= cap) wgs *= 2;
    double *stack = static_cast<double *>(workspace(sizeof(double) * tri * (size_t)(B * wgs), kWsChunkStack));
    if (!stack) return FIGH_ERR_ALLOC;
    {
        ProfileScope scope("tsqr_batch");
        if (int rc = launch_tsqr_wide_batch(Wc, ldc, cw.d_cols, n, nc, B, n_per, rps, N_tot, wgs, stack)) return rc;
    }
    const double *cur = stack;
    WorkspaceSlot slot = kWsMergeA;
    for (long w = wgs; w > 1; w /= 2) {
        ProfileScope scope("tsqr_reduce");
        double *dst = (w == 2 && !d_R_stack) ? d_R_out : static_cast<double *>(workspace(sizeof(double) * tri * (size_t)(B * w / 2), slot));
        if (!dst) return FIGH_ERR_ALLOC;
        if (int rc = launch_tsqr_wide_pairs(cur, B * w, nc, dst)) return rc;
        cur = dst;
        slot = slot == kWsMergeA ? kWsMergeB : kWsMergeA;
    }
    if (!d_R_stack) {
        if (cur != d_R_out) FIGH_HIP(hipMemcpyAsync(d_R_out, cur, sizeof(double) * tri * B, hipMemcpyDeviceToDevice, stream()));
        return FIGH_OK;
    }
    double *both = static_cast<double *>(workspace(sizeof(double) * 2 * tri * (size_t)B, kWsBatchPair));
    if (!both) return FIGH_ERR_ALLOC;
    hipLaunchKernelGGL(interleave_stack_kernel, dim3((unsigned)((tri * B + 255) / 256)), dim3(256), 0, stream(), d_R_stack, cur,
                       (long)tri, (long)B, both);
    FIGH_HIP(hipGetLastError());
    ProfileScope scope("tsqr_reduce");
    return launch_tsqr_wide_pairs(both, 2 * B, nc, d_R_out);
}

extern "C" int figh_regressor_gram(figh_model_t model, int mode, int flags, int ft_mask, int64_t N, const double *d_q,
                                   const double *d_v, const double *d_a, const int32_t *d_col_idx, int n,
                                   const double *d_tau, int64_t chunk_samples, double *h_G, double *h_g,
                                   double *h_tau_sq) {
    FIGH_REQUIRE(h_G, "NULL output");
    FIGH_REQUIRE(!d_tau || (h_g && h_tau_sq), "tau given but no output for W^T tau / tau^T tau");
    const int nc = n + (d_tau ? 1 : 0);
    FIGH_REQUIRE(n >= 1 && nc <= 512, "bad column count");
    double *d_R = static_cast<double *>(workspace(sizeof(double) * (size_t)nc * nc, kWsGramR));
    if (!d_R) return FIGH_ERR_ALLOC;
    if (int rc = figh_regressor_tsqr(model, mode, flags, ft_mask, N, d_q, d_v, d_a, d_col_idx, n, d_tau, nullptr, 0,
                                     chunk_samples, d_R))
        return rc;
    std::vector<double> R((size_t)nc * nc);
    if (int rc = figh_memcpy_d2h(R.data(), d_R, sizeof(double) * R.size())) return rc;
    // W^T W = R1^T R1, W^T tau = R1^T z, tau^T tau = z^T z + rho^2 with R = [R1 z; 0 rho]
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k <= i; ++k) s += R[(size_t)k * nc + i] * R[(size_t)k * nc + j];
            h_G[(size_t)i * n + j] = s;
            h_G[(size_t)j * n + i] = s;
        }
    if (d_tau) {
        double tt = 0.0;
        for (int k = 0; k < nc; ++k) tt += R[(size_t)k * nc + n] * R[(size_t)k * nc + n];
        *h_tau_sq = tt;
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            for (int k = 0; k <= i; ++k) s += R[(size_t)k * nc + i] * R[(size_t)k * nc + n];
            h_g[i] = s;
        }
    }
    return FIGH_OK;
}
