// The two ends of the excitation loop on the device: waypoints in, resident (q, v, a) out
// (CubicSpline.get_full_config, examples/tiago/utils/cubic_spline.py:82-181), and the constraint vectors of
// get_constraints_all_samples (examples/tiago/optimal_trajectory.py:136-188, without the collision distances) out of the
// resident v and tau.  In between run figh_regressor_tsqr_batch[_fused] and figh_regressor_apply on the same buffers.
//
// The trajectory.  The scripts always pass velocity and acceleration waypoints, so get_active_config builds one
// ndcurves.exact_cubic per pair of neighbouring waypoints with init_vel / end_vel / init_acc / end_acc: the unique quintic
// through position, velocity and acceleration at both ends.  This translation unit is compiled without FMA contraction and
// states that quintic in ONE operation order, which the NumPy mirror (tools/excitation.py, spline_coefficients /
// spline_samples) follows operation by operation; every operation below is one correctly rounded + - * /, evaluated left to
// right with the parentheses as written, so device and mirror are bit-equal.
//
//   segment k, active joint s:  h = tps[k+1] - tps[k];  h2 = h * h;  h3 = h2 * h;  h4 = h3 * h;  h5 = h4 * h
//                               D = p1 - p0             ((p0, v0, a0) at waypoint k, (p1, v1, a1) at waypoint k + 1)
//     c0 = p0      c1 = v0      c2 = a0 / 2
//     c3 = ((20 * D - (8 * v1 + 12 * v0) * h) - (3 * a0 - a1) * h2) / (2 * h3)
//     c4 = ((-30 * D + (14 * v1 + 16 * v0) * h) + (3 * a0 - 2 * a1) * h2) / (2 * h4)
//     c5 = ((12 * D - (6 * (v1 + v0)) * h) - (a0 - a1) * h2) / (2 * h5)
//   sample i:  t = tps[0] + i * delta_t  (delta_t = 1 / freq);  k = the largest index with tps[k] <= t, at most n_wps - 2;
//              u = min(t - tps[k], tps[k+1] - tps[k])
//     q   = ((((c5 * u + c4) * u + c3) * u + c2) * u + c1) * u + c0
//     dq  = ((((5 * c5) * u + 4 * c4) * u + 3 * c3) * u + 2 * c2) * u + c1
//     ddq = (((20 * c5) * u + 12 * c4) * u + 6 * c3) * u + 2 * c2
//
// The cap on u changes nothing except where rounding puts the last sample behind tps[-1]: ndcurves raises there, this code
// evaluates the end of the last segment.
#include "figh_internal.h"

using namespace figh;

namespace {

constexpr long kMaxGrid = 1 << 16;               // workgroups per launch; every kernel loops over what is left
constexpr int kMaxQ = 7 * (kMaxJoints - 1);      // position columns of the widest model
constexpr int kMaxV = 6 * (kMaxJoints - 1);      // velocity columns

// column -> active joint (position in the waypoint arrays) or -1, by value: read through the kernel-argument segment
struct SplinePlan {
    int nq, nv, n_act;
    short qmap[kMaxQ];
    short vmap[kMaxV];
};

// active joint -> column, for the constraint gather
struct ConstraintPlan {
    int n_act;
    short idxq[kMaxV];
    short idxv[kMaxV];
};

// First phase, one launch: items [0, B * nseg * n_act) form the six coefficients of (trajectory, segment, active joint);
// items behind them, one per sample of a trajectory, form the segment index and the local time that all B trajectories
// share.
__global__ __launch_bounds__(256) void spline_prologue_kernel(const long B, const int n_wps, const int n_act, const long n_per,
                                                              const double delta_t, const double *__restrict__ tps,
                                                              const double *__restrict__ wps, const double *__restrict__ vel,
                                                              const long vel_stride, const double *__restrict__ acc,
                                                              const long acc_stride, double *__restrict__ coef,
                                                              int *__restrict__ seg, double *__restrict__ local) {
    const int nseg = n_wps - 1;
    const long ncoef = B * nseg * n_act, total = ncoef + n_per;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        if (e < ncoef) {
            const int s = (int)(e % n_act);
            const long bk = e / n_act;
            const int k = (int)(bk % nseg);
            const long b = bk / nseg;
            const long at = (long)s * n_wps + k;  // the reference's (n_act, n_wps) layout
            const double p0 = wps[b * n_act * n_wps + at], p1 = wps[b * n_act * n_wps + at + 1];
            const double v0 = vel[b * vel_stride + at], v1 = vel[b * vel_stride + at + 1];
            const double a0 = acc[b * acc_stride + at], a1 = acc[b * acc_stride + at + 1];
            const double h = tps[k + 1] - tps[k];
            const double h2 = h * h, h3 = h2 * h, h4 = h3 * h, h5 = h4 * h;
            const double D = p1 - p0;
            double *c = coef + 6 * e;
            c[0] = p0;
            c[1] = v0;
            c[2] = a0 / 2.0;
            c[3] = ((20.0 * D - (8.0 * v1 + 12.0 * v0) * h) - (3.0 * a0 - a1) * h2) / (2.0 * h3);
            c[4] = ((-30.0 * D + (14.0 * v1 + 16.0 * v0) * h) + (3.0 * a0 - 2.0 * a1) * h2) / (2.0 * h4);
            c[5] = ((12.0 * D - (6.0 * (v1 + v0)) * h) - (a0 - a1) * h2) / (2.0 * h5);
        } else {
            const long i = e - ncoef;
            const double t = tps[0] + (double)i * delta_t;
            int lo = 0, hi = nseg - 1;  // the largest k <= n_wps - 2 with tps[k] <= t (tps[0] <= t always)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (tps[mid] <= t) lo = mid;
                else hi = mid - 1;
            }
            const double u = t - tps[lo], h = tps[lo + 1] - tps[lo];
            seg[i] = lo;
            local[i] = u < h ? u : h;
        }
    }
}

// Second phase: one thread per output element.  blockIdx.z picks the array (0: q, 1: v, 2: a), so the derivative order is
// uniform in a workgroup; blockIdx.y walks the trajectories; blockIdx.x walks the n_per x width elements of one trajectory
// with consecutive lanes along a row (contiguous 8-byte stores).  The only division per element is a 32-bit one (the entry
// refuses n_per * width >= 2^31); addresses are formed in 64 bits.
__global__ __launch_bounds__(256) void spline_sample_kernel(const SplinePlan P, const long B, const long n_per, const int nseg,
                                                            const double *__restrict__ coef, const int *__restrict__ seg,
                                                            const double *__restrict__ local, const double *__restrict__ q0,
                                                            double *__restrict__ q, const long ldq, double *__restrict__ v,
                                                            double *__restrict__ a, const long ldv) {
    const int which = blockIdx.z;
    const unsigned width = which == 0 ? P.nq : P.nv;
    double *out = which == 0 ? q : which == 1 ? v : a;
    const long ld = which == 0 ? ldq : ldv;
    const unsigned total = (unsigned)n_per * width;
    for (long b = blockIdx.y; b < B; b += gridDim.y) {
        double *dst = out + b * n_per * ld;
        const double *cb = coef + 6 * b * nseg * P.n_act;
        for (unsigned e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
            const unsigned i = e / width, c = e - i * width;
            const int s = which == 0 ? P.qmap[c] : P.vmap[c];
            double r = which == 0 ? q0[c] : 0.0;  // columns no active joint owns: robot.q0 / +0.0
            if (s >= 0) {
                const double u = local[i];
                const double *k = cb + 6 * (seg[i] * P.n_act + s);
                if (which == 0) r = ((((k[5] * u + k[4]) * u + k[3]) * u + k[2]) * u + k[1]) * u + k[0];
                else if (which == 1) r = ((((5.0 * k[5]) * u + 4.0 * k[4]) * u + 3.0 * k[3]) * u + 2.0 * k[2]) * u + k[1];
                else r = (((20.0 * k[5]) * u + 12.0 * k[4]) * u + 6.0 * k[3]) * u + 2.0 * k[2];
            }
            dst[(long)i * ld + c] = r;
        }
    }
}

// np.concatenate((q_wp, v_act, tau_act), axis=None) of every trajectory: pure copies.  blockIdx.y walks the trajectories,
// blockIdx.x the n_con entries of a row of out with consecutive lanes along it; one 32-bit division per element (the entry
// refuses n_con >= 2^31).
__global__ __launch_bounds__(256) void excitation_constraints_kernel(const ConstraintPlan P, const long B, const long n_per,
                                                                     const int n_idx, const int *__restrict__ idx_wp,
                                                                     const double *__restrict__ q, const long ldq,
                                                                     const double *__restrict__ v, const long ldv,
                                                                     const double *__restrict__ tau, double *__restrict__ out,
                                                                     const long ld_out) {
    const unsigned n_act = P.n_act;
    const unsigned nq_part = (unsigned)n_idx * n_act, nv_part = (unsigned)n_per * n_act, n_con = nq_part + 2 * nv_part;
    for (long b = blockIdx.y; b < B; b += gridDim.y) {
        const double *qb = q + b * n_per * ldq, *vb = v + b * n_per * ldv, *tb = tau + b * n_per;
        for (unsigned c = blockIdx.x * 256 + threadIdx.x; c < n_con; c += gridDim.x * 256) {
            const unsigned part = c < nq_part ? 0 : c < nq_part + nv_part ? 1 : 2;
            const unsigned off = c - (part == 0 ? 0 : part == 1 ? nq_part : nq_part + nv_part);
            const unsigned i = off / n_act, k = off - i * n_act;
            double r;
            if (part == 0) r = qb[(long)idx_wp[i] * ldq + P.idxq[k]];          // p_f[idx_waypoints][:, act_idxq]
            else if (part == 1) r = vb[(long)i * ldv + P.idxv[k]];            // v_f[:, act_idxv]
            else r = tb[(long)P.idxv[k] * (B * n_per) + i];                   // tau[act_idxv[k] * Ns + i], batched layout
            out[b * ld_out + c] = r;
        }
    }
}

// The constraint Jacobian by difference quotients: J[i][j] = (C[hi_j][i] - C[lo_j][i]) / dx[j] with hi_j = 1 + j and lo_j =
// 0 (2-point) or 1 + n_var + j (3-point) -- one subtraction and one IEEE division, as NumPy rounds them.  A transposing
// kernel: a workgroup stages a tile of 32 rows of J x 32 stencil rows through LDS; C is read with consecutive lanes along i
// (runs of 32 doubles of one stencil row), J is written with consecutive lanes along j (runs of up to 32 doubles of one
// row of J).  The tile's rows are 33 doubles apart: lanes along i write 66 banks apart, lanes along j read neighbours.
// Tiles are walked by a capped grid; every address is formed in 64 bits; nothing outside [n_con, n_var) is touched.
constexpr int kDqTile = 32;
__global__ __launch_bounds__(256) void difference_quotients_kernel(const double *__restrict__ C, const long ldc, const long n_con,
                                                                   const int n_var, const int three_point,
                                                                   const double *__restrict__ dx, double *__restrict__ J,
                                                                   const long ldj) {
    __shared__ double tile[kDqTile][kDqTile + 1];
    const int fast = threadIdx.x & 31, slow = threadIdx.x >> 5;  // 32 x 8 threads, four passes over the tile
    const long tiles_i = (n_con + kDqTile - 1) / kDqTile, tiles_j = (n_var + kDqTile - 1) / kDqTile;
    for (long t = blockIdx.x; t < tiles_i * tiles_j; t += gridDim.x) {
        const long i0 = (t / tiles_j) * kDqTile;
        const int j0 = (int)(t % tiles_j) * kDqTile;
        for (int k = 0; k < kDqTile; k += 8) {
            const long i = i0 + fast;
            const int j = j0 + slow + k;
            if (i < n_con && j < n_var) {
                const long lo = three_point ? 1 + (long)n_var + j : 0;
                tile[fast][slow + k] = (C[(1 + (long)j) * ldc + i] - C[lo * ldc + i]) / dx[j];
            }
        }
        __syncthreads();
        for (int k = 0; k < kDqTile; k += 8) {
            const long i = i0 + slow + k;
            const int j = j0 + fast;
            if (i < n_con && j < n_var) J[i * ldj + j] = tile[slow + k][fast];
        }
        __syncthreads();
    }
}

// The active joints as columns.  FIGH_ERR_UNSUPPORTED for a joint that is not one revolute or prismatic degree of freedom,
// FIGH_ERR_INVALID for an index pair that is no joint of the model or is listed twice.
int check_active_joints(const DevModel &m, const int n_act, const int32_t *idxq, const int32_t *idxv) {
    for (int s = 0; s < n_act; ++s) {
        int found = 0;
        for (int j = 1; j < m.njoints && !found; ++j)
            if (m.idx_q[j] == idxq[s] && m.idx_v[j] == idxv[s]) found = j;
        FIGH_REQUIRE(found, "an active joint's (idx_q, idx_v) is no joint of the model");
        if (m.jtype[found] != FIGH_JT_REVOLUTE && m.jtype[found] != FIGH_JT_PRISMATIC) {
            set_error("spline: an active joint must be one revolute or prismatic degree of freedom (nq = nv = 1); a "
                      "continuous or free-flyer joint has no waypoint in joint coordinates");
            return FIGH_ERR_UNSUPPORTED;
        }
        for (int r = 0; r < s; ++r) FIGH_REQUIRE(idxq[r] != idxq[s], "an active joint is listed twice");
    }
    return FIGH_OK;
}

}  // namespace

extern "C" int figh_spline_sample(figh_model_t model, int64_t B, int n_wps, int n_act, int64_t n_per, double freq,
                                  const int32_t *h_act_idxq, const int32_t *h_act_idxv, const double *h_tps,
                                  const double *d_wps, const double *d_vel_wps, int64_t vel_stride, const double *d_acc_wps,
                                  int64_t acc_stride, const double *d_q0, double *d_q, int64_t ldq, double *d_v, double *d_a,
                                  int64_t ldv) {
    if (int rc = ensure_device()) return rc;  // (first: without a device no model handle exists either)
    FIGH_REQUIRE(model && h_act_idxq && h_act_idxv && h_tps && d_wps && d_vel_wps && d_acc_wps && d_q0 && d_q && d_v && d_a,
                 "NULL pointer");
    const DevModel &m = model->host;
    FIGH_REQUIRE(m.nq >= 1 && m.nq <= kMaxQ && m.nv >= 1 && m.nv <= kMaxV, "bad model");
    FIGH_REQUIRE(B >= 1 && n_wps >= 2 && n_per >= 1 && n_act >= 1 && n_act <= m.nv, "bad shape");
    FIGH_REQUIRE(ldq >= m.nq && ldv >= m.nv, "leading dimension below the width");
    const long per_traj = (long)n_per * (m.nq > m.nv ? m.nq : m.nv);
    FIGH_REQUIRE(per_traj < (1L << 31), "n_per * max(nq, nv) must stay below 2^31 (the kernel indexes a trajectory in 32 bits)");
    const long wp_set = (long)n_act * n_wps;
    FIGH_REQUIRE((vel_stride == 0 || vel_stride >= wp_set) && (acc_stride == 0 || acc_stride >= wp_set),
                 "the batch stride of the velocity / acceleration waypoints is 0 (one set for all) or at least n_act * n_wps");
    FIGH_REQUIRE(freq > 0.0 && freq < 1e300, "freq must be positive");
    for (int k = 0; k + 1 < n_wps; ++k) FIGH_REQUIRE(h_tps[k] < h_tps[k + 1], "time points must be strictly increasing");
    FIGH_REQUIRE(h_tps[0] - h_tps[0] == 0.0 && h_tps[n_wps - 1] - h_tps[n_wps - 1] == 0.0, "time points must be finite");
    if (int rc = check_active_joints(m, n_act, h_act_idxq, h_act_idxv)) return rc;
    SplinePlan P;
    P.nq = m.nq;
    P.nv = m.nv;
    P.n_act = n_act;
    for (int c = 0; c < kMaxQ; ++c) P.qmap[c] = -1;
    for (int c = 0; c < kMaxV; ++c) P.vmap[c] = -1;
    for (int s = 0; s < n_act; ++s) {
        P.qmap[h_act_idxq[s]] = (short)s;
        P.vmap[h_act_idxv[s]] = (short)s;
    }
    const int nseg = n_wps - 1;
    const long ncoef = (long)B * nseg * n_act;
    // one buffer: coefficients | local times | time points | segment indices
    const size_t doubles = 6 * (size_t)ncoef + (size_t)n_per + (size_t)n_wps;
    double *ws = (double *)workspace(8 * doubles + 4 * (size_t)n_per, kWsSplineTable);
    if (!ws) return FIGH_ERR_ALLOC;
    double *coef = ws, *local = coef + 6 * ncoef, *tps = local + n_per;
    int *seg = (int *)(tps + n_wps);
    ProfileScope scope("spline_sample");
    FIGH_HIP(hipMemcpyAsync(tps, h_tps, sizeof(double) * n_wps, hipMemcpyHostToDevice, stream()));
    hipLaunchKernelGGL(spline_prologue_kernel, dim3(capped_grid(ncoef + n_per, 256, kMaxGrid)), dim3(256), 0, stream(),
                       (long)B, n_wps, n_act, (long)n_per, 1.0 / freq, tps, d_wps, d_vel_wps, (long)vel_stride, d_acc_wps,
                       (long)acc_stride, coef, seg, local);
    hipLaunchKernelGGL(spline_sample_kernel, dim3(capped_grid(per_traj, 256, kMaxGrid), capped_grid_rows(B), 3), dim3(256), 0,
                       stream(), P, (long)B, (long)n_per, nseg, coef, seg, local, d_q0, d_q, (long)ldq, d_v, d_a, (long)ldv);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}

extern "C" int figh_excitation_constraints(figh_model_t model, int64_t B, int64_t n_per, int n_act, const int32_t *h_act_idxq,
                                           const int32_t *h_act_idxv, int n_idx, const int32_t *h_idx_waypoints,
                                           const double *d_q, int64_t ldq, const double *d_v, int64_t ldv, const double *d_tau,
                                           double *d_out, int64_t ld_out) {
    if (int rc = ensure_device()) return rc;
    FIGH_REQUIRE(model && h_act_idxq && h_act_idxv && d_q && d_v && d_tau && d_out, "NULL pointer");
    FIGH_REQUIRE(n_idx == 0 || h_idx_waypoints, "NULL waypoint sample list");
    const DevModel &m = model->host;
    FIGH_REQUIRE(m.nq >= 1 && m.nq <= kMaxQ && m.nv >= 1 && m.nv <= kMaxV, "bad model");
    FIGH_REQUIRE(B >= 1 && n_per >= 1 && n_act >= 1 && n_act <= m.nv && n_idx >= 0, "bad shape");
    const long n_con = (long)n_idx * n_act + 2 * (long)n_per * n_act;
    FIGH_REQUIRE(ldq >= m.nq && ldv >= m.nv && ld_out >= n_con, "leading dimension below the width");
    FIGH_REQUIRE(n_con < (1L << 31), "n_con must stay below 2^31 (the kernel indexes a row of the output in 32 bits)");
    for (int w = 0; w < n_idx; ++w)
        FIGH_REQUIRE(h_idx_waypoints[w] >= 0 && h_idx_waypoints[w] < n_per, "a waypoint sample index is outside [0, n_per)");
    if (int rc = check_active_joints(m, n_act, h_act_idxq, h_act_idxv)) return rc;
    ConstraintPlan P;
    P.n_act = n_act;
    for (int s = 0; s < kMaxV; ++s) P.idxq[s] = P.idxv[s] = 0;
    for (int s = 0; s < n_act; ++s) {
        P.idxq[s] = (short)h_act_idxq[s];
        P.idxv[s] = (short)h_act_idxv[s];
    }
    int *d_idx = (int *)workspace(4 * (size_t)(n_idx > 0 ? n_idx : 1), kWsConstraintIdx);
    if (!d_idx) return FIGH_ERR_ALLOC;
    ProfileScope scope("excitation_constraints");
    if (n_idx > 0) FIGH_HIP(hipMemcpyAsync(d_idx, h_idx_waypoints, sizeof(int) * n_idx, hipMemcpyHostToDevice, stream()));
    hipLaunchKernelGGL(excitation_constraints_kernel, dim3(capped_grid(n_con, 256, kMaxGrid), capped_grid_rows(B)), dim3(256),
                       0, stream(), P, (long)B, (long)n_per, n_idx, d_idx, d_q, (long)ldq, d_v, (long)ldv, d_tau, d_out,
                       (long)ld_out);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}

extern "C" int figh_difference_quotients(const double *d_C, int64_t ldc, int64_t n_con, int n_var, int scheme,
                                         const double *d_dx, double *d_J, int64_t ldj) {
    if (int rc = ensure_device()) return rc;
    FIGH_REQUIRE(d_C && d_dx && d_J, "NULL pointer");
    FIGH_REQUIRE(scheme == 2 || scheme == 3, "difference quotients: the scheme is 2 (forward) or 3 (central)");
    FIGH_REQUIRE(n_var >= 1 && n_con >= 1, "difference quotients: n_var and n_con must be at least 1");
    FIGH_REQUIRE(ldc >= n_con && ldj >= n_var, "leading dimension below the width");
    const long tiles = ((long)(n_con + kDqTile - 1) / kDqTile) * ((n_var + kDqTile - 1) / kDqTile);
    ProfileScope scope("difference_quotients");
    hipLaunchKernelGGL(difference_quotients_kernel, dim3(capped_grid(tiles, 1, kMaxGrid)), dim3(256), 0, stream(), d_C, (long)ldc,
                       (long)n_con, n_var, scheme == 3 ? 1 : 0, d_dx, d_J, (long)ldj);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}
