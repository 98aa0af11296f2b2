// Geometric calibration on the device (src/figaroh/calibration/calibration_tools.py): the kinematic regressor and frame
// Jacobian over independent configurations (calculate_identifiable_kinematics_model, :1395-1466, with
// calculate_kinematics_model :1368-1392 and get_rel_kinreg / get_rel_jac :677-740 inside its loop), the updated forward
// kinematics of the Levenberg-Marquardt cost for a batch of parameter vectors (calc_updated_fkm, :1148-1331, its loop over
// the poses), and the order-preserving row gather behind the reference's zero-row deletion (:1451-1461).
//
// Conventions: 6-vectors are (linear, angular); a placement M = (R, p) maps child to parent coordinates;
// Ad(M) = [[R, skew(p) R], [0, R]]; A_j = oM_parent(j) . jointPlacement_j; oM_j = A_j . M_j(q_j); oMf = oM_jf . P_f.
//
// The regressor, one sample per lane, one wave per workgroup.  Everything follows from ONE walk from the frame down to the
// root with a single running placement X in registers:
//     X = P_f^-1;  at joint j:  X = oMf^-1 . oM_j            -> J's columns of j are Ad(X) . S_j
//                               X <- X . M_j(q_j)^-1 = oMf^-1 . A_j   -> R's block of j is Ad(X)
//                               X <- X . jointPlacement_j^-1 = oMf^-1 . oM_parent(j)
// For a start frame on another branch (get_sup_joints cases 2 and 3) the supporting joints of that branch get their blocks
// from a second, upward walk that starts from the X saved at the last joint both branches share.  Neither walk keeps
// per-joint state.  The blocks of up to two joints with consecutive ids (96 bytes of a row) or the Jacobian columns of up to
// twelve consecutive degrees of freedom are staged in LDS for the wave's 64 samples and swept out row by row, so a wave
// stores contiguous runs of every row, not 8-byte elements 64 rows apart.  Columns off the support are written by ONE
// hipMemset2DAsync per matrix ahead of the launch.  No atomics; the row sums of squares are summed per lane in walk order,
// whether or not the matrix itself is stored.
#include "figh_internal.h"
#include "figh_spatial.h"

using namespace figh;

namespace {

constexpr int kStageCols = 12;              // columns staged per run: two joint blocks, or twelve Jacobian columns
constexpr int kStageLd = kStageCols + 1;    // odd leading dimension of a staged row: lanes 26 dwords apart
constexpr long kMaxGrid = 1 << 20;          // workgroups per launch; the kernels loop over the rest

enum { kModeR = 0, kModeJ = 1, kModeJSub = 2 };

// One walk, by value (kernel-argument segment: every index into it is wave-uniform).  Step s visits joint[s]; want[s] != 0:
// the step's columns go to the staging tile at column lcol[s]; flush_w[s] != 0: after the step the first flush_w[s] staged
// columns are swept out to columns [flush_col[s], flush_col[s] + flush_w[s]) of the output.
struct KinWalk {
    int n;
    short joint[kMaxJoints];
    short flush_col[kMaxJoints];
    unsigned char want[kMaxJoints];
    unsigned char lcol[kMaxJoints];
    unsigned char flush_w[kMaxJoints];
};

struct KinPlan {
    KinWalk down;      // from the frame's joint towards the root
    KinWalk up;        // kModeR: from the last shared joint's child up the start branch
    int save_at;       // kModeR with an upward walk: X is saved after step save_at of `down` (-1: the initial X)
    double Pinv[12];   // P_f^-1
};

struct FkmPlan {
    int n_s, n_e;                  // joints of the start / end branch above the last joint both share, from it outwards
    short js[kMaxJoints], slot_s[kMaxJoints];  // slot: position in the chain list (updated placement) or -1 (the model's)
    short je[kMaxJoints], slot_e[kMaxJoints];
    double Ps[12], Pe[12];
};

__device__ __forceinline__ void matmul3T(const double *A, const double *B, double *C) {  // C = A B^T
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1] + A[3 * r + 2] * B[3 * c + 2];
}

// (R, p) <- (R, p) . (Rb, pb)^-1
__device__ __forceinline__ void mul_inverse(double *R, double *p, const double *Rb, const double *pb) {
    double Rn[9], t[3];
    matmul3T(R, Rb, Rn);
    rot(Rn, pb, t);
#pragma unroll
    for (int d = 0; d < 9; ++d) R[d] = Rn[d];
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] -= t[d];
}

// (R, p) <- (R, p) . (Rb, pb)
__device__ __forceinline__ void mul_right(double *R, double *p, const double *Rb, const double *pb) {
    double Rn[9], t[3];
    rot(R, pb, t);
    matmul3(R, Rb, Rn);
#pragma unroll
    for (int d = 0; d < 9; ++d) R[d] = Rn[d];
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] += t[d];
}

// M_j(q_j) of joint j of the model for the sample at qi.  (The outputs are preset although joint_transform writes all of
// them: without these stores the walk kernels and calib_fkm_kernel are allocated 1 .. 6 other VGPRs than before,
// profiles/rigid_body_ab.txt.)
__device__ __forceinline__ void joint_motion(const DevModel *M, const int j, const double *qi, double *Rj, double *pj) {
    const int jt = M->jtype[j], iq = M->idx_q[j];
    const double ax[3] = {M->axis[j][0], M->axis[j][1], M->axis[j][2]};
#pragma unroll
    for (int d = 0; d < 9; ++d) Rj[d] = (d % 4 == 0) ? 1.0 : 0.0;
    pj[0] = pj[1] = pj[2] = 0.0;
    // (sin q is read only where there is one: behind the q of the last joint the row ends)
    const double sin_q = jt == FIGH_JT_CONTINUOUS ? qi[iq + 1] : 0.0;
    joint_transform<false>(jt, ax, qi[iq], sin_q, 0.0, 0.0, qi + iq, nullptr, nullptr, 1, Rj, pj, nullptr, nullptr);
}

// Column c of Ad(X) for X = (R, p): c < 3: (R[:, c], 0); c >= 3: (p x R[:, c - 3], R[:, c - 3])
__device__ __forceinline__ void action_column(const double *R, const double *p, const int c, double *col) {
    const int k = c < 3 ? c : c - 3;
    const double r[3] = {R[k], R[3 + k], R[6 + k]};
    if (c < 3) {
        col[0] = r[0]; col[1] = r[1]; col[2] = r[2];
        col[3] = col[4] = col[5] = 0.0;
    } else {
        cross3(p, r, col);
        col[3] = r[0]; col[4] = r[1]; col[5] = r[2];
    }
}

// one 6-vector into the staging tile (measured components only) and into the row sums of squares
__device__ __forceinline__ void stage_column(double *tile, const int lane, const int col, const double *v, const int mask,
                                             double *sq) {
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if ((mask >> k) & 1) {
            tile[(k * 64 + lane) * kStageLd + col] = v[k];
            sq[k] += v[k] * v[k];
        }
}

// sweep columns [0, w) of the staged tile to columns [col0, col0 + w) of rows {m N + i0 + s}: consecutive lanes along a row
template <bool SUB>
__device__ __forceinline__ void sweep(const double *tile, const int lane, const int nvalid, const int w, const int col0,
                                      const int mask, const long N, const long i0, double *out, const long ld) {
    __syncthreads();
    const int total = nvalid * w;
    int m = 0;
    for (int k = 0; k < 6; ++k) {
        if (!((mask >> k) & 1)) continue;
        double *dst = out + ((long)m * N + i0) * ld + col0;
        for (int e = lane; e < total; e += 64) {
            const int s = e / w, c = e - s * w;
            const double v = tile[(k * 64 + s) * kStageLd + c];
            if (SUB) dst[(long)s * ld + c] -= v;
            else dst[(long)s * ld + c] = v;
        }
        ++m;
    }
    __syncthreads();
}

template <int MODE>
__global__ __launch_bounds__(64) void kinematic_walk_kernel(const DevModel *__restrict__ M, const KinPlan P, const long N,
                                                            const double *__restrict__ q, const long ldq, const int mask,
                                                            double *__restrict__ out, const long ld,
                                                            double *__restrict__ rowsq) {
    __shared__ double tile[6 * 64 * kStageLd];
    const int lane = threadIdx.x;
    const long ntiles = (N + 63) / 64;
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long i0 = t * 64;
        const int nvalid = (int)((N - i0) < 64 ? (N - i0) : 64);
        const double *qi = q + (i0 + (lane < nvalid ? lane : nvalid - 1)) * ldq;
        double sq[6] = {0, 0, 0, 0, 0, 0};
        double R[9], p[3], Rs[9], ps[3];
#pragma unroll
        for (int d = 0; d < 9; ++d) R[d] = Rs[d] = P.Pinv[d];
#pragma unroll
        for (int d = 0; d < 3; ++d) p[d] = ps[d] = P.Pinv[9 + d];
        for (int s = 0; s < P.down.n; ++s) {
            const int j = P.down.joint[s];
            double Rj[9], pj[3], col[6];
            joint_motion(M, j, qi, Rj, pj);
            if (MODE != kModeR) {  // X = oMf^-1 . oM_j: the Jacobian columns Ad(X) . S_j
                const int jt = M->jtype[j], lc = P.down.lcol[s];
                if (jt == FIGH_JT_FREEFLYER) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
                        action_column(R, p, c, col);
                        stage_column(tile, lane, lc + c, col, mask, sq);
                    }
                } else {
                    const double ax[3] = {M->axis[j][0], M->axis[j][1], M->axis[j][2]};
                    double ra[3];
                    rot(R, ax, ra);
                    if (jt == FIGH_JT_PRISMATIC) {
                        col[0] = ra[0]; col[1] = ra[1]; col[2] = ra[2];
                        col[3] = col[4] = col[5] = 0.0;
                    } else {
                        cross3(p, ra, col);
                        col[3] = ra[0]; col[4] = ra[1]; col[5] = ra[2];
                    }
                    stage_column(tile, lane, lc, col, mask, sq);
                }
            }
            mul_inverse(R, p, Rj, pj);  // X = oMf^-1 . A_j
            if (MODE == kModeR && P.down.want[s]) {
                const int lc = P.down.lcol[s];
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    action_column(R, p, c, col);
                    stage_column(tile, lane, lc + c, col, mask, sq);
                }
            }
            if (P.down.flush_w[s] && out)
                sweep<MODE == kModeJSub>(tile, lane, nvalid, P.down.flush_w[s], P.down.flush_col[s], mask, N, i0, out, ld);
            mul_inverse(R, p, M->placement[j], M->placement[j] + 9);  // X = oMf^-1 . oM_parent(j)
            if (MODE == kModeR && s == P.save_at) {
#pragma unroll
                for (int d = 0; d < 9; ++d) Rs[d] = R[d];
#pragma unroll
                for (int d = 0; d < 3; ++d) ps[d] = p[d];
            }
        }
        if (MODE == kModeR) {
            for (int s = 0; s < P.up.n; ++s) {  // Z = oMf^-1 . oM_c, up the start branch
                const int j = P.up.joint[s];
                double Rj[9], pj[3], col[6];
                mul_right(Rs, ps, M->placement[j], M->placement[j] + 9);  // Z = oMf^-1 . A_j
                if (P.up.want[s]) {
                    const int lc = P.up.lcol[s];
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
                        action_column(Rs, ps, c, col);
                        stage_column(tile, lane, lc + c, col, mask, sq);
                    }
                }
                if (P.up.flush_w[s] && out)
                    sweep<false>(tile, lane, nvalid, P.up.flush_w[s], P.up.flush_col[s], mask, N, i0, out, ld);
                if (s + 1 < P.up.n) {
                    joint_motion(M, j, qi, Rj, pj);
                    mul_right(Rs, ps, Rj, pj);  // Z = oMf^-1 . oM_j
                }
            }
        }
        if (rowsq && lane < nvalid) {
            int m = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if ((mask >> k) & 1) rowsq[(long)(m++) * N + i0 + lane] = sq[k];
        }
    }
}

// row sums of squares of a stored matrix, one row per thread, columns in order (the Jacobian between two frames, whose
// entries are differences of two walks)
__global__ __launch_bounds__(256) void row_sumsq_kernel(const double *__restrict__ W, const long rows, const int cols,
                                                        const long ld, double *__restrict__ out) {
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
        double s = 0.0;
        for (int c = 0; c < cols; ++c) s += W[r * ld + c] * W[r * ld + c];
        out[r] = s;
    }
}

__device__ __forceinline__ void load12(const double *src, double *R, double *p) {
#pragma unroll
    for (int d = 0; d < 9; ++d) R[d] = src[d];
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] = src[9 + d];
}

// The frame on top of `n` joints seen from the joint below them: prod_j (placement_j . M_j(q_j)) . P
__device__ __forceinline__ void branch_placement(const DevModel *M, const int n, const short *joints, const short *slots,
                                                 const double *__restrict__ pl_b, const double *P, const double *qi, double *R,
                                                 double *p) {
#pragma unroll
    for (int d = 0; d < 9; ++d) R[d] = (d % 4 == 0) ? 1.0 : 0.0;
    p[0] = p[1] = p[2] = 0.0;
    for (int s = 0; s < n; ++s) {
        const int j = joints[s];
        const double *pl = slots[s] >= 0 ? pl_b + 12 * slots[s] : M->placement[j];
        double Rj[9], pj[3];
        mul_right(R, p, pl, pl + 9);
        joint_motion(M, j, qi, Rj, pj);
        mul_right(R, p, Rj, pj);
    }
    mul_right(R, p, P, P + 9);
}

// lane = pose i, blockIdx.y = parameter vector b (looping over the rest): out[b ld_out + k N + i]
__global__ __launch_bounds__(256) void calib_fkm_kernel(const DevModel *__restrict__ M, const FkmPlan P, const long B, const long N,
                                                        const double *__restrict__ q, const long ldq, const int n_chain,
                                                        const double *__restrict__ placements, const double *__restrict__ wMo,
                                                        const double *__restrict__ eeMf, const int mask,
                                                        double *__restrict__ out, const long ld_out) {
    for (long b = blockIdx.y; b < B; b += gridDim.y) {
        const double *pl_b = placements + b * 12 * n_chain;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
            const double *qi = q + i * ldq;
            double Rs[9], ps[3], Re[9], pe[3];
            branch_placement(M, P.n_s, P.js, P.slot_s, pl_b, P.Ps, qi, Rs, ps);
            branch_placement(M, P.n_e, P.je, P.slot_e, pl_b, P.Pe, qi, Re, pe);
            double Rr[9], d[3], pr[3];  // cMs^-1 . cMe
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) Rr[3 * r + c] = Rs[r] * Re[c] + Rs[3 + r] * Re[3 + c] + Rs[6 + r] * Re[6 + c];
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = pe[k] - ps[k];
            rotT(Rs, d, pr);
            double R[9], p[3], Rt[9], pt[3];
            load12(wMo + 12 * b, R, p);
            mul_right(R, p, Rr, pr);
            load12(eeMf + 12 * b, Rt, pt);
            mul_right(R, p, Rt, pt);
            double loc[6] = {p[0], p[1], p[2], atan2(R[7], R[8]), atan2(-R[6], sqrt(R[0] * R[0] + R[3] * R[3])),
                             atan2(R[3], R[0])};
            int m = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if ((mask >> k) & 1) out[b * ld_out + (long)(m++) * N + i] = loc[k];
        }
    }
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const double *__restrict__ W, const long ldw, const int cols,
                                                          const int *__restrict__ idx, const long n, double *__restrict__ out,
                                                          const long ld_out) {
    const long total = n * cols;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / cols;
        const int c = (int)(e - r * cols);
        out[r * ld_out + c] = W[(long)idx[r] * ldw + c];
    }
}

void invert12(const double *P, double *out) {  // (R, p)^-1 = (R^T, -R^T p)
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[3 * r + c] = P[3 * c + r];
    for (int r = 0; r < 3; ++r) out[9 + r] = -(out[3 * r] * P[9] + out[3 * r + 1] * P[10] + out[3 * r + 2] * P[11]);
}

bool finite12(const double *P) {
    for (int d = 0; d < 12; ++d)
        if (!(P[d] - P[d] == 0.0)) return false;
    return true;
}

// joints from j down to the root's child
int branch_of(const DevModel &m, int j, short *out) {
    int n = 0;
    while (j > 0 && n < kMaxJoints) {
        out[n++] = (short)j;
        j = m.parents[j];
    }
    return n;
}

// Group the wanted steps of a walk into runs of consecutive output columns of at most kStageCols.  width[s]: the columns
// step s produces, first[s]: its first output column.  descending: the walk visits falling columns (towards the root).
void plan_runs(KinWalk &w, const int *first, const int *width, const bool descending) {
    int s = 0;
    while (s < w.n) {
        w.lcol[s] = 0;
        w.flush_w[s] = 0;
        w.flush_col[s] = 0;
        if (!w.want[s]) {
            ++s;
            continue;
        }
        int e = s, total = width[s];  // steps s .. e form one run
        while (e + 1 < w.n && w.want[e + 1] && total + width[e + 1] <= kStageCols &&
               (descending ? first[e + 1] + width[e + 1] == first[e] : first[e] + width[e] == first[e + 1])) {
            ++e;
            total += width[e];
        }
        const int col0 = descending ? first[e] : first[s];
        for (int k = s; k <= e; ++k) {
            w.lcol[k] = (unsigned char)(first[k] - col0);
            w.flush_w[k] = 0;
            w.flush_col[k] = 0;
        }
        w.flush_w[e] = (unsigned char)total;
        w.flush_col[e] = (short)col0;
        s = e + 1;
    }
}

int check_frame_args(const DevModel &m, const int end_joint, const double *h_end_placement, const int start_joint,
                     const double *h_start_placement, const int meas_mask) {
    FIGH_REQUIRE(m.njoints >= 2 && m.njoints <= kMaxJoints && m.nq >= 1 && m.nv >= 1, "bad model");
    FIGH_REQUIRE(end_joint >= 0 && end_joint < m.njoints, "the end joint is no joint of the model");
    FIGH_REQUIRE(start_joint >= -1 && start_joint < m.njoints, "the start joint is no joint of the model (-1: universe)");
    FIGH_REQUIRE(h_end_placement && finite12(h_end_placement), "the end frame's placement is NULL or not finite");
    FIGH_REQUIRE(start_joint < 0 || (h_start_placement && finite12(h_start_placement)),
                 "the start frame's placement is NULL or not finite");
    FIGH_REQUIRE(meas_mask >= 1 && meas_mask <= 63, "meas_mask selects one to six of the components x y z roll pitch yaw");
    return FIGH_OK;
}

}  // namespace

extern "C" int figh_kinematic_regressor(figh_model_t model, int64_t N, const double *d_q, int64_t ldq, int end_joint,
                                        const double *h_end_placement, int start_joint, const double *h_start_placement,
                                        const int32_t *h_support, int n_support, int meas_mask, double *d_R, int64_t ldr,
                                        double *d_J, int64_t ldj, double *d_rowsq_R, double *d_rowsq_J) {
    if (int rc = ensure_device()) return rc;  // (first: without a device no model handle exists either)
    FIGH_REQUIRE(model && d_q, "NULL pointer");
    const DevModel &m = model->host;
    if (int rc = check_frame_args(m, end_joint, h_end_placement, start_joint, h_start_placement, meas_mask)) return rc;
    FIGH_REQUIRE(N >= 1 && ldq >= m.nq, "bad shape, or the leading dimension of q is below nq");
    FIGH_REQUIRE(n_support >= 0 && n_support < kMaxJoints && (n_support == 0 || h_support), "bad support list");
    const int ncols_R = 6 * (m.njoints - 1);
    FIGH_REQUIRE(!d_R || ldr >= ncols_R, "leading dimension of R below 6 (njoints - 1)");
    FIGH_REQUIRE(!d_J || ldj >= m.nv, "leading dimension of J below nv");
    const bool want_R = d_R || d_rowsq_R, want_J = d_J || d_rowsq_J;
    short end_branch[kMaxJoints], start_branch[kMaxJoints];
    const int n_end = branch_of(m, end_joint, end_branch);
    const int n_start = start_joint > 0 ? branch_of(m, start_joint, start_branch) : 0;
    // the joints both branches share are the tails of the two lists
    int shared = 0;
    while (shared < n_end && shared < n_start && end_branch[n_end - 1 - shared] == start_branch[n_start - 1 - shared]) ++shared;
    bool in_support[kMaxJoints] = {};
    for (int k = 0; k < n_support; ++k) {
        const int p = h_support[k];
        FIGH_REQUIRE(p >= 1 && p < m.njoints, "a support joint is no joint of the model");
        bool on_path = false;
        for (int s = 0; s < n_end; ++s) on_path |= end_branch[s] == p;
        for (int s = 0; s < n_start; ++s) on_path |= start_branch[s] == p;
        FIGH_REQUIRE(on_path, "a support joint lies neither between the root and the end frame nor between the root and the "
                              "start frame");
        FIGH_REQUIRE(!in_support[p], "a support joint is listed twice");
        in_support[p] = true;
    }
    const int nmeas = __builtin_popcount((unsigned)meas_mask);
    const long rows = (long)nmeas * N;
    int first[kMaxJoints], width[kMaxJoints];
    const long ntiles = (N + 63) / 64;
    const unsigned grid = capped_grid(ntiles, 1, kMaxGrid);
    ProfileScope scope("kinematic_regressor");
    if (want_R) {
        KinPlan P = {};
        invert12(h_end_placement, P.Pinv);
        const int n_up = n_start - shared;  // the start branch above the last shared joint, walked from it outwards
        bool any_up = false;
        for (int s = 0; s < n_up; ++s) any_up |= in_support[start_branch[s]];
        // the walk stops behind the last step anything depends on
        int last = -1;
        for (int s = 0; s < n_end; ++s)
            if (in_support[end_branch[s]]) last = s;
        P.save_at = -1;
        if (any_up) {
            P.save_at = n_end - shared - 1;  // after the step of the end branch's first joint above the shared ones
            if (P.save_at > last) last = P.save_at;
        }
        P.down.n = last + 1;
        for (int s = 0; s < P.down.n; ++s) {
            P.down.joint[s] = end_branch[s];
            P.down.want[s] = in_support[end_branch[s]];
            first[s] = 6 * (end_branch[s] - 1);
            width[s] = 6;
        }
        plan_runs(P.down, first, width, true);
        if (any_up) {
            int n = 0;
            for (int s = n_up - 1; s >= 0; --s) {
                P.up.joint[n] = start_branch[s];
                P.up.want[n] = in_support[start_branch[s]];
                first[n] = 6 * (start_branch[s] - 1);
                width[n] = 6;
                ++n;
            }
            while (n > 0 && !P.up.want[n - 1]) --n;
            P.up.n = n;
            plan_runs(P.up, first, width, false);
        }
        // (d_R == NULL: the same walk, nothing stored, the sums of squares alone)
        if (d_R) FIGH_HIP(hipMemset2DAsync(d_R, sizeof(double) * ldr, 0, sizeof(double) * ncols_R, rows, stream()));
        hipLaunchKernelGGL(kinematic_walk_kernel<kModeR>, dim3(grid), dim3(64), 0, stream(), model->dev, P, (long)N, d_q,
                           (long)ldq, meas_mask, d_R, (long)ldr, d_rowsq_R);
    }
    if (want_J) {
        const bool relative = n_start > 0;
        if (!d_J && relative) {  // the sums of squares of a difference of two walks are taken from the stored difference
            d_J = (double *)workspace(sizeof(double) * (size_t)rows * m.nv, kWsKinematicJacobian);
            if (!d_J) return FIGH_ERR_ALLOC;
            ldj = m.nv;
        }
        if (d_J) FIGH_HIP(hipMemset2DAsync(d_J, sizeof(double) * ldj, 0, sizeof(double) * m.nv, rows, stream()));
        for (int pass = 0; pass < (relative ? 2 : 1); ++pass) {
            KinPlan P = {};
            invert12(pass == 0 ? h_end_placement : h_start_placement, P.Pinv);
            const short *branch = pass == 0 ? end_branch : start_branch;
            P.down.n = pass == 0 ? n_end : n_start;
            P.save_at = -2;
            for (int s = 0; s < P.down.n; ++s) {
                const int j = branch[s];
                P.down.joint[s] = (short)j;
                P.down.want[s] = 1;
                first[s] = m.idx_v[j];
                width[s] = m.jtype[j] == FIGH_JT_FREEFLYER ? 6 : 1;
            }
            plan_runs(P.down, first, width, true);
            if (pass == 0)
                hipLaunchKernelGGL(kinematic_walk_kernel<kModeJ>, dim3(grid), dim3(64), 0, stream(), model->dev, P, (long)N, d_q,
                                   (long)ldq, meas_mask, d_J, (long)ldj, relative ? nullptr : d_rowsq_J);
            else
                hipLaunchKernelGGL(kinematic_walk_kernel<kModeJSub>, dim3(grid), dim3(64), 0, stream(), model->dev, P, (long)N,
                                   d_q, (long)ldq, meas_mask, d_J, (long)ldj, (double *)nullptr);
        }
        if (relative && d_rowsq_J)
            hipLaunchKernelGGL(row_sumsq_kernel, dim3(capped_grid(rows, 256, kMaxGrid)), dim3(256), 0, stream(), d_J, rows,
                               m.nv, (long)ldj, d_rowsq_J);
    }
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}

extern "C" int figh_calib_fkm_batch(figh_model_t model, int64_t B, int64_t N, const double *d_q, int64_t ldq, int n_chain,
                                    const int32_t *h_chain, const double *d_placements, const double *d_wMo,
                                    const double *d_eeMf, int end_joint, const double *h_end_placement, int start_joint,
                                    const double *h_start_placement, int meas_mask, double *d_out, int64_t ld_out) {
    if (int rc = ensure_device()) return rc;
    FIGH_REQUIRE(model && d_q && d_wMo && d_eeMf && d_out, "NULL pointer");
    const DevModel &m = model->host;
    if (int rc = check_frame_args(m, end_joint, h_end_placement, start_joint, h_start_placement, meas_mask)) return rc;
    FIGH_REQUIRE(B >= 1 && N >= 1 && ldq >= m.nq, "bad shape, or the leading dimension of q is below nq");
    FIGH_REQUIRE(n_chain >= 0 && n_chain < kMaxJoints && (n_chain == 0 || (h_chain && d_placements)), "bad chain list");
    const int nmeas = __builtin_popcount((unsigned)meas_mask);
    FIGH_REQUIRE(ld_out >= (long)nmeas * N, "leading dimension of the output below n_meas N");
    short slot_of[kMaxJoints];
    for (int j = 0; j < kMaxJoints; ++j) slot_of[j] = -1;
    for (int k = 0; k < n_chain; ++k) {
        FIGH_REQUIRE(h_chain[k] >= 1 && h_chain[k] < m.njoints, "a chain joint is no joint of the model");
        FIGH_REQUIRE(slot_of[h_chain[k]] < 0, "a chain joint is listed twice");
        slot_of[h_chain[k]] = (short)k;
    }
    short end_branch[kMaxJoints], start_branch[kMaxJoints];
    const int n_end = branch_of(m, end_joint, end_branch);
    const int n_start = start_joint > 0 ? branch_of(m, start_joint, start_branch) : 0;
    int shared = 0;
    while (shared < n_end && shared < n_start && end_branch[n_end - 1 - shared] == start_branch[n_start - 1 - shared]) ++shared;
    FkmPlan P = {};
    for (int s = n_start - shared - 1; s >= 0; --s) {
        P.js[P.n_s] = start_branch[s];
        P.slot_s[P.n_s++] = slot_of[start_branch[s]];
    }
    for (int s = n_end - shared - 1; s >= 0; --s) {
        P.je[P.n_e] = end_branch[s];
        P.slot_e[P.n_e++] = slot_of[end_branch[s]];
    }
    for (int d = 0; d < 12; ++d) {
        P.Pe[d] = h_end_placement[d];
        P.Ps[d] = start_joint >= 0 ? h_start_placement[d] : (d < 9 && d % 4 == 0 ? 1.0 : 0.0);
    }
    ProfileScope scope("calib_fkm_batch");
    hipLaunchKernelGGL(calib_fkm_kernel, dim3(capped_grid(N, 256, kMaxGrid), capped_grid_rows(B)), dim3(256), 0, stream(),
                       model->dev, P, (long)B, (long)N, d_q, (long)ldq, n_chain, d_placements, d_wMo, d_eeMf, meas_mask, d_out,
                       (long)ld_out);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}

extern "C" int figh_gather_rows(const double *d_W, int64_t ldw, int cols, const int32_t *d_row_idx, int64_t n, double *d_out,
                                int64_t ld_out) {
    if (int rc = ensure_device()) return rc;
    FIGH_REQUIRE(n >= 0 && cols >= 1 && ldw >= cols && ld_out >= cols, "bad shape, or a leading dimension below the width");
    if (n == 0) return FIGH_OK;
    FIGH_REQUIRE(d_W && d_row_idx && d_out, "NULL pointer");
    ProfileScope scope("gather_rows");
    hipLaunchKernelGGL(gather_rows_kernel, dim3(capped_grid((long)n * cols, 256, kMaxGrid)), dim3(256), 0, stream(), d_W,
                       (long)ldw, cols, d_row_idx, (long)n, d_out, (long)ld_out);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}
