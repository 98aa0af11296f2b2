// Inverse dynamics on gfx950: tau = W(q, v, a) . phi without W (figh_regressor_apply).
//
// Replaces, for one parameter vector, build_regressor_basic followed by np.dot(W, phi): the pin.rnea loops of
// get_torque_rand (src/figaroh/tools/randomdata.py:93-147) and calc_torque (examples/tiago/utils/cubic_spline.py:448-455),
// and tau_base = np.dot(W_b, phi_b) of examples/staubli_TX40/identification.py:244 on a fresh trajectory.  Output in the
// reference's row order, row j*N + i; phi in the reference's column order, 14 entries per link
// [Ixx Ixy Ixz Iyy Iyz Izz mx my mz m Ia fv fs off] (+ the three TX40 coupling entries).
//
// One sample per lane, 64 consecutive samples per wavefront, model constants wave-uniform.  Recursive Newton-Euler with the
// wrench of a link in BODY-REGRESSOR form: with acc = a_lin + w x v_lin, h = (mx my mz),
//     force  = m acc + dw x h + w x (w x h)
//     moment = h x acc + I dw + w x (I w)
// which is bodyRegressor(V, A) . pi term by term -- every product is one the regressor kernels form as well, so the result
// carries the error scale of W . phi.  The spatial-momentum form I A + V x* (I V) forms v_lin x (m v_lin), zero only
// analytically: on the wheel rows of TIAGo at 2000 rad/s it is off by 2.3e3 u T (T: the a-priori scale of the row, see
// tests/dynamics_exact.py) where this form stays below 7.  The backward pass carries the wrench to the parent,
// f_p += X f_k, and projects it on the joint axis, tau_j = S_j^T f_j; the Ia / fv / fs / off and coupling columns are added
// per row from their inputs.  O(links) per sample, no atomics, bit-reproducible.
//
//  inverse_dynamics_chain_kernel<NJ, TX40>   fixed-base serial chains of NJ <= 8 revolute joints (ChainParams<NJ>, SGPRs).
//      Everything in registers: (cos, sin) and the wrench of every link, 8 NJ doubles; the rotation of a joint is formed
//      again from (cos, sin) on the way back.  tau leaves as NJ coalesced 512-byte runs per wave.  192 B per sample (UR10).
//
//  inverse_dynamics_tree_kernel   any flattened tree; joint torques, or the external wrench on a free-flyer root (the six
//      rows are the accumulated wrench of link 1 in its own frame; massless bodies and components outside ft_mask carry
//      no inertial term; Ia / fv / fs / off act on all six rows with v[i, k], a[i, k] of link index k, regressor.py:142-169).
//      What has to survive from the forward to the backward pass -- the wrench f_k and the child -> parent transform of
//      every link, 18 doubles, and the motion (V, A) of the links with a child that does not follow them directly, 12 doubles -- lives in the
//      wave's region of a library workspace slot, laid out [link][component][lane]: every access is one contiguous
//      512-byte line.  The grid is persistent (kDynWavesPerCu waves per CU at most, each looping over sample tiles), so
//      the workspace is bounded by the grid, never by N.  On the way back a wrench whose parent is the link in front of it
//      stays in registers; only branch points go through the parent's slot.
//
// All arithmetic is fp64.  6-vectors are (linear, angular).
#include <cmath>

#include "figh_internal.h"
#include "figh_spatial.h"
#include "figh_chain.h"

namespace figh {

namespace {

constexpr int kDynLinkState = 18;    // per link: wrench (6), rotation (9) and translation (3) of child -> parent
constexpr int kDynBranchState = 12;  // per link with several children: V (6), A (6)

// a link with a child that does not directly follow it in the numbering keeps its motion for that child: slot in the wave's
// branch region, -1 = none
struct DynPlan {
    int nbranch;
    int bslot[kMaxJoints];
};

// The launch rule of both kernels: one wave per workgroup, at most kDynWavesPerCu waves per compute unit, each looping over
// the sample tiles (figaroh_plus_amd/_lib.py regressor_apply_waves states the same rule for the tests).
constexpr int kDynWavesPerCu = 8;

// f = bodyRegressor(V, A) . pi for pi = [Ixx Ixy Ixz Iyy Iyz Izz mx my mz m] (wave-uniform)
__device__ __forceinline__ void link_wrench(const double *vl, const double *w, const double *al, const double *dw,
                                            const double *__restrict__ pi, double *f) {
    double t[3], acc[3];
    cross3(w, vl, t);
#pragma unroll
    for (int d = 0; d < 3; ++d) acc[d] = al[d] + t[d];
    const double h[3] = {pi[6], pi[7], pi[8]}, m = pi[9];
    double dwh[3], wh[3], wwh[3], hacc[3], Idw[3], Iw[3], wIw[3];
    cross3(dw, h, dwh);
    cross3(w, h, wh);
    cross3(w, wh, wwh);
    cross3(h, acc, hacc);
    Idw[0] = pi[0] * dw[0] + pi[1] * dw[1] + pi[2] * dw[2];
    Idw[1] = pi[1] * dw[0] + pi[3] * dw[1] + pi[4] * dw[2];
    Idw[2] = pi[2] * dw[0] + pi[4] * dw[1] + pi[5] * dw[2];
    Iw[0] = pi[0] * w[0] + pi[1] * w[1] + pi[2] * w[2];
    Iw[1] = pi[1] * w[0] + pi[3] * w[1] + pi[4] * w[2];
    Iw[2] = pi[2] * w[0] + pi[4] * w[1] + pi[5] * w[2];
    cross3(w, Iw, wIw);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        f[d] = m * acc[d] + dwh[d] + wwh[d];
        f[3 + d] = hacc[d] + Idw[d] + wIw[d];
    }
}

// wrench of the child seen from the parent: lin = R f_lin, ang = R f_ang + p x lin
__device__ __forceinline__ void wrench_to_parent(const double *R, const double *p, const double *f, double *o) {
    double t[3];
    rot(R, f, o);
    rot(R, f + 3, o + 3);
    cross3(p, o, t);
#pragma unroll
    for (int d = 0; d < 3; ++d) o[3 + d] += t[d];
}

// ---------------------------------------------------------------------------------------------- chain kernel
template <int NJ, bool TX40>
__global__ __launch_bounds__(64) void inverse_dynamics_chain_kernel(const ChainParams<NJ> P, const int flags, const long N,
                                                                    const double *__restrict__ q,
                                                                    const double *__restrict__ v,
                                                                    const double *__restrict__ a,
                                                                    const double *__restrict__ phi,
                                                                    double *__restrict__ tau) {
    const int lane = threadIdx.x;
    const long ntiles = (N + 63) / 64;
    const bool fric = flags & FIGH_FLAG_FRICTION, actin = flags & FIGH_FLAG_ACT_INERTIA, offs = flags & FIGH_FLAG_OFFSET;
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long i0 = t * 64;
        const int nvalid = (int)((N - i0) < 64 ? (N - i0) : 64);
        const long is = i0 + (lane < nvalid ? lane : nvalid - 1);
        double cs[NJ][2], f[NJ][6];
        {
            double vl[3] = {0, 0, 0}, om[3] = {0, 0, 0}, al[3] = {-P.g[0], -P.g[1], -P.g[2]}, da[3] = {0, 0, 0};
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                const double qk = q[is * NJ + k];
                const double qdk = v[is * NJ + k], qddk = a[is * NJ + k];
                double s, c;
                sincos_angle(qk, &s, &c);
                cs[k][0] = c;
                cs[k][1] = s;
                double Rj[9], R[9];
                rodrigues(P.axis[k], c, s, Rj);
                matmul3(P.Rp[k], Rj, R);
                double nvl[3], nom[3], nal[3], nda[3], t1[3], t2[3];
                motion_to_child(R, P.pp[k], vl, om, nvl, nom);
                motion_to_child(R, P.pp[k], al, da, nal, nda);
                const double vj[3] = {P.axis[k][0] * qdk, P.axis[k][1] * qdk, P.axis[k][2] * qdk};
#pragma unroll
                for (int d = 0; d < 3; ++d) nom[d] += vj[d];
                cross3(nvl, vj, t1);
                cross3(nom, vj, t2);
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    vl[d] = nvl[d];
                    om[d] = nom[d];
                    al[d] = nal[d] + t1[d];
                    da[d] = nda[d] + P.axis[k][d] * qddk + t2[d];
                }
                link_wrench(vl, om, al, da, phi + 14 * k, f[k]);
            }
        }
        double fc[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) fc[d] = f[NJ - 1][d];
#pragma unroll
        for (int k = NJ - 1; k >= 0; --k) {
            double tk = P.axis[k][0] * fc[3] + P.axis[k][1] * fc[4] + P.axis[k][2] * fc[5];
            // Ia fv fs off of the joint's own row (regressor.py:55-70); a flag that is off leaves phi's entry unread.  (qd, qdd
            // are read again here, from cache, instead of being held in registers across both passes)
            if (actin) tk += phi[14 * k + 10] * a[is * NJ + k];
            if (fric) {
                const double qdk = v[is * NJ + k];
                tk += phi[14 * k + 11] * qdk + phi[14 * k + 12] * sgn(qdk);
            }
            if (offs) tk += phi[14 * k + 13];
            if constexpr (TX40) {  // regressor.py:216-225: rows of joints 5 and 6 (0-based 4, 5)
                if (k == 4 || k == 5) {
                    const int o = k == 4 ? 5 : 4;
                    tk += phi[14 * NJ] * a[is * NJ + o] + phi[14 * NJ + 1] * v[is * NJ + o] +
                          phi[14 * NJ + 2] * sgn(v[is * NJ + 4] + v[is * NJ + 5]);
                }
            }
            if (lane < nvalid) tau[(long)k * N + i0 + lane] = tk;
            if (k > 0) {
                double Rj[9], R[9], up[6];
                // (formed again, not kept: without the barrier the compiler reuses the forward pass's rotation and holds nine
                // more doubles per link, 326 registers for six links)
                double c = cs[k][0], s = cs[k][1];
                asm volatile("" : "+v"(c), "+v"(s));
                rodrigues(P.axis[k], c, s, Rj);
                matmul3(P.Rp[k], Rj, R);
                wrench_to_parent(R, P.pp[k], fc, up);
#pragma unroll
                for (int d = 0; d < 6; ++d) fc[d] = f[k - 1][d] + up[d];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- tree kernel
// ws: this launch's workspace, ws_wave doubles per wave: [link][18][lane], then [branch slot][12][lane]
__global__ __launch_bounds__(64) void inverse_dynamics_tree_kernel(const DevModel *__restrict__ M, const DynPlan plan,
                                                                   const int extff, const int flags, const int ft_mask,
                                                                   const long N, const double *__restrict__ q,
                                                                   const double *__restrict__ v,
                                                                   const double *__restrict__ a,
                                                                   const double *__restrict__ phi, double *__restrict__ ws,
                                                                   const long ws_wave, double *__restrict__ tau) {
    const int lane = threadIdx.x;
    const int nj = M->njoints, nl = nj - 1, nq = M->nq, nv = M->nv;
    const bool fric = flags & FIGH_FLAG_FRICTION, actin = flags & FIGH_FLAG_ACT_INERTIA, offs = flags & FIGH_FLAG_OFFSET;
    const bool tx40 = flags & FIGH_FLAG_TX40;
    const double g0 = M->gravity[0], g1 = M->gravity[1], g2 = M->gravity[2];
    double *const st = ws + (long)blockIdx.x * ws_wave + lane;           // link k, component c: st[((k - 1) * 18 + c) * 64]
    double *const br = st + (long)nl * kDynLinkState * 64;               // branch slot s, component c: br[(s * 12 + c) * 64]
    const long ntiles = (N + 63) / 64;
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long i0 = t * 64;
        const int nvalid = (int)((N - i0) < 64 ? (N - i0) : 64);
        const long i = i0 + (lane < nvalid ? lane : nvalid - 1);
        const double *qi = q + i * nq, *vi = v + i * nv, *ai = a + i * nv;
        // ---- forward: motion of every link, its wrench and its transform to the workspace
        double V[6] = {0, 0, 0, 0, 0, 0}, A[6] = {0, 0, 0, 0, 0, 0};
        // inputs of the coming single-dof joint, requested one joint ahead: q (cos q for a continuous joint), sin q, qd, qdd
        double nx0 = 0.0, nx1 = 0.0, nxd = 0.0, nxdd = 0.0;
        auto fetch = [&](const int k) {
            if (k < nj && M->jtype[k] != FIGH_JT_FREEFLYER) {
                const int iq = M->idx_q[k], iv = M->idx_v[k];
                nx0 = qi[iq];
                nx1 = M->jtype[k] == FIGH_JT_CONTINUOUS ? qi[iq + 1] : 0.0;
                nxd = vi[iv];
                nxdd = ai[iv];
            }
        };
        fetch(1);
        for (int k = 1; k < nj; ++k) {
            const int jt = M->jtype[k], par = M->parents[k];
            const double jq0 = nx0, jq1 = nx1, jqd = nxd, jqdd = nxdd;
            fetch(k + 1);
            if (par == 0) {
#pragma unroll
                for (int d = 0; d < 6; ++d) V[d] = A[d] = 0.0;
                A[0] = -g0;
                A[1] = -g1;
                A[2] = -g2;
            } else if (par != k - 1) {  // a later child of a branch link
                const double *b = br + (long)plan.bslot[par] * kDynBranchState * 64;
#pragma unroll
                for (int d = 0; d < 6; ++d) {
                    V[d] = b[d * 64];
                    A[d] = b[(6 + d) * 64];
                }
            }
            const double ax[3] = {M->axis[k][0], M->axis[k][1], M->axis[k][2]};
            double Rj[9], pj[3], vj[6], aj[6];
            const int iq = M->idx_q[k], iv = M->idx_v[k];
            joint_transform<true>(jt, ax, jq0, jq1, jqd, jqdd, qi + iq, vi + iv, ai + iv, 1, Rj, pj, vj, aj);
            double Rk[9], pk[3];  // liMi = placement * M_joint(q)
            tree_forward_step(M->placement[k], Rj, pj, vj, aj, V, A, Rk, pk);
            if (plan.bslot[k] >= 0) {
                double *b = br + (long)plan.bslot[k] * kDynBranchState * 64;
#pragma unroll
                for (int d = 0; d < 6; ++d) {
                    b[d * 64] = V[d];
                    b[(6 + d) * 64] = A[d];
                }
            }
            double f[6] = {0, 0, 0, 0, 0, 0};
            // external wrench: massless bodies are skipped (regressor.py:36-39)
            if (!extff || M->body_mask[k]) link_wrench(V, V + 3, A, A + 3, phi + 14 * (k - 1), f);
            double *s = st + (long)(k - 1) * kDynLinkState * 64;
#pragma unroll
            for (int d = 0; d < 6; ++d) s[d * 64] = f[d];
#pragma unroll
            for (int d = 0; d < 9; ++d) s[(6 + d) * 64] = Rk[d];
#pragma unroll
            for (int d = 0; d < 3; ++d) s[(15 + d) * 64] = pk[d];
        }
        // ---- backward: f_parent += X f_k, tau_j = S_j^T f_j
        double fc[6] = {0, 0, 0, 0, 0, 0};
        bool have = false;  // fc already is the accumulated wrench of link k (its only pending child was k + 1)
        for (int k = nj - 1; k >= 1; --k) {
            const double *s = st + (long)(k - 1) * kDynLinkState * 64;
            if (!have) {
#pragma unroll
                for (int d = 0; d < 6; ++d) fc[d] = s[d * 64];
            }
            const int par = M->parents[k];
            if (!extff) {
                const int jt = M->jtype[k], iv = M->idx_v[k];
                const int o = jt == FIGH_JT_PRISMATIC ? 0 : 3;
                double tk = M->axis[k][0] * fc[o] + M->axis[k][1] * fc[o + 1] + M->axis[k][2] * fc[o + 2];
                const double *pe = phi + 14 * (k - 1) + 10;  // Ia fv fs off: the joint's own row (regressor.py:55-70)
                if (actin) tk += pe[0] * ai[iv];
                if (fric) {
                    const double vv = vi[iv];
                    tk += pe[1] * vv + pe[2] * sgn(vv);
                }
                if (offs) tk += pe[3];
                if (tx40 && (iv == 4 || iv == 5)) {  // regressor.py:216-225
                    const int oo = iv == 4 ? 5 : 4;
                    tk += phi[14 * nl] * ai[oo] + phi[14 * nl + 1] * vi[oo] + phi[14 * nl + 2] * sgn(vi[4] + vi[5]);
                }
                if (lane < nvalid) tau[(long)iv * N + i0 + lane] = tk;
            }
            have = false;
            if (par > 0) {
                double Rk[9], pk[3], up[6];
#pragma unroll
                for (int d = 0; d < 9; ++d) Rk[d] = s[(6 + d) * 64];
#pragma unroll
                for (int d = 0; d < 3; ++d) pk[d] = s[(15 + d) * 64];
                wrench_to_parent(Rk, pk, fc, up);
                double *sp = st + (long)(par - 1) * kDynLinkState * 64;
#pragma unroll
                for (int d = 0; d < 6; ++d) fc[d] = sp[d * 64] + up[d];
                if (par == k - 1) {
                    have = true;  // the parent comes next and has no other child left: its wrench stays in registers
                } else {
#pragma unroll
                    for (int d = 0; d < 6; ++d) sp[d * 64] = fc[d];
                }
            }
        }
        if (extff) {
            // fc: the accumulated wrench of link 1 in its own frame -- the six rows; Ia / fv / fs / off of every link on all
            // six of them, with v[i, k], a[i, k] of LINK index k (regressor.py:142-169)
            double ex = 0.0;
            if (actin || fric || offs) {
                for (int b = 0; b < nl; ++b) {
                    const double *pe = phi + 14 * b + 10;
                    if (actin) ex += pe[0] * ai[b];
                    if (fric) {
                        const double vv = vi[b];
                        ex += pe[1] * vv + pe[2] * sgn(vv);
                    }
                    if (offs) ex += pe[3];
                }
            }
            if (lane < nvalid) {
#pragma unroll
                for (int c = 0; c < 6; ++c) tau[(long)c * N + i0 + lane] = (((ft_mask >> c) & 1) ? fc[c] : 0.0) + ex;
            }
        }
    }
}

template <int NJ, bool TX40>
int launch_dynamics_chain(const figh_model_s *m, int flags, long N, long waves, const double *q, const double *v,
                          const double *a, const double *phi, double *tau) {
    const ChainParams<NJ> P = chain_params<NJ>(m);
    ProfileScope scope("inverse_dynamics", true);
    FIGH_LAUNCH_TIMED((inverse_dynamics_chain_kernel<NJ, TX40>), dim3((unsigned)waves), dim3(64), 0, P, flags, N, q, v, a, phi,
                      tau);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}

}  // namespace

int launch_inverse_dynamics(const figh_model_s *m, int mode, int flags, int ft_mask, long N, const double *q, const double *v,
                            const double *a, const double *phi, double *tau) {
    const DevModel &h = m->host;
    const long ntiles = (N + 63) / 64;
    long waves = (long)kDynWavesPerCu * cu_count();
    if (waves > ntiles) waves = ntiles;
    if (waves < 1) waves = 1;
    const bool tx40 = flags & FIGH_FLAG_TX40;
    if (m->is_chain && mode == FIGH_MODE_JOINT_TORQUE && !(flags & FIGH_FLAG_GENERIC)) {
        const int f = flags & 7;
        switch (h.nlinks) {
#define FIGH_DYN_CASE(NJ) \
    case NJ:              \
        return launch_dynamics_chain<NJ, false>(m, f, N, waves, q, v, a, phi, tau);
            FIGH_DYN_CASE(1)
            FIGH_DYN_CASE(2)
            FIGH_DYN_CASE(3)
            FIGH_DYN_CASE(4)
            FIGH_DYN_CASE(5)
            case 6:
                return tx40 ? launch_dynamics_chain<6, true>(m, f, N, waves, q, v, a, phi, tau)
                            : launch_dynamics_chain<6, false>(m, f, N, waves, q, v, a, phi, tau);
            FIGH_DYN_CASE(7)
            FIGH_DYN_CASE(8)
#undef FIGH_DYN_CASE
            default:
                break;  // (is_chain implies 1 .. 8 links)
        }
    }
    DynPlan plan;
    plan.nbranch = 0;
    for (int k = 0; k < kMaxJoints; ++k) plan.bslot[k] = -1;
    for (int k = 2; k < h.njoints; ++k) {
        const int par = h.parents[k];
        if (par > 0 && par != k - 1 && plan.bslot[par] < 0) plan.bslot[par] = plan.nbranch++;
    }
    const long ws_wave = 64L * ((long)kDynLinkState * h.nlinks + (long)kDynBranchState * plan.nbranch);
    double *ws = static_cast<double *>(workspace(sizeof(double) * (size_t)ws_wave * (size_t)waves, kWsDynamicsState));
    if (!ws) return FIGH_ERR_ALLOC;
    const int extff = mode == FIGH_MODE_EXT_WRENCH;
    ProfileScope scope("inverse_dynamics", true);
    FIGH_LAUNCH_TIMED(inverse_dynamics_tree_kernel, dim3((unsigned)waves), dim3(64), 0, m->dev, plan, extff,
                      flags & (7 | FIGH_FLAG_TX40), ft_mask, N, q, v, a, phi, ws, ws_wave, tau);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}

}  // namespace figh
