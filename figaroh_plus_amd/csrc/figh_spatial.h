// 3-vector / rotation helpers and the rigid-body step of the device kernels (fp64, 6-vectors are (linear, angular)).
#pragma once

#include <hip/hip_runtime.h>

#include "figh.h"

namespace figh {

__device__ __forceinline__ void cross3(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void rot(const double *R, const double *x, double *y) {  // y = R x
    y[0] = R[0] * x[0] + R[1] * x[1] + R[2] * x[2];
    y[1] = R[3] * x[0] + R[4] * x[1] + R[5] * x[2];
    y[2] = R[6] * x[0] + R[7] * x[1] + R[8] * x[2];
}
__device__ __forceinline__ void rotT(const double *R, const double *x, double *y) {  // y = R^T x
    y[0] = R[0] * x[0] + R[3] * x[1] + R[6] * x[2];
    y[1] = R[1] * x[0] + R[4] * x[1] + R[7] * x[2];
    y[2] = R[2] * x[0] + R[5] * x[1] + R[8] * x[2];
}
__device__ __forceinline__ void rodrigues(const double *a, double c, double s, double *R) {
    const double t = 1.0 - c;
    R[0] = 1.0 - t * (a[2] * a[2] + a[1] * a[1]);
    R[1] = t * a[0] * a[1] - s * a[2];
    R[2] = t * a[0] * a[2] + s * a[1];
    R[3] = t * a[0] * a[1] + s * a[2];
    R[4] = 1.0 - t * (a[2] * a[2] + a[0] * a[0]);
    R[5] = t * a[1] * a[2] - s * a[0];
    R[6] = t * a[0] * a[2] - s * a[1];
    R[7] = t * a[1] * a[2] + s * a[0];
    R[8] = 1.0 - t * (a[1] * a[1] + a[0] * a[0]);
}
__device__ __forceinline__ void matmul3(const double *A, const double *B, double *C) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ double sgn(double x) { return (double)((x > 0.0) - (x < 0.0)); }

// sin and cos of a joint angle.  Below 2^30 this is the device library's sincos of x itself (n = 0: the FMAs return x).
// From 2^30 on the library switches to another argument reduction, whose result on gfx950 was measured off by about
// |x| 2^-53 -- 1e-4 at 2^40 rad, every entry of W behind that joint with it (tests/test_regressor_entrywise.py, regime
// bigq).  Angles from 2^30 to 2^45 are therefore reduced here, x - n 2 pi with 2 pi as the sum of two doubles and one
// rounding per FMA: the reduced angle is good to 7e-16 absolutely, which is what the rotation entries are worth anyway.
// Branch-free and two temporaries, so that the kernels keep their register allocation.  Larger angles go to the
// library as they are.
__device__ __forceinline__ void sincos_angle(double x, double *s, double *c) {
    const double ax = fabs(x);
    const double n = (ax >= 0x1p30 && ax < 0x1p45) ? rint(x * 0x1.45f306dc9c883p-3) : 0.0;
    const double r = fma(-n, 0x1.1a62633145c07p-52, fma(-n, 0x1.921fb54442d18p+2, x));
    sincos(r, s, c);
}

// ---- the rigid-body step of a tree walk, written once (plain pointers, no DevModel).  regressor_tape_kernel keeps hand
// copies of the joint model and the forward step: see the comment there.

// rotation of the unit quaternion (x y z w), row-major
__device__ __forceinline__ void quat_to_rotation(const double x, const double y, const double z, const double w, double *R) {
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}

// The joint model M_j(q_j) = (Rj, pj) and, with RATES, the joint's own velocity and acceleration (vj, aj; unused otherwise).
// A single-dof joint takes x0 = q (cos q for a continuous joint), x1 = sin q (continuous only), xd, xdd; a free-flyer reads
// its q = [p, qx qy qz qw] and its v, a (joint frame) from qf, vf, af, `stride` doubles apart (1: sample-major inputs).
// Every branch writes every output and ends on the same element: with outputs preset by the caller the branches' last
// stores went to different elements, the compiler merged them into one store through a selected address, and the arrays
// behind it stayed in scratch (32 bytes per lane in inverse_dynamics_tree_kernel).
template <bool RATES>
__device__ __forceinline__ void joint_transform(const int jtype, const double *ax, const double x0, const double x1,
                                                const double xd, const double xdd, const double *qf, const double *vf,
                                                const double *af, const int stride, double *Rj, double *pj, double *vj,
                                                double *aj) {
    if (jtype == FIGH_JT_REVOLUTE || jtype == FIGH_JT_CONTINUOUS) {
        double s = x1, c = x0;
        if (jtype == FIGH_JT_REVOLUTE) sincos_angle(x0, &s, &c);
        rodrigues(ax, c, s, Rj);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            pj[d] = 0.0;
            if constexpr (RATES) {
                vj[d] = 0.0;
                aj[d] = 0.0;
                vj[3 + d] = ax[d] * xd;
                aj[3 + d] = ax[d] * xdd;
            }
        }
    } else if (jtype == FIGH_JT_PRISMATIC) {
#pragma unroll
        for (int d = 0; d < 9; ++d) Rj[d] = (d % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            pj[d] = ax[d] * x0;
            if constexpr (RATES) {
                vj[d] = ax[d] * xd;
                aj[d] = ax[d] * xdd;
                vj[3 + d] = 0.0;
                aj[3 + d] = 0.0;
            }
        }
    } else {
        quat_to_rotation(qf[3 * stride], qf[4 * stride], qf[5 * stride], qf[6 * stride], Rj);
#pragma unroll
        for (int d = 0; d < 3; ++d) pj[d] = qf[d * stride];
        if constexpr (RATES) {
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                vj[d] = vf[d * stride];
                aj[d] = af[d * stride];
            }
        }
    }
}

// motion of the parent seen from the child: (R, p) = child -> parent
__device__ __forceinline__ void motion_to_child(const double *R, const double *p, const double *lin, const double *ang,
                                                double *olin, double *oang) {
    double t1[3], t2[3];
    cross3(p, ang, t1);
#pragma unroll
    for (int d = 0; d < 3; ++d) t2[d] = lin[d] - t1[d];
    rotT(R, t2, olin);
    rotT(R, ang, oang);
}

// Forward step of a tree walk onto a joint (the first loop of pinocchio::computeJointTorqueRegressor / rnea): with
// liMi = (Rk, pk) = placement . M_j(q), (V, A) of the parent become (V, A) of the link, V = liMi^-1 V + vj,
// A = liMi^-1 A + aj + V x vj.  placement: 9 rotation entries, then the translation.
__device__ __forceinline__ void tree_forward_step(const double *placement, const double *Rj, const double *pj,
                                                  const double *vj, const double *aj, double *V, double *A, double *Rk,
                                                  double *pk) {
    matmul3(placement, Rj, Rk);
    rot(placement, pj, pk);
#pragma unroll
    for (int d = 0; d < 3; ++d) pk[d] += placement[9 + d];
    double Vk[6], Ak[6];
    motion_to_child(Rk, pk, V, V + 3, Vk, Vk + 3);
    motion_to_child(Rk, pk, A, A + 3, Ak, Ak + 3);
#pragma unroll
    for (int d = 0; d < 6; ++d) Vk[d] += vj[d];
    double c1[3], c2[3], c3[3];  // Vk x vj
    cross3(Vk + 3, vj, c1);
    cross3(Vk, vj + 3, c2);
    cross3(Vk + 3, vj + 3, c3);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        Ak[d] += aj[d] + c1[d] + c2[d];
        Ak[3 + d] += aj[3 + d] + c3[d];
    }
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        V[d] = Vk[d];
        A[d] = Ak[d];
    }
}

// J^T B for the body regressor B = bodyRegressor(v, a) of one link and a motion axis J = (Jl, Ja) expressed in the
// link frame, in closed form -- the ten entries of one row of pin.computeJointTorqueRegressor for that link, in
// FIGAROH's column order [Ixx Ixy Ixz Iyy Iyz Izz mx my mz m] (regressor.py:73-82).  acc = a_lin + w x v_lin,
// dw = a_ang, w = v_ang.  Equal to propagating the 6 x 10 body regressor up the chain and projecting it on the joint
// axis (validated to 1.6e-16 relative), with 5x fewer flops and no per-thread arrays.
__device__ __forceinline__ void axis_times_body_regressor(const double *Jl, const double *Ja, const double *acc,
                                                          const double *dw, const double *w, double *o) {
    o[9] = Jl[0] * acc[0] + Jl[1] * acc[1] + Jl[2] * acc[2];  // m
    double h1[3], h2[3], h3[3], h4[3];  // mx my mz: Jl x dw + w x (w x Jl) + acc x Ja
    cross3(Jl, dw, h1);
    cross3(w, Jl, h2);
    cross3(w, h2, h3);
    cross3(acc, Ja, h4);
    o[6] = h1[0] + h3[0] + h4[0];
    o[7] = h1[1] + h3[1] + h4[1];
    o[8] = h1[2] + h3[2] + h4[2];
    // inertia: L(dw)^T Ja - L(w)^T (w x Ja),  L(x)^T y = [x0y0, x1y0+x0y1, x1y1, x2y0+x0y2, x2y1+x1y2, x2y2]
    double u[3];
    cross3(w, Ja, u);
    o[0] = dw[0] * Ja[0] - w[0] * u[0];                                              // Ixx
    o[1] = dw[1] * Ja[0] + dw[0] * Ja[1] - (w[1] * u[0] + w[0] * u[1]);                // Ixy
    o[3] = dw[1] * Ja[1] - w[1] * u[1];                                              // Iyy
    o[2] = dw[2] * Ja[0] + dw[0] * Ja[2] - (w[2] * u[0] + w[0] * u[2]);                // Ixz
    o[4] = dw[2] * Ja[1] + dw[1] * Ja[2] - (w[2] * u[1] + w[1] * u[2]);                // Iyz
    o[5] = dw[2] * Ja[2] - w[2] * u[2];                                              // Izz
}

// ... for a pure translation axis (Ja = 0: the three force rows of the external-wrench regressor): the six rotational-inertia
// entries are exact zeros and mx my mz lose their acc x Ja term -- 40 instead of 110 flops.  o[0 .. 5] are not written.
__device__ __forceinline__ void axis_times_body_regressor_lin(const double *Jl, const double *acc, const double *dw,
                                                              const double *w, double *o) {
    o[9] = Jl[0] * acc[0] + Jl[1] * acc[1] + Jl[2] * acc[2];  // m
    double h1[3], h2[3], h3[3];                                 // mx my mz: Jl x dw + w x (w x Jl)
    cross3(Jl, dw, h1);
    cross3(w, Jl, h2);
    cross3(w, h2, h3);
    o[6] = h1[0] + h3[0];
    o[7] = h1[1] + h3[1];
    o[8] = h1[2] + h3[2];
}

}  // namespace figh
