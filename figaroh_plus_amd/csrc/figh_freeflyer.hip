// The floating-base half of the real-data chain (examples/human/identification.py): the three per-sample Python loops the
// script puts around the filters and the regressor.
//   - :330-339  pin.log3(pin.Quaternion(q[3:7])) of every sample                        -> figh_quat_log
//   - :349-364  pin.Quaternion(pin.exp3(rotvec)) with the sign chosen against the raw
//               quaternion of the same row                                              -> figh_rotvec_to_quat
//   - :434-453  pin.Force(F).se3ActionInverse(oMi[root_joint]) stored as tau[j N + i],
//     :471-555  se3Action of the simulated and identified wrenches                      -> figh_wrench_transport
// All three are parallel in time, one lane per sample, fp64, no atomics, no LDS allocation.  The translation unit is compiled
// without FMA contraction: every statement below is one rounding per operation, in the order written, and the NumPy mirrors
// (identification/identification_tools.py) repeat them element by element.  The device differs from the mirrors only through
// the math library (sqrt, atan2, sincos); the transport over a path of free-flyers and constant placements calls none of
// them and is bit-equal.
//
// figh_quat_log.  n = sqrt((x x + y y) + z z), s = w < 0 ? -1 : +1, t = n / |w|.
//     n == 0:            r = (+0, +0, +0)
//     n < 2^-13 |w|:     f = 2 ((1 - t^2 / 3) + t^4 / 5) / |w|      (atan(t) / t; the next term, t^6 / 7, is below 2^-80)
//     otherwise:         f = 2 atan2(n, |w|) / n
//     r = (s f) (x, y, z)
// The threshold is on n relative to |w| (2^-13 for a unit quaternion): the series is the one of atan(t) / t and stays valid
// for a quaternion that is not normalised.
//
// figh_rotvec_to_quat.  th = sqrt((rx rx + ry ry) + rz rz).
//     th < 2^-13:        a = (1/2 - th^2 / 48) + th^4 / 3840,  c = (1 - th^2 / 8) + th^4 / 384   (next terms below 2^-90)
//     otherwise:         a = sin(th / 2) / th,                  c = cos(th / 2)
//     q^ = (a rx, a ry, a rz, c)
//     Eigen's representative:  |c| > 1/2: sE = c > 0 ? 1 : -1;  else i = 0; if |q^_1| > |q^_0|: i = 1; if |q^_2| > |q^_i|: i = 2
//                              (strict comparisons: the first of equal components wins, as in Eigen); sE = q^_i < 0 ? -1 : 1
//     d = sE ((((q^_0 ref_0) + q^_1 ref_1) + q^_2 ref_2) + q^_3 ref_3);  keep sE q^ iff d > 0.7071067811865476, else -sE q^.
// The reference negates when rounding makes d > 1 (its arccos is NaN); here that case keeps (include/figh.h).
//
// figh_wrench_transport.  (R, p) = oMi[joint]: for the joints j of the support path, root first,
//     (Rk, pk) = placement_j . M_j(q_j)   (matmul3, rot + translation: tree_forward_step's statements),
//     (R, p) = (Rk, pk) for the first joint, else (R Rk, p + R pk).
//     action:          f' = R f,     n' = R n + p x f'
//     inverse action:  f' = R^T f,   n' = R^T (n - p x f)
// A wave takes 64 consecutive samples.  In the stacked layout lane i reads and writes element k N + i0 + i of every
// component: consecutive lanes, consecutive addresses.  In the sample layout the 384 doubles of the tile are one contiguous
// run: the wave loads (stores) it as six rows of 64 consecutive doubles and moves every value to (from) the lane of its
// sample with wave shuffles -- two per component and direction, no LDS allocation, and no 48-byte-strided access.
#include "figh_internal.h"
#include "figh_spatial.h"

using namespace figh;

namespace {

constexpr long kMaxGrid = 1 << 16;        // workgroups per launch; every kernel loops over what is left
constexpr double kSeriesBelow = 0x1p-13;  // both series (the header comment states them)
constexpr double kKeepAbove = 0.7071067811865476;  // cos(pi / 4): 2 acos(d) < pi / 2

__global__ __launch_bounds__(256) void quat_log_kernel(const double *__restrict__ quat, const long N, const long ldq,
                                                       double *__restrict__ rotvec, const long ldr) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
        const double *qi = quat + i * ldq;
        const double x = qi[0], y = qi[1], z = qi[2], w = qi[3];
        const double n = sqrt((x * x + y * y) + z * z), aw = fabs(w);
        const double s = w < 0.0 ? -1.0 : 1.0;
        double f;
        if (n < kSeriesBelow * aw) {
            const double t = n / aw, t2 = t * t;
            f = 2.0 * ((1.0 - t2 / 3.0) + (t2 * t2) / 5.0) / aw;
        } else {
            f = 2.0 * atan2(n, aw) / n;
        }
        const double sf = s * f;
        double *r = rotvec + i * ldr;
        const bool zero = n == 0.0;
        r[0] = zero ? 0.0 : sf * x;
        r[1] = zero ? 0.0 : sf * y;
        r[2] = zero ? 0.0 : sf * z;
    }
}

// out may be ref itself (same pointer, same leading dimension; neither is __restrict__): the lane reads its row of ref before
// it writes it
__global__ __launch_bounds__(256) void rotvec_to_quat_kernel(const double *__restrict__ rotvec, const long N, const long ldr,
                                                             const double *ref, const long ldref, double *out,
                                                             const long ldo) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
        const double *ri = rotvec + i * ldr, *fi = ref + i * ldref;
        const double rx = ri[0], ry = ri[1], rz = ri[2];
        const double f0 = fi[0], f1 = fi[1], f2 = fi[2], f3 = fi[3];
        const double th2 = (rx * rx + ry * ry) + rz * rz, th = sqrt(th2);
        double a, c;
        if (th < kSeriesBelow) {
            const double th4 = th2 * th2;
            a = (0.5 - th2 / 48.0) + th4 / 3840.0;
            c = (1.0 - th2 / 8.0) + th4 / 384.0;
        } else {
            double sh;
            sincos(0.5 * th, &sh, &c);
            a = sh / th;
        }
        const double q0 = a * rx, q1 = a * ry, q2 = a * rz;
        double lead;  // the component Eigen's conversion makes positive
        if (fabs(c) > 0.5) {
            lead = c;
        } else {
            lead = q0;
            if (fabs(q1) > fabs(lead)) lead = q1;
            if (fabs(q2) > fabs(lead)) lead = q2;
        }
        const double sE = lead < 0.0 ? -1.0 : 1.0;
        const double d = sE * (((q0 * f0 + q1 * f1) + q2 * f2) + c * f3);
        const double sg = d > kKeepAbove ? sE : -sE;
        double *o = out + i * ldo;
        o[0] = sg * q0;
        o[1] = sg * q1;
        o[2] = sg * q2;
        o[3] = sg * c;
    }
}

// the support path of the joint, root first, by value (kernel-argument segment: every index into it is wave-uniform)
constexpr int kMaxPath = kMaxJoints;
struct WrenchPath {
    int n;
    short joint[kMaxPath];
};

// (R, p) <- (R, p) . (Rb, pb)
__device__ __forceinline__ void compose_right(double *R, double *p, const double *Rb, const double *pb) {
    double Rn[9], t[3];
    rot(R, pb, t);
    matmul3(R, Rb, Rn);
#pragma unroll
    for (int d = 0; d < 9; ++d) R[d] = Rn[d];
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] += t[d];
}

// The sample layout of a tile: element e = 6 l + k of the 384 is component k of sample l, and lane s of row r of the tile
// holds element 64 r + s.  6 l = s - k (mod 64) has no solution when s - k is odd and the two solutions l0 and l0 + 32
// otherwise, l0 = 11 (s - k) / 2 (mod 32) (3 . 11 = 1 mod 32); their elements lie in rows r0 = (6 l0 + k) / 64 <= 2 and r0 + 3
// (6 . 32 = 3 . 64).  So every component moves with two shuffles, one per half of the wave.
__device__ __forceinline__ int asker(const int s, const int k) { return (11 * (((s - k) & 63) >> 1)) & 31; }

template <bool IN_SAMPLE, bool OUT_SAMPLE, bool INVERSE>
__global__ __launch_bounds__(256) void wrench_transport_kernel(const DevModel *__restrict__ M, const WrenchPath P, const long N,
                                                               const double *__restrict__ q, const long ldq,
                                                               const double *__restrict__ F, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long ntiles = (N + 63) / 64, wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    for (long t = wave; t < ntiles; t += nwaves) {  // (wave-uniform bounds: every lane of a wave takes part in the shuffles)
        const long i0 = t * 64;
        const int nvalid = (int)((N - i0) < 64 ? (N - i0) : 64);
        const bool valid = lane < nvalid;
        double f[6];
        if constexpr (IN_SAMPLE) {
            const double *src = F + i0 * 6;
            double row[6];
#pragma unroll
            for (int r = 0; r < 6; ++r) row[r] = (r * 64 + lane) < 6 * nvalid ? src[r * 64 + lane] : 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                // as a source: the lanes that want this lane's element for their component k are l0 and l0 + 32, and they
                // want rows r0 and r0 + 3 of it; as a destination: component k of sample `lane` is element 6 lane + k
                const int l0 = asker(lane, k), r0 = (6 * l0 + k) >> 6, src = (6 * lane + k) & 63;
                const double lo = __shfl(r0 == 0 ? row[0] : r0 == 1 ? row[1] : row[2], src);
                const double hi = __shfl(r0 == 0 ? row[3] : r0 == 1 ? row[4] : row[5], src);
                f[k] = lane < 32 ? lo : hi;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) f[k] = valid ? F[(long)k * N + i0 + lane] : 0.0;
        }
        const double *qi = q + (i0 + (valid ? lane : nvalid - 1)) * ldq;
        double R[9], p[3];
#pragma unroll
        for (int d = 0; d < 9; ++d) R[d] = (d % 4 == 0) ? 1.0 : 0.0;
        p[0] = p[1] = p[2] = 0.0;
        for (int s = 0; s < P.n; ++s) {
            const int j = P.joint[s], jt = M->jtype[j], iq = M->idx_q[j];
            const double ax[3] = {M->axis[j][0], M->axis[j][1], M->axis[j][2]};
            double Rj[9], pj[3], Rk[9], pk[3];
            // (preset as joint_motion of figh_kinematics.hip presets them: joint_transform writes every output in every
            // branch, but without these stores the compiler left pj[0] and pj[1] of a continuous joint undefined)
#pragma unroll
            for (int d = 0; d < 9; ++d) Rj[d] = (d % 4 == 0) ? 1.0 : 0.0;
            pj[0] = pj[1] = pj[2] = 0.0;
            // (sin q is read only where there is one: behind the q of the last joint the row ends)
            const double sin_q = jt == FIGH_JT_CONTINUOUS ? qi[iq + 1] : 0.0;
            joint_transform<false>(jt, ax, qi[iq], sin_q, 0.0, 0.0, qi + iq, nullptr, nullptr, 1, Rj, pj, nullptr, nullptr);
            const double *pl = M->placement[j];
            matmul3(pl, Rj, Rk);
            rot(pl, pj, pk);
#pragma unroll
            for (int d = 0; d < 3; ++d) pk[d] += pl[9 + d];
            if (s == 0) {
#pragma unroll
                for (int d = 0; d < 9; ++d) R[d] = Rk[d];
#pragma unroll
                for (int d = 0; d < 3; ++d) p[d] = pk[d];
            } else {
                compose_right(R, p, Rk, pk);
            }
        }
        double o[6];
        if constexpr (INVERSE) {
            double c[3], m[3];
            cross3(p, f, c);
#pragma unroll
            for (int d = 0; d < 3; ++d) m[d] = f[3 + d] - c[d];
            rotT(R, f, o);
            rotT(R, m, o + 3);
        } else {
            double c[3], m[3];
            rot(R, f, o);
            rot(R, f + 3, m);
            cross3(p, o, c);
#pragma unroll
            for (int d = 0; d < 3; ++d) o[3 + d] = m[d] + c[d];
        }
        if constexpr (OUT_SAMPLE) {
            double *dst = out + i0 * 6;
            double row[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                // component k of samples l0 and l0 + 32 are the elements of rows r0 and r0 + 3 that this lane stores
                const int l0 = asker(lane, k), r0 = (6 * l0 + k) >> 6;
                const double lo = __shfl(o[k], l0), hi = __shfl(o[k], l0 + 32);
                if (((lane - k) & 1) == 0) {
                    row[0] = r0 == 0 ? lo : row[0];
                    row[1] = r0 == 1 ? lo : row[1];
                    row[2] = r0 == 2 ? lo : row[2];
                    row[3] = r0 == 0 ? hi : row[3];
                    row[4] = r0 == 1 ? hi : row[4];
                    row[5] = r0 == 2 ? hi : row[5];
                }
            }
#pragma unroll
            for (int r = 0; r < 6; ++r)
                if (r * 64 + lane < 6 * nvalid) dst[r * 64 + lane] = row[r];
        } else {
            if (valid) {
#pragma unroll
                for (int k = 0; k < 6; ++k) out[(long)k * N + i0 + lane] = o[k];
            }
        }
    }
}

// [a, a + na) and [b, b + nb) doubles share an address
bool overlap(const double *a, long na, const double *b, long nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 8 * (uintptr_t)na, b0 = (uintptr_t)b, b1 = b0 + 8 * (uintptr_t)nb;
    return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" int figh_quat_log(const double *d_quat, int64_t N, int64_t ld_quat, double *d_rotvec, int64_t ld_rotvec) {
    FIGH_REQUIRE(d_quat && d_rotvec, "NULL pointer");
    FIGH_REQUIRE(N >= 1, "quat_log: at least one sample");
    FIGH_REQUIRE(ld_quat >= 4 && ld_rotvec >= 3, "quat_log: a leading dimension below the width (4 in, 3 out)");
    FIGH_REQUIRE(!overlap(d_quat, (N - 1) * ld_quat + 4, d_rotvec, (N - 1) * ld_rotvec + 3), "quat_log: output overlaps input");
    if (int rc = ensure_device()) return rc;
    ProfileScope scope("quat_log");
    hipLaunchKernelGGL(quat_log_kernel, dim3(capped_grid((long)N, 256, kMaxGrid)), dim3(256), 0, stream(), d_quat, (long)N,
                       (long)ld_quat, d_rotvec, (long)ld_rotvec);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}

extern "C" int figh_rotvec_to_quat(const double *d_rotvec, int64_t N, int64_t ld_rotvec, const double *d_ref, int64_t ld_ref,
                                   double *d_out, int64_t ld_out) {
    FIGH_REQUIRE(d_rotvec && d_ref && d_out, "NULL pointer");
    FIGH_REQUIRE(N >= 1, "rotvec_to_quat: at least one sample");
    FIGH_REQUIRE(ld_rotvec >= 3 && ld_ref >= 4 && ld_out >= 4,
                 "rotvec_to_quat: a leading dimension below the width (3 in, 4 reference, 4 out)");
    const bool alias = d_out == d_ref && ld_out == ld_ref;
    FIGH_REQUIRE(alias || !overlap(d_ref, (N - 1) * ld_ref + 4, d_out, (N - 1) * ld_out + 4),
                 "rotvec_to_quat: the output overlaps the reference without being the reference itself");
    FIGH_REQUIRE(!overlap(d_rotvec, (N - 1) * ld_rotvec + 3, d_out, (N - 1) * ld_out + 4),
                 "rotvec_to_quat: the output overlaps the rotation vectors");
    if (int rc = ensure_device()) return rc;
    ProfileScope scope("rotvec_to_quat");
    hipLaunchKernelGGL(rotvec_to_quat_kernel, dim3(capped_grid((long)N, 256, kMaxGrid)), dim3(256), 0, stream(), d_rotvec,
                       (long)N, (long)ld_rotvec, d_ref, (long)ld_ref, d_out, (long)ld_out);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}

extern "C" int figh_wrench_transport(figh_model_t model, int joint, int64_t N, const double *d_q, int64_t ldq, const double *d_F,
                                     int layout_in, int inverse, double *d_out, int layout_out) {
    FIGH_REQUIRE(model && d_q && d_F && d_out, "NULL pointer");
    FIGH_REQUIRE(N >= 1, "wrench_transport: at least one sample");
    const DevModel &m = model->host;
    FIGH_REQUIRE(ldq >= m.nq, "wrench_transport: ldq below nq");
    FIGH_REQUIRE(joint >= 0 && joint < m.njoints, "wrench_transport: joint outside the model");
    FIGH_REQUIRE((layout_in == FIGH_WRENCH_SAMPLE || layout_in == FIGH_WRENCH_STACKED) &&
                     (layout_out == FIGH_WRENCH_SAMPLE || layout_out == FIGH_WRENCH_STACKED),
                 "wrench_transport: unknown layout");
    FIGH_REQUIRE(inverse == 0 || inverse == 1, "wrench_transport: inverse is 0 or 1");
    FIGH_REQUIRE(!overlap(d_F, 6 * N, d_out, 6 * N), "wrench_transport: output overlaps input");
    WrenchPath P;
    P.n = 0;
    short up[kMaxJoints];
    int depth = 0;
    for (int j = joint; j > 0; j = m.parents[j]) {
        if (depth >= kMaxPath) {
            set_error("wrench_transport: the support path is longer than the kernel arguments hold");
            return FIGH_ERR_UNSUPPORTED;
        }
        const int t = m.jtype[j], iq = m.idx_q[j], wq = t == 3 ? 7 : t == 2 ? 2 : 1;
        FIGH_REQUIRE(t >= 0 && t <= 3 && iq >= 0 && iq + wq <= m.nq && m.parents[j] >= 0 && m.parents[j] < j, "bad joint table");
        up[depth++] = (short)j;
    }
    for (int s = 0; s < kMaxPath; ++s) P.joint[s] = s < depth ? up[depth - 1 - s] : 0;
    P.n = depth;
    if (int rc = ensure_device()) return rc;
    ProfileScope scope("wrench_transport");
    const dim3 grid(capped_grid((long)((N + 63) / 64), 4, kMaxGrid)), block(256);
#define FIGH_WT_LAUNCH(A, B, C)                                                                                           \
    hipLaunchKernelGGL((wrench_transport_kernel<A, B, C>), grid, block, 0, stream(), model->dev, P, (long)N, d_q, (long)ldq, \
                       d_F, d_out)
    const int which = (layout_in == FIGH_WRENCH_SAMPLE ? 4 : 0) | (layout_out == FIGH_WRENCH_SAMPLE ? 2 : 0) | inverse;
    switch (which) {
        case 0: FIGH_WT_LAUNCH(false, false, false); break;
        case 1: FIGH_WT_LAUNCH(false, false, true); break;
        case 2: FIGH_WT_LAUNCH(false, true, false); break;
        case 3: FIGH_WT_LAUNCH(false, true, true); break;
        case 4: FIGH_WT_LAUNCH(true, false, false); break;
        case 5: FIGH_WT_LAUNCH(true, false, true); break;
        case 6: FIGH_WT_LAUNCH(true, true, false); break;
        default: FIGH_WT_LAUNCH(true, true, true); break;
    }
#undef FIGH_WT_LAUNCH
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}
