// Self-collision distances of the excitation problem on the device: CollisionWrapper.computeCollisions + getDistances
// (src/figaroh/tools/robotcollisions.py:62-72, :108-113) over the simplified collision model
// (examples/tiago/utils/simplified_colission_model.py:55-180), for the samples of a batch of trajectories
// (examples/tiago/optimal_trajectory.py:176-186).  Boxes, cylinders, spheres and capsules only; no hpp-fcl.
//
// Convention: a shape is a convex core and a radius (box, cylinder: their own core, r = 0; sphere: its centre; capsule: its
// axis segment) and d = dist(core_A, core_B) - (r_A + r_B); when the cores intersect d = -(r_A + r_B) exactly.
//
// One query per lane, one wave per workgroup, the pair on blockIdx.y: shape kinds, support-function branches and the two
// joint paths are uniform in a wave, only the iteration count diverges.  Each lane walks the parent chains of its two
// geometries to the root itself (X <- jointPlacement_j . M_j(q_j) . X from the geometry's placement), then runs GJK in the
// world frame in fp64 -- the algorithm of tools/robotcollisions.py (module docstring), statement for statement:
//   w = s_A(-v) - s_B(v);  with a simplex in hand: stop (OK) when |v| - v.w / |v| <= tol;
//   w joins the simplex (<= 4 points, each with its witness on A); closest point of the simplex to the origin by cases
//   (segment: clamped projection; triangle: vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, face; tetrahedron: the
//   closest of the three faces that hold the new point, and "encloses the origin" when the origin is strictly on the inner side
//   of all four faces, none of them within 2^-40 of flat, and the step's lower bound v.w is not positive);
//   zero-weight points leave; stop (CORES_INTERSECT) when enclosed or |v|^2 <= 2^-80 max |s_i|^2.
// The loop runs at most max_iter times (ITERATION_CAP).  Simplex and witness points are named registers and the cases are
// written out: no indexed local array, no scratch.  Plain stores, no atomics: two calls give the same bits.
#include "figh_internal.h"
#include "figh_spatial.h"

using namespace figh;

namespace {

constexpr int kMaxGeoms = FIGH_COLLISION_MAX_GEOMETRIES;
constexpr int kMaxPairs = FIGH_COLLISION_MAX_PAIRS;
constexpr long kMaxGrid = 1 << 16;
constexpr double kZeroRelSq = 0x1p-80;

// launch-uniform, by value (kernel-argument segment: every index into it is wave-uniform)
struct CollisionPlan {
    unsigned char first[kMaxPairs], second[kMaxPairs];
    int kind[kMaxGeoms], parent[kMaxGeoms];
    double placement[kMaxGeoms][12];
    double half[kMaxGeoms][3];  // box: half sides; cylinder: radius, half length; capsule: 0, half length; sphere: zeros
    double radius[kMaxGeoms];   // of the rounding: sphere and capsule
};

struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 operator-(const V3 a, const V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator-(const V3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ double dot(const V3 a, const V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(const V3 a, const V3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// ((la a + lb b) + lc c) + ld d
__device__ __forceinline__ V3 combine(const double la, const V3 a, const double lb, const V3 b, const double lc, const V3 c,
                                      const double ld, const V3 d) {
    return {((la * a.x + lb * b.x) + lc * c.x) + ld * d.x, ((la * a.y + lb * b.y) + lc * c.y) + ld * d.y,
            ((la * a.z + lb * b.z) + lc * c.z) + ld * d.z};
}

// M_j(q_j) of joint j for the configuration at qi
__device__ __forceinline__ void joint_motion(const DevModel *M, const int j, const double *qi, double *Rj, double *pj) {
    const int jt = M->jtype[j], iq = M->idx_q[j];
    const double ax[3] = {M->axis[j][0], M->axis[j][1], M->axis[j][2]};
    const double sin_q = jt == FIGH_JT_CONTINUOUS ? qi[iq + 1] : 0.0;
    // (preset as figh_kinematics.hip's joint_motion does, although joint_transform writes every output: without these stores
    // the rotation of a CONTINUOUS joint came back uninitialised on gfx950 -- measured on the free-flyer tree, every geometry
    // behind its continuous joint misplaced -- while revolute, prismatic and free-flyer joints were right either way)
#pragma unroll
    for (int d = 0; d < 9; ++d) Rj[d] = (d % 4 == 0) ? 1.0 : 0.0;
    pj[0] = pj[1] = pj[2] = 0.0;
    joint_transform<false>(jt, ax, qi[iq], sin_q, 0.0, 0.0, qi + iq, nullptr, nullptr, 1, Rj, pj, nullptr, nullptr);
}

// (R, p) <- (Rb, pb) . (R, p)
__device__ __forceinline__ void mul_left(const double *Rb, const double *pb, double *R, double *p) {
    double Rn[9], t[3];
    matmul3(Rb, R, Rn);
    rot(Rb, p, t);
#pragma unroll
    for (int d = 0; d < 9; ++d) R[d] = Rn[d];
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] = t[d] + pb[d];
}

// oM_parent . placement: from the geometry up its parent chain to the universe (joint 0), at most njoints steps
__device__ __forceinline__ void geometry_placement(const DevModel *M, const int parent, const double *placement,
                                                   const double *qi, double *R, double *p) {
#pragma unroll
    for (int d = 0; d < 9; ++d) R[d] = placement[d];
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] = placement[9 + d];
    int j = parent;
    for (int step = 0; step < kMaxJoints && j > 0; ++step) {
        double Rj[9], pj[3];
        joint_motion(M, j, qi, Rj, pj);
        mul_left(Rj, pj, R, p);
        mul_left(M->placement[j], M->placement[j] + 9, R, p);
        j = M->parents[j];
    }
}

// support point of a core in the local direction d (kind is wave-uniform)
__device__ __forceinline__ V3 support_local(const int kind, const double *h, const V3 d) {
    if (kind == FIGH_GEOM_BOX) return {d.x >= 0.0 ? h[0] : -h[0], d.y >= 0.0 ? h[1] : -h[1], d.z >= 0.0 ? h[2] : -h[2]};
    if (kind == FIGH_GEOM_SPHERE) return {0.0, 0.0, 0.0};
    const double z = d.z >= 0.0 ? h[1] : -h[1];
    if (kind == FIGH_GEOM_CAPSULE) return {0.0, 0.0, z};
    const double dxy = sqrt(d.x * d.x + d.y * d.y);
    const double s = dxy > 0.0 ? h[0] / dxy : 0.0;  // d_xy = 0: the cap centre
    return {s * d.x, s * d.y, z};
}
// R s(R^T d) + p
__device__ __forceinline__ V3 support_world(const int kind, const double *h, const double *R, const double *p, const V3 d) {
    const V3 dl = {R[0] * d.x + R[3] * d.y + R[6] * d.z, R[1] * d.x + R[4] * d.y + R[7] * d.z,
                   R[2] * d.x + R[5] * d.y + R[8] * d.z};
    const V3 s = support_local(kind, h, dl);
    return {(R[0] * s.x + R[1] * s.y + R[2] * s.z) + p[0], (R[3] * s.x + R[4] * s.y + R[5] * s.z) + p[1],
            (R[6] * s.x + R[7] * s.y + R[8] * s.z) + p[2]};
}

__device__ __forceinline__ void closest_segment(const V3 a, const V3 b, double &la, double &lb) {
    const V3 ab = b - a;
    const double t = -dot(a, ab), den = dot(ab, ab);
    const double u = t <= 0.0 ? 0.0 : t >= den ? 1.0 : t / den;
    la = 1.0 - u;
    lb = u;
}

// the regions of Ericson's closest point of a triangle, in his order; the face weights as triple products (the products
// d1 d4 - d3 d2 ... cancel badly on the needle triangles of a converging query)
__device__ __forceinline__ void closest_triangle(const V3 a, const V3 b, const V3 c, double &la, double &lb, double &lc) {
    const V3 ab = b - a, ac = c - a;
    const double d1 = -dot(ab, a), d2 = -dot(ac, a);
    const double d3 = -dot(ab, b), d4 = -dot(ac, b);
    const double d5 = -dot(ab, c), d6 = -dot(ac, c);
    const V3 nrm = cross(ab, ac);
    const double vc = dot(nrm, cross(a, ab));
    const double vb = dot(nrm, cross(ac, a));
    const double va = dot(nrm, cross(b, c - b));
    if (d1 <= 0.0 && d2 <= 0.0) {
        la = 1.0; lb = 0.0; lc = 0.0;
    } else if (d3 >= 0.0 && d4 <= d3) {
        la = 0.0; lb = 1.0; lc = 0.0;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double t = d1 / (d1 - d3);
        la = 1.0 - t; lb = t; lc = 0.0;
    } else if (d6 >= 0.0 && d5 <= d6) {
        la = 0.0; lb = 0.0; lc = 1.0;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double t = d2 / (d2 - d6);
        la = 1.0 - t; lb = 0.0; lc = t;
    } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        la = 0.0; lb = 1.0 - t; lc = t;
    } else {
        const double den = 1.0 / (va + vb + vc);
        const double fv = vb * den, fw = vc * den;
        la = (1.0 - fv) - fw; lb = fv; lc = fw;
    }
}

// the origin strictly on e's side of the plane abc, e not within 2^-40 (relative) of that plane
__device__ __forceinline__ bool inner_side(const V3 a, const V3 b, const V3 c, const V3 e) {
    const V3 nrm = cross(b - a, c - a), ea = e - a;
    const double side_o = -dot(a, nrm), side_e = dot(ea, nrm);
    return side_o * side_e > 0.0 && side_e * side_e > kZeroRelSq * (dot(nrm, nrm) * dot(ea, ea));
}

__global__ __launch_bounds__(64) void collision_distances_kernel(const DevModel *__restrict__ M, const CollisionPlan P,
                                                                 const long B, const long n_per, const long n_eval,
                                                                 const int *__restrict__ idx, const double *__restrict__ q,
                                                                 const long ldq, const double tol, const int max_iter,
                                                                 const int n_pairs, double *__restrict__ out, const long ld_b,
                                                                 double *__restrict__ witness, int *__restrict__ status_out) {
    const int pair = blockIdx.y;
    const int ga = P.first[pair], gb = P.second[pair];
    const int kind_a = P.kind[ga], kind_b = P.kind[gb];
    const double ha[3] = {P.half[ga][0], P.half[ga][1], P.half[ga][2]};
    const double hb[3] = {P.half[gb][0], P.half[gb][1], P.half[gb][2]};
    const double rr = P.radius[ga] + P.radius[gb];
    const long total = B * n_eval;
    for (long e = (long)blockIdx.x * 64 + threadIdx.x; e < total; e += (long)gridDim.x * 64) {
        const long b = e / n_eval, i = e - b * n_eval;
        const long sample = idx ? idx[i] : i;
        const double *qi = q + (b * n_per + sample) * ldq;
        double Ra[9], pa[3], Rb[9], pb[3];
        geometry_placement(M, P.parent[ga], P.placement[ga], qi, Ra, pa);
        geometry_placement(M, P.parent[gb], P.placement[gb], qi, Rb, pb);

        V3 v = {pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2]};
        if (v.x == 0.0 && v.y == 0.0 && v.z == 0.0) v = {1.0, 0.0, 0.0};
        const V3 zero = {0.0, 0.0, 0.0};
        V3 s0 = zero, s1 = zero, s2 = zero, s3 = zero, a0 = zero, a1 = zero, a2 = zero, a3 = zero;
        double l0 = 0.0, l1 = 0.0, l2 = 0.0, l3 = 0.0;
        int n = 0, status = FIGH_COLLISION_ITERATION_CAP, iters = 0;
        for (int it = 1; it <= max_iter; ++it) {
            iters = it;
            const V3 a = support_world(kind_a, ha, Ra, pa, -v);
            const V3 w = a - support_world(kind_b, hb, Rb, pb, v);
            const double sep = dot(v, w);
            if (n > 0) {
                const double vn = sqrt(dot(v, v));
                if (vn - sep / vn <= tol) {
                    status = FIGH_COLLISION_OK;
                    break;
                }
            }
            bool enclosed = false;
            if (n == 0) {
                s0 = w; a0 = a;
                l0 = 1.0; l1 = 0.0; l2 = 0.0; l3 = 0.0;
            } else if (n == 1) {
                s1 = w; a1 = a;
                closest_segment(s0, s1, l0, l1);
                l2 = 0.0; l3 = 0.0;
            } else if (n == 2) {
                s2 = w; a2 = a;
                closest_triangle(s0, s1, s2, l0, l1, l2);
                l3 = 0.0;
            } else {
                s3 = w; a3 = a;
                enclosed = inner_side(s0, s1, s2, s3) && inner_side(s0, s1, s3, s2) && inner_side(s0, s2, s3, s1) &&
                           inner_side(s1, s2, s3, s0) && sep <= 0.0;
                double best, x, y, z;
                {  // face 0 1 3
                    closest_triangle(s0, s1, s3, x, y, z);
                    const V3 pt = combine(x, s0, y, s1, z, s3, 0.0, zero);
                    best = dot(pt, pt);
                    l0 = x; l1 = y; l2 = 0.0; l3 = z;
                }
                {  // face 0 2 3
                    closest_triangle(s0, s2, s3, x, y, z);
                    const V3 pt = combine(x, s0, y, s2, z, s3, 0.0, zero);
                    const double vv = dot(pt, pt);
                    if (vv < best) {
                        best = vv;
                        l0 = x; l1 = 0.0; l2 = y; l3 = z;
                    }
                }
                {  // face 1 2 3
                    closest_triangle(s1, s2, s3, x, y, z);
                    const V3 pt = combine(x, s1, y, s2, z, s3, 0.0, zero);
                    const double vv = dot(pt, pt);
                    if (vv < best) {
                        l0 = 0.0; l1 = x; l2 = y; l3 = z;
                    }
                }
            }
            ++n;
            double big = dot(s0, s0);
            if (n > 1) big = fmax(big, dot(s1, s1));
            if (n > 2) big = fmax(big, dot(s2, s2));
            if (n > 3) big = fmax(big, dot(s3, s3));
            // points of zero weight leave, the others keep their order (from the last slot down)
            int m = n;
            if (n > 3 && !(l3 > 0.0)) {
                l3 = 0.0;
                --m;
            }
            if (n > 2 && !(l2 > 0.0)) {
                s2 = s3; a2 = a3; l2 = l3; l3 = 0.0;
                --m;
            }
            if (n > 1 && !(l1 > 0.0)) {
                s1 = s2; a1 = a2; l1 = l2;
                s2 = s3; a2 = a3; l2 = l3; l3 = 0.0;
                --m;
            }
            if (!(l0 > 0.0)) {
                s0 = s1; a0 = a1; l0 = l1;
                s1 = s2; a1 = a2; l1 = l2;
                s2 = s3; a2 = a3; l2 = l3; l3 = 0.0;
                --m;
            }
            n = m;
            v = combine(l0, s0, l1, s1, l2, s2, l3, s3);
            if (enclosed || dot(v, v) <= kZeroRelSq * big) {
                status = FIGH_COLLISION_CORES_INTERSECT;
                break;
            }
        }
        const V3 pA = combine(l0, a0, l1, a1, l2, a2, l3, a3);
        const V3 pB = status == FIGH_COLLISION_CORES_INTERSECT ? pA : pA - v;
        const V3 diff = pA - pB;
        const double d_core = sqrt(dot(diff, diff));
        const long query = e * n_pairs + pair;
        out[b * ld_b + i * n_pairs + pair] = d_core - rr;
        if (witness) {
            double *wq = witness + 6 * query;
            wq[0] = pA.x; wq[1] = pA.y; wq[2] = pA.z;
            wq[3] = pB.x; wq[4] = pB.y; wq[5] = pB.z;
        }
        if (status_out) status_out[query] = status | (iters << 16);
    }
}

bool all_finite(const double *x, const int n) {
    for (int d = 0; d < n; ++d)
        if (!(x[d] - x[d] == 0.0)) return false;
    return true;
}

}  // namespace

extern "C" int figh_collision_distances(figh_model_t model, int64_t B, int64_t n_per, int n_idx, const int32_t *h_idx,
                                        const double *d_q, int64_t ldq, int n_geom, const int32_t *h_kind,
                                        const int32_t *h_parent, const double *h_placement, const double *h_dims, int n_pairs,
                                        const int32_t *h_pairs, double tol, int max_iter, double *d_out, int64_t ld_b,
                                        double *d_witness, int32_t *d_status) {
    if (int rc = ensure_device()) return rc;  // (first: without a device no model handle exists either)
    FIGH_REQUIRE(model && d_q && d_out && h_kind && h_parent && h_placement && h_dims && h_pairs, "NULL pointer");
    const DevModel &m = model->host;
    FIGH_REQUIRE(m.njoints >= 1 && m.njoints <= kMaxJoints && m.nq >= 1, "bad model");
    FIGH_REQUIRE(B >= 1 && n_per >= 1 && ldq >= m.nq, "bad shape, or the leading dimension of q is below nq");
    FIGH_REQUIRE(n_geom >= 1 && n_geom <= kMaxGeoms, "the geometry table holds 1 .. FIGH_COLLISION_MAX_GEOMETRIES objects");
    FIGH_REQUIRE(n_pairs >= 1 && n_pairs <= kMaxPairs, "the pair list holds 1 .. FIGH_COLLISION_MAX_PAIRS pairs");
    FIGH_REQUIRE(max_iter >= 1 && max_iter <= 1024, "max_iter outside [1, 1024]");
    FIGH_REQUIRE(tol > 0.0 && tol - tol == 0.0, "tol must be positive and finite");
    FIGH_REQUIRE(!h_idx || n_idx >= 1, "an index list needs at least one index");
    const long n_eval = h_idx ? n_idx : n_per;
    for (int w = 0; h_idx && w < n_idx; ++w)
        FIGH_REQUIRE(h_idx[w] >= 0 && h_idx[w] < n_per, "a sample index is outside [0, n_per)");
    FIGH_REQUIRE(ld_b >= n_eval * n_pairs, "the row stride of the output is below n_idx n_pairs");
    FIGH_REQUIRE(B * n_eval < (1L << 31) / kMaxPairs, "B n_idx n_pairs must stay below 2^31");
    CollisionPlan P = {};
    for (int g = 0; g < n_geom; ++g) {
        const double *dims = h_dims + 3 * g;
        FIGH_REQUIRE(h_kind[g] >= FIGH_GEOM_BOX && h_kind[g] <= FIGH_GEOM_CAPSULE, "unknown geometry kind");
        FIGH_REQUIRE(h_parent[g] >= 0 && h_parent[g] < m.njoints, "a geometry's parent joint is no joint of the model");
        FIGH_REQUIRE(all_finite(h_placement + 12 * g, 12), "a geometry placement is not finite");
        FIGH_REQUIRE(all_finite(dims, 3) && dims[0] >= 0.0 && dims[1] >= 0.0 && dims[2] >= 0.0,
                     "geometry dimensions must be finite and non-negative");
        P.kind[g] = h_kind[g];
        P.parent[g] = h_parent[g];
        for (int d = 0; d < 12; ++d) P.placement[g][d] = h_placement[12 * g + d];
        // the constructors' arguments (full lengths) -> what the support functions read
        if (h_kind[g] == FIGH_GEOM_BOX) {
            for (int d = 0; d < 3; ++d) P.half[g][d] = dims[d] * 0.5;
        } else if (h_kind[g] == FIGH_GEOM_CYLINDER) {
            P.half[g][0] = dims[0];
            P.half[g][1] = dims[1] * 0.5;
        } else if (h_kind[g] == FIGH_GEOM_CAPSULE) {
            P.half[g][1] = dims[1] * 0.5;
            P.radius[g] = dims[0];
        } else {
            P.radius[g] = dims[0];
        }
    }
    for (int p = 0; p < n_pairs; ++p) {
        const int f = h_pairs[2 * p], s = h_pairs[2 * p + 1];
        FIGH_REQUIRE(f >= 0 && f < n_geom && s >= 0 && s < n_geom && f != s, "a pair names an object that does not exist");
        P.first[p] = (unsigned char)f;
        P.second[p] = (unsigned char)s;
    }
    int *d_idx = nullptr;
    if (h_idx) {
        d_idx = (int *)workspace(4 * (size_t)n_idx, kWsCollisionIdx);
        if (!d_idx) return FIGH_ERR_ALLOC;
    }
    ProfileScope scope("collision_distances");
    if (h_idx) FIGH_HIP(hipMemcpyAsync(d_idx, h_idx, sizeof(int) * n_idx, hipMemcpyHostToDevice, stream()));
    hipLaunchKernelGGL(collision_distances_kernel, dim3(capped_grid(B * n_eval, 64, kMaxGrid), (unsigned)n_pairs), dim3(64), 0,
                       stream(), model->dev, P, (long)B, (long)n_per, n_eval, d_idx, d_q, (long)ldq, tol, max_iter, n_pairs,
                       d_out, (long)ld_b, d_witness, d_status);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}
