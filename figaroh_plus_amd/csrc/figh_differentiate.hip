// The device front end of the real-data chain: what the scripts do to the raw joint positions before
// build_regressor_basic sees them.
//   - scipy.signal.medfilt(x, kernel_size) over every column (examples/tiago/identification.py:63-90, apply_filters);
//   - pin.difference(model, q[i], q[i+1]) / ts, the first-order step of calculate_first_second_order_differentiation
//     (identification_tools.py:334-387; a Python loop over the samples for every model with a free-flyer or a continuous
//     joint);
//   - np.gradient(dq[:, j], edge_order=1) / h, its second-order step (identification_tools.py:378-384) and the TIAGo script's
//     estimate_acceleration (examples/tiago/identification.py:92-99).
// All three are parallel in time.  A median picks an element, the plain-joint difference and the gradient are two or three
// correctly rounded operations: this translation unit is compiled without FMA contraction, so those results are bit-equal to
// SciPy's / NumPy's.  Only the SO(2) / SE(3) logarithms go through the device math library (acos, atan2, sin, cos, sqrt).
#include "figh_internal.h"
#include "figh_spatial.h"

using namespace figh;

namespace {

constexpr long kMaxGrid = 1 << 16;  // workgroups per launch; every kernel loops over what is left

// ---------------------------------------------------------------------------------------------------------------- medfilt
__device__ __forceinline__ void order2(double &a, double &b) {
    const double lo = b < a ? b : a, hi = b < a ? a : b;
    a = lo;
    b = hi;
}

// K > 0: the window lives in registers and is sorted by an odd-even transposition network (K rounds of compare-exchange on
// fixed positions: no indexing, no scratch).  K == 0: any odd size up to 63 -- insertion sort of a scratch array (slow).
template <int K>
__global__ __launch_bounds__(256) void medfilt_cols_kernel(const double *__restrict__ X, const long L, const int cols,
                                                           const long ldx, const long total, const int ksize,
                                                           double *__restrict__ Y, const long ldy) {
    constexpr int W = K ? K : 63;
    const int k = K ? K : ksize, half = k / 2;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long row = e / cols;
        const int col = (int)(e - row * cols);
        const long blk = row / L, i = row - blk * L;
        const double *x = X + blk * L * ldx + col;  // x[n] = x[n * ldx], n in [0, L): one (row block, column) sequence
        double w[W];
        if constexpr (K != 0) {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const long n = i + j - half;
                w[j] = (n >= 0 && n < L) ? x[n * ldx] : 0.0;  // zero padding at both ends of the block
            }
#pragma unroll
            for (int round = 0; round < W; ++round) {
#pragma unroll
                for (int j = round & 1; j + 1 < W; j += 2) order2(w[j], w[j + 1]);
            }
            Y[row * ldy + col] = w[W / 2];
        } else {
            for (int j = 0; j < k; ++j) {
                const long n = i + j - half;
                const double v = (n >= 0 && n < L) ? x[n * ldx] : 0.0;
                int p = j;
                while (p > 0 && v < w[p - 1]) {
                    w[p] = w[p - 1];
                    --p;
                }
                w[p] = v;
            }
            Y[row * ldy + col] = w[half];
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- gradient
__global__ __launch_bounds__(256) void gradient_cols_kernel(const double *__restrict__ F, const long rows, const int cols,
                                                            const long ld, const int nactive, const double h,
                                                            const double *__restrict__ dh, double *__restrict__ G,
                                                            const long ldg) {
    const long total = rows * cols;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long i = e / cols;
        const int c = (int)(e - i * cols);
        double g = 0.0;  // the reference never writes the columns behind range(model.nq - 1)
        if (c < nactive) {
            const double *f = F + c;
            double num;  // numpy/lib/function_base.py gradient, uniform unit spacing, edge_order=1
            if (i == 0) num = f[ld] - f[0];
            else if (i == rows - 1) num = f[(rows - 1) * ld] - f[(rows - 2) * ld];
            else num = (f[(i + 1) * ld] - f[(i - 1) * ld]) / 2.0;
            g = num / (dh ? dh[i] : h);
        }
        G[i * ldg + c] = g;
    }
}

// ------------------------------------------------------------------------------------------------------- joint difference
constexpr int kMaxDiffV = 6 * (kMaxJoints - 1);

// what the kernel needs of the model, by value (wave-uniform: scalar registers / scalar loads)
struct DiffPlan {
    int nq, nv, nspecial;
    short vq[kMaxDiffV];         // velocity column -> position column of a revolute / prismatic joint, -1: not a plain joint
    short sp_type[kMaxJoints];   // 2: continuous (cos, sin), 3: free-flyer
    short sp_q[kMaxJoints], sp_v[kMaxJoints];
};

struct M3 {
    double m[3][3];
};

// identification_tools._log3, branch for branch
__device__ __forceinline__ void log3(const M3 &R, double (&out)[3]) {
    double tr = ((R.m[0][0] + R.m[1][1] + R.m[2][2]) - 1.0) / 2.0;
    tr = tr < -1.0 ? -1.0 : tr;
    tr = tr > 1.0 ? 1.0 : tr;
    const double theta = acos(tr);
    const double w[3] = {R.m[2][1] - R.m[1][2], R.m[0][2] - R.m[2][0], R.m[1][0] - R.m[0][1]};
    if (theta < 1e-8) {
        for (int i = 0; i < 3; ++i) out[i] = 0.5 * w[i];
        return;
    }
    if (3.141592653589793 - theta < 1e-6) {  // symmetric part: A = (R + I) / 2 = ax ax^T
        const double d0 = (R.m[0][0] + 1.0) / 2.0, d1 = (R.m[1][1] + 1.0) / 2.0, d2 = (R.m[2][2] + 1.0) / 2.0;
        int k = 0;  // np.argmax: the first of the largest
        double dk = d0;
        if (d1 > dk) k = 1, dk = d1;
        if (d2 > dk) k = 2, dk = d2;
        const double root = sqrt(dk);
        double ax[3];
        for (int i = 0; i < 3; ++i) ax[i] = ((k == 0 ? R.m[i][0] : k == 1 ? R.m[i][1] : R.m[i][2]) + (i == k ? 1.0 : 0.0)) / 2.0 / root;
        const double dot = w[0] * ax[0] + w[1] * ax[1] + w[2] * ax[2];
        for (int i = 0; i < 3; ++i) out[i] = theta * (dot >= 0 ? ax[i] : -ax[i]);
        return;
    }
    const double f = theta / (2.0 * sin(theta));
    for (int i = 0; i < 3; ++i) out[i] = f * w[i];
}

// free-flyer: log6(R0^T R1, R0^T (p1 - p0)), (linear, angular) -- identification_tools.joint_difference / _log6
__device__ __forceinline__ void freeflyer_difference(const double *q0, const double *q1, double (&v)[3], double (&w)[3]) {
    M3 R0, R1;  // identification_tools._quat_to_rot
    quat_to_rotation(q0[3], q0[4], q0[5], q0[6], &R0.m[0][0]);
    quat_to_rotation(q1[3], q1[4], q1[5], q1[6], &R1.m[0][0]);
    const double dp[3] = {q1[0] - q0[0], q1[1] - q0[1], q1[2] - q0[2]};
    M3 R;
    double p[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R.m[i][j] = R0.m[0][i] * R1.m[0][j] + R0.m[1][i] * R1.m[1][j] + R0.m[2][i] * R1.m[2][j];
        p[i] = R0.m[0][i] * dp[0] + R0.m[1][i] * dp[1] + R0.m[2][i] * dp[2];
    }
    log3(R, w);
    const double t = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double alpha, beta;
    if (t < 1e-4) {
        const double t2 = t * t;
        alpha = 1.0 - t2 / 12.0 - t2 * t2 / 720.0;
        beta = 1.0 / 12.0 + t2 / 720.0;
    } else {
        const double st = sin(t), ct = cos(t);
        alpha = t * st / (2.0 * (1.0 - ct));
        beta = 1.0 / (t * t) - st / (2.0 * t * (1.0 - ct));
    }
    const double cr[3] = {w[1] * p[2] - w[2] * p[1], w[2] * p[0] - w[0] * p[2], w[0] * p[1] - w[1] * p[0]};
    const double bwp = beta * (w[0] * p[0] + w[1] * p[1] + w[2] * p[2]);
    for (int i = 0; i < 3; ++i) v[i] = alpha * p[i] - 0.5 * cr[i] + bwp * w[i];
}

// A workgroup takes tiles of `tile` consecutive sample pairs: rows [p0, p0 + cnt] of q (cnt + 1 of them, a contiguous run
// of the row-major array; p0 + cnt <= N - 1, so row N is never touched) are staged in LDS with an odd row stride, pass A
// does the plain joints element by element, pass B gives the pairs of the tile one lane each for the model's continuous and
// free-flyer joints, and the cnt rows of dq leave as one contiguous run.
__global__ __launch_bounds__(256) void joint_difference_kernel(const DiffPlan P, const long npairs, const int tile,
                                                               const double *__restrict__ q, const double ts,
                                                               const double *__restrict__ dt, double *__restrict__ dq) {
    extern __shared__ double lds[];
    const int nq = P.nq, nv = P.nv, sq = nq | 1, sv = nv | 1;
    double *sQ = lds, *sD = lds + (long)(tile + 1) * sq;
    const long ntiles = (npairs + tile - 1) / tile;
    for (long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const long p0 = tl * tile;
        const int cnt = (int)(npairs - p0 < tile ? npairs - p0 : tile);
        const double *src = q + p0 * nq;
        for (int e = threadIdx.x; e < (cnt + 1) * nq; e += 256) {
            const int r = e / nq;
            sQ[r * sq + (e - r * nq)] = src[e];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * nv; e += 256) {  // pass A: q1 - q0
            const int r = e / nv, v = e - r * nv, c = P.vq[v];
            if (c >= 0) sD[r * sv + v] = (sQ[(r + 1) * sq + c] - sQ[r * sq + c]) / (dt ? dt[p0 + r] : ts);
        }
        if (P.nspecial > 0 && (int)threadIdx.x < cnt) {  // pass B: one lane per sample pair
            const int r = threadIdx.x;
            const double div = dt ? dt[p0 + r] : ts;
            const double *q0 = sQ + r * sq, *q1 = q0 + sq;
            double *d = sD + r * sv;
            for (int s = 0; s < P.nspecial; ++s) {
                const int iq = P.sp_q[s], iv = P.sp_v[s];
                if (P.sp_type[s] == 2) {  // (cos, sin): the angle of R0^T R1
                    const double c0 = q0[iq], s0 = q0[iq + 1], c1 = q1[iq], s1 = q1[iq + 1];
                    d[iv] = atan2(s1 * c0 - c1 * s0, c1 * c0 + s1 * s0) / div;
                } else {
                    double v[3], w[3];
                    freeflyer_difference(q0 + iq, q1 + iq, v, w);
                    for (int i = 0; i < 3; ++i) {
                        d[iv + i] = v[i] / div;
                        d[iv + 3 + i] = w[i] / div;
                    }
                }
            }
        }
        __syncthreads();
        double *dst = dq + p0 * nv;
        for (int e = threadIdx.x; e < cnt * nv; e += 256) {
            const int r = e / nv;
            dst[e] = sD[r * sv + (e - r * nv)];
        }
        __syncthreads();  // the next tile overwrites both stages
    }
}

// pairs per tile: both stages of a tile of 64 k pairs fit 64 KB of LDS, k <= 4 (one lane per pair of a 256-thread workgroup);
// 0: the model is too wide.  (_lib.joint_difference_tile states the same rule for the tests and the bench tool.)
int difference_tile(const DevModel &m) {
    const long per_row = 8L * ((m.nq | 1) + (m.nv | 1));
    const long k = (65536 - 8L * (m.nq | 1)) / (64 * per_row);
    return (int)(64 * (k > 4 ? 4 : k));
}

}  // namespace

extern "C" int figh_medfilt_cols(const double *d_X, int64_t rows, int cols, int64_t ldx, int nblocks, int kernel_size,
                                 double *d_Y, int64_t ldy) {
    FIGH_REQUIRE(d_X && d_Y, "NULL pointer");
    FIGH_REQUIRE(rows > 0 && cols > 0 && ldx >= cols && ldy >= cols && nblocks > 0 && rows % nblocks == 0, "bad shape");
    FIGH_REQUIRE(kernel_size % 2 == 1, "Each element of kernel_size should be odd.");
    FIGH_REQUIRE(kernel_size >= 1 && kernel_size <= 63, "kernel_size must be an odd number in [1, 63]");
    if (int rc = ensure_device()) return rc;
    ProfileScope scope("medfilt_cols");
    const long L = rows / nblocks, total = (long)rows * cols;
    const dim3 grid(capped_grid(total, 256, kMaxGrid)), block(256);
#define FIGH_MF_LAUNCH(K)                                                                                              \
    hipLaunchKernelGGL((medfilt_cols_kernel<K>), grid, block, 0, stream(), d_X, L, cols, (long)ldx, total, kernel_size, \
                       d_Y, (long)ldy)
    switch (kernel_size) {
        case 1: FIGH_MF_LAUNCH(1); break;
        case 3: FIGH_MF_LAUNCH(3); break;
        case 5: FIGH_MF_LAUNCH(5); break;
        case 7: FIGH_MF_LAUNCH(7); break;
        case 9: FIGH_MF_LAUNCH(9); break;
        default: FIGH_MF_LAUNCH(0); break;
    }
#undef FIGH_MF_LAUNCH
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}

extern "C" int figh_gradient_cols(const double *d_F, int64_t rows, int cols, int64_t ld, int ncols_active, double h,
                                  const double *d_h, double *d_G, int64_t ldg) {
    FIGH_REQUIRE(d_F && d_G, "NULL pointer");
    FIGH_REQUIRE(rows >= 2, "Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements "
                            "are required.");
    FIGH_REQUIRE(cols > 0 && ld >= cols && ldg >= cols && ncols_active >= 0 && ncols_active <= cols, "bad shape");
    if (int rc = ensure_device()) return rc;
    ProfileScope scope("gradient_cols");
    hipLaunchKernelGGL(gradient_cols_kernel, dim3(capped_grid((long)rows * cols, 256, kMaxGrid)), dim3(256), 0, stream(),
                       d_F, (long)rows, cols, (long)ld, ncols_active, h, d_h, d_G, (long)ldg);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}

extern "C" int figh_joint_difference(figh_model_t model, int64_t N, const double *d_q, double ts, const double *d_dt,
                                     double *d_dq) {
    FIGH_REQUIRE(model && d_q && d_dq, "NULL pointer");
    FIGH_REQUIRE(N >= 2, "at least two samples");
    const DevModel &m = model->host;
    FIGH_REQUIRE(m.nv >= 1 && m.nv <= kMaxDiffV && m.nq >= m.nv, "bad model");
    DiffPlan P;
    P.nq = m.nq;
    P.nv = m.nv;
    P.nspecial = 0;
    for (int v = 0; v < kMaxDiffV; ++v) P.vq[v] = -1;
    for (int j = 1; j < m.njoints; ++j) {
        const int t = m.jtype[j], iq = m.idx_q[j], iv = m.idx_v[j];
        const int wq = t == 3 ? 7 : t == 2 ? 2 : 1, wv = t == 3 ? 6 : 1;
        FIGH_REQUIRE(t >= 0 && t <= 3 && iq >= 0 && iv >= 0 && iq + wq <= m.nq && iv + wv <= m.nv, "bad joint table");
        if (t <= 1) {
            P.vq[iv] = (short)iq;
        } else {
            P.sp_type[P.nspecial] = (short)t;
            P.sp_q[P.nspecial] = (short)iq;
            P.sp_v[P.nspecial] = (short)iv;
            ++P.nspecial;
        }
    }
    const int tile = difference_tile(m);
    FIGH_REQUIRE(tile >= 64, "model too wide for the LDS tile of the difference kernel");
    if (int rc = ensure_device()) return rc;
    ProfileScope scope("joint_difference");
    const long npairs = N - 1;
    const size_t lds_bytes = 8 * ((size_t)(tile + 1) * (m.nq | 1) + (size_t)tile * (m.nv | 1));
    const long cap = 8L * cu_count();
    const long ntiles = (npairs + tile - 1) / tile;
    hipLaunchKernelGGL(joint_difference_kernel, dim3((unsigned)(ntiles < cap ? ntiles : cap)), dim3(256), lds_bytes, stream(),
                       P, npairs, tile, d_q, ts, d_dt, d_dq);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}
