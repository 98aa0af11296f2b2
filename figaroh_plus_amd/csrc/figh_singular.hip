// Singular values of B small upper triangles on the device (figh_singular_values_batch): the last array-sized host step
// of the excitation objective, np.linalg.svd of the B r x r triangles of one finite-difference gradient.
//
// Algorithm: one-sided (Hestenes) Jacobi on the columns of R, fp64, no contraction (this unit is compiled with
// -ffp-contract=off, and _host.jacobi_singular_values_mirror states the same operations in the same order).  For a column
// pair (p, q), p < q:
//     alpha = a_p . a_p     beta = a_q . a_q     gamma = a_p . a_q          (recomputed from the columns, no running norms)
//     the pair is skipped when |gamma| <= 2^-52 sqrt(alpha beta)            (a zero column included)
//     zeta = (beta - alpha) / (2 gamma);  t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), sign(0) = +1
//     c = 1 / sqrt(1 + t^2);  s = c t;    a_p <- c a_p - s a_q;  a_q <- s a_p + c a_q
// A sweep visits every pair once, in the round-robin (circle) order: with n = r rounded up to even and m = n - 1, step
// s < m holds the pairs k < n / 2:  k = 0: (s, n - 1);  k >= 1: ((s + k) mod m, (s - k) mod m), ordered p < q; for odd r the
// pair that holds index r is the bye.  The pairs of a step are disjoint.  A sweep without a rotation ends the matrix as
// converged; sigma_k = sqrt(a_k . a_k).
//
// Kernel: one workgroup per matrix, looping over the matrices its grid does not cover.  The matrix sits in LDS column by
// column (rows padded to whole 16s with zeros, the strict lower triangle +0.0, never read from memory).  A pair belongs to
// one 16-lane group (a DPP row); lane l holds rows l, l + 16, ... of both columns in registers, adds its products in
// ascending row order, and the 16 partial sums meet in a fixed butterfly (xor 1, xor 2, mirror of 8, mirror of 16: every
// lane ends with the same bits).  The rotation is written back in place; one barrier per step.
//
// LDS layout: column c starts at c * ld doubles, ld = the smallest number >= the padded rows with ld = 16 (mod 32).  A
// ds_read_b64 is served in two groups of 32 lanes over 64 banks of 4 bytes: 16 lanes reading consecutive rows of one
// column cover 32 consecutive banks, and the other 16-lane group of the same half wave reads a column that is an odd number
// of columns away (neighbouring pairs k, k + 1 of a step differ by one column in p and in q, except where the index wraps),
// i.e. an odd multiple of 2 * 16 = 32 banks: the other half of the banks.  An odd ld (r + 1) would shift the second group by
// two banks only and make every read a two-way conflict.
//
// Bounds: the sweep loop has trip count max_sweeps, the step loop m, the row loops NCH; no lane waits for another.  Every
// barrier sits in control flow that depends on blockIdx, the launch arguments and the "rotated" word alone.  That word is
// one of three LDS words used in turn: sweep w sets word w mod 3, every wave reads it after the last barrier of the sweep,
// and thread 0 clears word (w + 1) mod 3 at the start of sweep w -- it was last read at the end of sweep w - 2 and is next
// set in sweep w + 1, and at least one barrier lies between each of these and the clearing.
#include "figh_internal.h"

using namespace figh;

namespace {

constexpr int kMaxR = 128;           // 128 x 144 x 8 B = 144 KB of LDS: one workgroup per CU
constexpr int kMaxWgsPerCu = 8;      // resident workgroups per CU the grid counts on, at most

__host__ __device__ inline int padded_rows(const int r) { return (r + 15) & ~15; }
__host__ __device__ inline int leading_dim(const int r) {
    const int rows = padded_rows(r);
    return (rows & 16) ? rows : rows + 16;  // = 16 (mod 32)
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(const double x) {  // x of the lane that the DPP control names, within a row of 16
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// sum over the 16 lanes of a DPP row, the same bits in every lane: (x_l + x_{l^1}), then the quad, then the 8, then the 16
__device__ __forceinline__ double row_sum(double x) {
    x = x + dpp_f64<0xB1>(x);   // quad_perm [1, 0, 3, 2]
    x = x + dpp_f64<0x4E>(x);   // quad_perm [2, 3, 0, 1]
    x = x + dpp_f64<0x141>(x);  // row_half_mirror: lane i <-> 7 - i, the other quad of the 8
    x = x + dpp_f64<0x140>(x);  // row_mirror: lane i <-> 15 - i, the other 8
    return x;
}

template <int NCH>
__global__ __launch_bounds__(1024) void jacobi_sv_kernel(const double *__restrict__ R, const long B, const int r,
                                                         const long stride, const int max_sweeps, double *__restrict__ sigma,
                                                         const long ld_sigma, int *__restrict__ status) {
    extern __shared__ double lds[];
    const int rows = 16 * NCH, ld = leading_dim(r);
    double *A = lds;
    volatile int *rotated = (volatile int *)(lds + (size_t)r * ld);  // three words
    const int tid = threadIdx.x, l = tid & 15, grp = tid >> 4;
    const int n = r + (r & 1), m = n - 1, npairs = n >> 1;
    const double thr = 0x1p-52;
    for (long b = blockIdx.x; b < B; b += gridDim.x) {
        const double *Rb = R + b * stride;
        for (int e = tid; e < rows * r; e += blockDim.x) {  // consecutive lanes along a row of R
            const int row = e / r, c = e - row * r;
            A[c * ld + row] = (row <= c) ? Rb[(long)row * r + c] : 0.0;
        }
        if (tid < 3) rotated[tid] = 0;
        __syncthreads();
        int sweeps = max_sweeps, converged = 0;
        for (int w = 0; w < max_sweeps; ++w) {
            const int word = w % 3;
            if (tid == 0) rotated[(w + 1) % 3] = 0;
            for (int s = 0; s < m; ++s) {
                int p = s, q = n - 1;
                if (grp > 0 && grp < npairs) {
                    p = s + grp;
                    p = p >= m ? p - m : p;
                    q = s - grp;
                    q = q < 0 ? q + m : q;
                }
                if (p > q) {
                    const int x = p;
                    p = q;
                    q = x;
                }
                if (grp < npairs && q < r) {  // (q == r: the bye of an odd r)
                    double *cp = A + p * ld + l, *cq = A + q * ld + l;
                    double ap[NCH], aq[NCH];
#pragma unroll
                    for (int j = 0; j < NCH; ++j) {
                        ap[j] = cp[16 * j];
                        aq[j] = cq[16 * j];
                    }
                    double alpha = ap[0] * ap[0], beta = aq[0] * aq[0], gamma = ap[0] * aq[0];
#pragma unroll
                    for (int j = 1; j < NCH; ++j) {
                        alpha = alpha + ap[j] * ap[j];
                        beta = beta + aq[j] * aq[j];
                        gamma = gamma + ap[j] * aq[j];
                    }
                    alpha = row_sum(alpha);
                    beta = row_sum(beta);
                    gamma = row_sum(gamma);
                    if (!(fabs(gamma) <= thr * sqrt(alpha * beta))) {  // (a NaN rotates: the matrix never converges)
                        const double zeta = (beta - alpha) / (2.0 * gamma);
                        const double den = fabs(zeta) + sqrt(1.0 + zeta * zeta);
                        const double t = (zeta < 0.0 ? -1.0 : 1.0) / den;
                        const double c = 1.0 / sqrt(1.0 + t * t);
                        const double sn = c * t;
#pragma unroll
                        for (int j = 0; j < NCH; ++j) {
                            cp[16 * j] = c * ap[j] - sn * aq[j];
                            cq[16 * j] = sn * ap[j] + c * aq[j];
                        }
                        if (l == 0) rotated[word] = 1;
                    }
                }
                __syncthreads();
            }
            if (rotated[word] == 0) {  // the same word, read by every wave behind the sweep's last barrier
                sweeps = w + 1;
                converged = 1;
                break;
            }
        }
        for (int c = grp; c < r; c += (int)(blockDim.x >> 4)) {
            const double *cc = A + c * ld + l;
            double acc = cc[0] * cc[0];
#pragma unroll
            for (int j = 1; j < NCH; ++j) acc = acc + cc[16 * j] * cc[16 * j];
            acc = row_sum(acc);
            if (l == 0) sigma[b * ld_sigma + c] = sqrt(acc);
        }
        if (tid == 0) {
            status[2 * b] = sweeps;
            status[2 * b + 1] = converged;
        }
        __syncthreads();  // the next matrix overwrites the columns
    }
}

template <int NCH>
int launch_jacobi(const unsigned grid, const unsigned threads, const size_t lds, const double *R, long B, int r, long stride,
                  int max_sweeps, double *sigma, long ld_sigma, int *status) {
    static bool raised = false;  // more than 64 KB of LDS per workgroup from r = 81 on: raised once, to the largest r of NCH
    if (!raised && lds > (64u << 10)) {
        constexpr int rmax = 16 * NCH < kMaxR ? 16 * NCH : kMaxR;
        FIGH_HIP(hipFuncSetAttribute((const void *)jacobi_sv_kernel<NCH>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(sizeof(double) * rmax * leading_dim(rmax) + 16)));
        raised = true;
    }
    ProfileScope scope("singular_values_batch", true);
    FIGH_LAUNCH_TIMED(jacobi_sv_kernel<NCH>, dim3(grid), dim3(threads), lds, R, B, r, stride, max_sweeps, sigma, ld_sigma,
                      status);
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}

}  // namespace

extern "C" int figh_singular_values_batch(const double *d_R, int64_t B, int r, int64_t stride, int max_sweeps, double *d_sigma,
                                          int64_t ld_sigma, int32_t *d_status) {
    if (int rc = ensure_device()) return rc;
    FIGH_REQUIRE(d_R && d_sigma && d_status, "NULL pointer");
    FIGH_REQUIRE(r >= 1 && B >= 1, "singular values: r and B must be at least 1");
    if (r > kMaxR) {
        set_error("singular values: more than 128 columns are not served on the device (the r x r SVD stays on the host)");
        return FIGH_ERR_UNSUPPORTED;
    }
    FIGH_REQUIRE(stride >= (int64_t)r * r, "singular values: the stride between the matrices is below r * r");
    FIGH_REQUIRE(ld_sigma >= r, "singular values: ld_sigma is below r");
    FIGH_REQUIRE(max_sweeps >= 1 && max_sweeps <= 1000, "singular values: max_sweeps must lie in [1, 1000]");
    const int npairs = (r + 1) / 2;
    const unsigned threads = (unsigned)((16 * npairs + 63) & ~63);  // one 16-lane group per pair of a step, whole waves
    const size_t lds = sizeof(double) * (size_t)r * leading_dim(r) + 16;
    long per_cu = (long)((160u << 10) / lds);
    const long by_threads = 2048 / threads;
    per_cu = per_cu < by_threads ? per_cu : by_threads;
    per_cu = per_cu < 1 ? 1 : per_cu > kMaxWgsPerCu ? kMaxWgsPerCu : per_cu;
    const unsigned grid = capped_grid(B, 1, per_cu * cu_count());
    switch (padded_rows(r) / 16) {
#define FIGH_JACOBI_CASE(NCH)                                                                                        \
    case NCH:                                                                                                        \
        return launch_jacobi<NCH>(grid, threads, lds, d_R, (long)B, r, (long)stride, max_sweeps, d_sigma, (long)ld_sigma, \
                                  d_status)
        FIGH_JACOBI_CASE(1);
        FIGH_JACOBI_CASE(2);
        FIGH_JACOBI_CASE(3);
        FIGH_JACOBI_CASE(4);
        FIGH_JACOBI_CASE(5);
        FIGH_JACOBI_CASE(6);
        FIGH_JACOBI_CASE(7);
        FIGH_JACOBI_CASE(8);
#undef FIGH_JACOBI_CASE
    }
    return FIGH_ERR_INVALID;
}
