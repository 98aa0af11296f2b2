// D-optimal posture selection (examples/tiago/optimal_config.py, examples/ur10/optimal_config.py) as two data-parallel
// passes over the resident base kinematic regressor d_R: row k N + i is measured component k < c of candidate posture i < N,
// n columns, leading dimension ldr -- the layout calculate_base_kinematics_regressor leaves (rearrange_rb, :31-39, is not
// needed).  No X_i = R_i^T R_i (sub_info_matrix, :42-60) is ever stored.
//
//   figh_design_gram     M(w) = sum_i w_i sum_k r_{k,i} r_{k,i}^T          (the Mw of SOCP.add_constraints, :137-140)
//   figh_design_scores   G_i = R_i M^-1 R_i^T through the Cholesky factor L of M:  tr G_i, det(I + G_i), det(I - G_i)
//                        (get_critD of Detmax.main_algo's add and remove scans, :98-119, as ratios to det M)
//
// The Gram pass.  v_mfma_f64_16x16x4_f64, not VALU FMAs: a VALU formulation has to stage the rows in LDS and reads
// 2 T doubles from it per T x T products, which bounds it near a quarter of the HBM rate at n = 34; the MFMA takes
// both operands as they come from memory (A[i][k] = w r[row k][16 ta + i], B[k][j] = r[row k][16 tb + j], four rows per
// instruction), so the only traffic is the one read of R.  Each wave owns a run of candidates and the tile pairs ta >= tb in
// registers; the four waves of a workgroup are summed through LDS in wave order, the workgroups' partials go through the
// library's workspace and are summed in workgroup order by a second launch, which writes entry (a, b), a >= b, to both
// triangles.  No atomics, nothing depends on ldr: two calls give the same bits.  w_i multiplies the A operand (one
// rounding), so w_i = 0 contributes exact zeros.  The builtins are explicit: -ffp-contract=off does not touch them.
//
// The scores pass is compiled WITHOUT FMA contraction and states ONE operation order, which the NumPy mirror
// (calibration/optimal_design.py, scores_mirror) follows operation by operation; every operation is one correctly rounded
// + - * /, so device and mirror are bit-equal:
//
//   row r = r_{k,i}:   for a = 0 .. n-1:   s = r_a;   for b = 0 .. a-1:  s = s - (L_ab * y_b);   y_a = s / L_aa
//   G[k][l] (l >= k):  g = 0.0;   for a = 0 .. n-1:  g = g + (y_{k,a} * y_{l,a})
//   trace:             t = 0.0;   for k = 0 .. c-1:  t = t + G[k][k]
//   det(I + G):  A[k][k] = 1.0 + G[k][k], A[k][l] = G[k][l];   det(I - G):  A[k][k] = 1.0 - G[k][k], A[k][l] = -G[k][l]  (l > k)
//     det = 1.0;  for p = 0 .. c-1:   piv = A[p][p];   det = det * piv
//                                    for r = p+1 .. c-1:  f = A[p][r] / piv;   for q = r .. c-1:  A[r][q] = A[r][q] - (f * A[p][q])
//     det(I - G) is +0.0 as soon as a pivot is not > 0 (M - X_i is then not positive definite).
//
// y lives in registers: the kernel is instantiated for n padded up to NP = 8, 16, ..., 96 and L is padded with identity
// rows, so a padded term is s - 0 * y = s and g + 0 * 0 = g exactly.  L sits packed in LDS (row a at a (a + 1) / 2), every
// lane of a wave reads the same address (broadcast).  Thread (k, lane) of a workgroup of c waves owns row k of candidate
// 64 tile + lane; up to NP = 80 a wave brings its 64 rows in eight columns at a time with eight lanes along a row (64-byte
// runs), one chunk ahead of its use, and turns them through a staging tile of its own in LDS; the y of a candidate's rows
// meet through LDS eight columns at a time, G through LDS once, and wave 0 eliminates.
#include "figh_internal.h"

#include <vector>

using namespace figh;

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxN = FIGH_DESIGN_MAX_COLS;  // 96: packed L is 37 KB of LDS
constexpr int kMaxC = 6;
constexpr int kChunk = 8;  // columns of y exchanged per step
constexpr int kMaxStagedNP = 80;  // the widest instantiation that brings its rows in through the staging tile
constexpr int kStageLd = 9;  // leading dimension of a wave's 64 x 8 staging tile (odd: the transposed reads spread over the banks)

// ------------------------------------------------------------------------------------------------------------ Gram
// D register r of lane 16 g + j holds entry (g + 4 r, j) of the 16 x 16 tile (figh_wave.h)
__device__ __forceinline__ int tile_slot(const int i, const int j) { return (i >> 2) * 64 + 16 * (i & 3) + j; }

template <int NT>
__global__ __launch_bounds__(256) void design_gram_kernel(const double *__restrict__ R, const long ldr, const long N, const int c,
                                                          const int n, const double *__restrict__ w, const long per,
                                                          double *__restrict__ part) {
    constexpr int NPAIR = NT * (NT + 1) / 2;
    __shared__ double sum[NPAIR * 256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, cc = lane & 15;
    f64x4 acc[NPAIR];
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) acc[p] = f64x4{0.0, 0.0, 0.0, 0.0};
    const long i0 = ((long)blockIdx.x * 4 + wv) * per;
    const long i1 = i0 + per < N ? i0 + per : N;
    // UNR steps of four rows per trip, every load of a trip ahead of its first product: the bytes in flight per wave are
    // what keeps the pass at the memory rate
    constexpr int UNR = NT <= 3 ? 4 : 2;
    for (int k = 0; k < c; ++k) {
        const double *Rk = R + (long)k * N * ldr;
        for (long ib = i0; ib < i1; ib += 4 * UNR) {
            double x[UNR][NT], a[UNR][NT];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const long i = ib + 4 * u + g;
                const bool on = i < i1;
                const double wi = on ? (w ? w[i] : 1.0) : 0.0;
                const double *row = Rk + (on ? i : i0) * ldr;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int col = 16 * t + cc;
                    x[u][t] = (on && col < n) ? row[col] : 0.0;
                    a[u][t] = wi * x[u][t];
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                int p = 0;
#pragma unroll
                for (int ta = 0; ta < NT; ++ta)
#pragma unroll
                    for (int tb = 0; tb <= ta; ++tb, ++p)
                        acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][ta], x[u][tb], acc[p], 0, 0, 0);
            }
        }
    }
    // the four waves in wave order; the last one writes the workgroup's partial
    double *out = part + (long)blockIdx.x * NPAIR * 256;
    for (int turn = 0; turn < 4; ++turn) {
        if (wv == turn) {
#pragma unroll
            for (int p = 0; p < NPAIR; ++p)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = p * 256 + r * 64 + lane;
                    const double v = turn == 0 ? acc[p][r] : sum[e] + acc[p][r];
                    if (turn == 3) out[e] = v;
                    else sum[e] = v;
                }
        }
        __syncthreads();
    }
}

// entry (a, b), a >= b, of M = the partials of that entry in workgroup order; written to both triangles
__global__ __launch_bounds__(256) void design_gram_reduce_kernel(const double *__restrict__ part, const int nblocks, const int npair,
                                                                 const int n, double *__restrict__ M) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n * (n + 1) / 2) return;
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= e) ++a;
    const int b = e - a * (a + 1) / 2;
    const int ta = a >> 4, tb = b >> 4;
    const double *src = part + (ta * (ta + 1) / 2 + tb) * 256 + tile_slot(a & 15, b & 15);
    double s = 0.0;
    for (int blk = 0; blk < nblocks; ++blk) s += src[(long)blk * npair * 256];
    M[a * n + b] = s;
    M[b * n + a] = s;
}

// ---------------------------------------------------------------------------------------------------------- scores
// the product of the pivots of the symmetric elimination of I + G (MINUS = false) or I - G (true), upper triangle only
template <bool MINUS>
__device__ __forceinline__ double pivots_product(const double (&G)[kMaxC][kMaxC], const int c) {
    double A[kMaxC][kMaxC];
#pragma unroll
    for (int p = 0; p < kMaxC; ++p)
#pragma unroll
        for (int q = p; q < kMaxC; ++q)
            A[p][q] = p == q ? (MINUS ? 1.0 - G[p][p] : 1.0 + G[p][p]) : (MINUS ? -G[p][q] : G[p][q]);
    double det = 1.0;
    bool ok = true;
#pragma unroll
    for (int p = 0; p < kMaxC; ++p) {
        if (p < c) {
            const double piv = A[p][p];
            if (MINUS && !(piv > 0.0)) ok = false;
            det = det * piv;
#pragma unroll
            for (int r = p + 1; r < kMaxC; ++r) {
                if (r < c) {
                    const double f = A[p][r] / piv;
#pragma unroll
                    for (int q = r; q < kMaxC; ++q)
                        if (q < c) A[r][q] = A[r][q] - f * A[p][q];
                }
            }
        }
    }
    return MINUS && !ok ? 0.0 : det;
}

template <int NP>
__global__ __launch_bounds__(64 * kMaxC) void design_scores_kernel(const double *__restrict__ R, const long ldr, const long N,
                                                                   const int c, const int n, const double *__restrict__ Lpacked,
                                                                   double *__restrict__ d_trace, double *__restrict__ d_add,
                                                                   double *__restrict__ d_rm, const long ntiles) {
    constexpr int NL = NP * (NP + 1) / 2;
    extern __shared__ double lds[];
    double *Ls = lds;       // packed, padded L
    double *ex = lds + NL;  // kMaxC x kChunk x 64: the exchange of y, then of G
    double *st = ex + kMaxC * kChunk * 64 + (threadIdx.x >> 6) * (64 * kStageLd);  // this wave's 64 x 8 staging tile
    const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < NL; e += blockDim.x) Ls[e] = Lpacked[e];
    __syncthreads();
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long i = tile * 64 + lane;
        const bool on = i < N;
        // (an offset the optimiser cannot see through: the reads of L are invariant in this loop and would all be hoisted
        // out of it, into more registers than there are)
        int l0 = 0;
        asm volatile("" : "+v"(l0));
        const double *Lt = Ls + l0;
        // the rows come in eight columns at a time, eight lanes along a row (64-byte runs, not 8-byte pieces a row apart),
        // one chunk ahead of the substitution that consumes them, and turn through the wave's own staging tile
        const int sub = lane >> 3, colj = lane & 7;
        const long tile_row0 = (long)k * N + tile * 64;
        double nx[kChunk], y[NP], gk[kMaxC];
        auto fetch = [&](const int ch) {
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                const long cand = tile * 64 + 8 * j + sub;
                const int col = kChunk * ch + colj;
                const bool ok = cand < N && col < n;
                const double v = R[(tile_row0 + (cand < N ? 8 * j + sub : 0)) * ldr + (col < n ? col : 0)];
                nx[j] = ok ? v : 0.0;
            }
        };
        // (NP = 88, 96: the chunk in flight and its addresses would spill; there every lane reads its own row up front)
        constexpr bool kStaged = NP <= kMaxStagedNP;
        if (kStaged) {
            fetch(0);
        } else {
            const double *row = R + ((long)k * N + (on ? i : 0)) * ldr;
#pragma unroll
            for (int a = 0; a < NP; ++a) {  // (an address inside the row for every a: one select per entry, no branch)
                const double v = row[a < n ? a : 0];
                y[a] = (on && a < n) ? v : 0.0;
            }
        }
#pragma unroll
        for (int l = 0; l < kMaxC; ++l) gk[l] = 0.0;
#pragma unroll
        for (int ch = 0; ch < NP / kChunk; ++ch) {
            if (kStaged) {
#pragma unroll
                for (int j = 0; j < kChunk; ++j) st[(8 * j + sub) * kStageLd + colj] = nx[j];
                if (ch + 1 < NP / kChunk) fetch(ch + 1);
                // (the wave reads what the wave wrote: LDS serves a wave's accesses in order, no barrier)
#pragma unroll
                for (int j = 0; j < kChunk; ++j) y[kChunk * ch + j] = st[lane * kStageLd + j];
            }
#pragma unroll
            for (int a = kChunk * ch; a < kChunk * (ch + 1); ++a) {
                double s = y[a];
#pragma unroll
                for (int b = 0; b < a; ++b) s = s - Lt[a * (a + 1) / 2 + b] * y[b];
                y[a] = s / Lt[a * (a + 1) / 2 + a];
                ex[(k * kChunk + a - kChunk * ch) * 64 + lane] = y[a];
            }
            __syncthreads();
#pragma unroll
            for (int l = 0; l < kMaxC; ++l) {
                if (l >= k && l < c) {
#pragma unroll
                    for (int j = 0; j < kChunk; ++j) gk[l] = gk[l] + y[kChunk * ch + j] * ex[(l * kChunk + j) * 64 + lane];
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int l = 0; l < kMaxC; ++l)
            if (l >= k && l < c) ex[(k * kMaxC + l) * 64 + lane] = gk[l];
        __syncthreads();
        if (k == 0 && on) {
            double G[kMaxC][kMaxC];
#pragma unroll
            for (int p = 0; p < kMaxC; ++p)
#pragma unroll
                for (int q = p; q < kMaxC; ++q) G[p][q] = q < c ? ex[(p * kMaxC + q) * 64 + lane] : 0.0;
            if (d_trace) {
                double t = 0.0;
#pragma unroll
                for (int p = 0; p < kMaxC; ++p)
                    if (p < c) t = t + G[p][p];
                d_trace[i] = t;
            }
            if (d_add) d_add[i] = pivots_product<false>(G, c);
            if (d_rm) d_rm[i] = pivots_product<true>(G, c);
        }
        __syncthreads();
    }
}

int check_shape(const double *d_R, const int64_t ldr, const int64_t N, const int c, const int n) {
    FIGH_REQUIRE(d_R, "NULL regressor");
    FIGH_REQUIRE(c >= 1 && c <= kMaxC, "calibration_index c must lie in 1 .. 6");
    FIGH_REQUIRE(n >= 1 && n <= kMaxN, "the number of columns n must lie in 1 .. FIGH_DESIGN_MAX_COLS");
    FIGH_REQUIRE(ldr >= n, "leading dimension below the width");
    FIGH_REQUIRE(N >= 1, "the pool needs at least one candidate");
    return FIGH_OK;
}

// workgroups of the Gram kernel that one compute unit holds at a time (asked once per instantiation; 1 when the query fails)
template <int NT>
int gram_resident_workgroups() {
    static int wgs = 0;
    if (!wgs && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, design_gram_kernel<NT>, 256, 0) != hipSuccess || wgs < 1)) {
        (void)hipGetLastError();
        wgs = 1;
    }
    return wgs;
}

template <int NT>
void launch_gram(const unsigned grid, const double *R, long ldr, long N, int c, int n, const double *w, long per, double *part) {
    hipLaunchKernelGGL(design_gram_kernel<NT>, dim3(grid), dim3(256), 0, stream(), R, ldr, N, c, n, w, per, part);
}

template <int NP>
void launch_scores(const unsigned grid, const int c, const double *R, long ldr, long N, int n, const double *L, double *t,
                   double *a, double *r, long ntiles) {
    const size_t lds = sizeof(double) * (NP * (NP + 1) / 2 + kMaxC * kChunk * 64 + (NP <= kMaxStagedNP ? kMaxC * 64 * kStageLd : 0));
    static bool raised = false;  // more than 64 KB of LDS per workgroup at NP = 64 .. 80
    if (!raised && lds > (64u << 10)) {
        (void)hipFuncSetAttribute((const void *)design_scores_kernel<NP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        raised = true;
    }
    hipLaunchKernelGGL(design_scores_kernel<NP>, dim3(grid), dim3(64 * c), lds, stream(), R, ldr, N, c, n, L, t, a, r, ntiles);
}

}  // namespace

extern "C" int figh_design_gram(const double *d_R, int64_t ldr, int64_t N, int c, int n, const double *d_w, double *h_M) {
    if (int rc = ensure_device()) return rc;
    if (int rc = check_shape(d_R, ldr, N, c, n)) return rc;
    FIGH_REQUIRE(h_M, "NULL output");
    const int nt = (n + 15) / 16, npair = nt * (nt + 1) / 2;
    // a wave owns `per` candidates (a multiple of four, at least 64); no more workgroups of four waves than are resident at a time
    static const int resident[6] = {gram_resident_workgroups<1>(), gram_resident_workgroups<2>(), gram_resident_workgroups<3>(),
                                    gram_resident_workgroups<4>(), gram_resident_workgroups<5>(), gram_resident_workgroups<6>()};
    long grid = (N + 255) / 256;
    const long cap = (long)resident[nt - 1] * cu_count();
    if (grid > cap) grid = cap;
    long per = (N + 4 * grid - 1) / (4 * grid);
    per = (per + 3) / 4 * 4;
    if (per < 64) per = 64;
    double *part = (double *)workspace(sizeof(double) * (size_t)grid * npair * 256, kWsDesignPartials);
    double *dM = (double *)workspace(sizeof(double) * (size_t)n * n, kWsDesignGram);
    if (!part || !dM) return FIGH_ERR_ALLOC;
    {
        ProfileScope scope("design_gram");
        const unsigned gr = (unsigned)grid;
        switch (nt) {
            case 1: launch_gram<1>(gr, d_R, ldr, N, c, n, d_w, per, part); break;
            case 2: launch_gram<2>(gr, d_R, ldr, N, c, n, d_w, per, part); break;
            case 3: launch_gram<3>(gr, d_R, ldr, N, c, n, d_w, per, part); break;
            case 4: launch_gram<4>(gr, d_R, ldr, N, c, n, d_w, per, part); break;
            case 5: launch_gram<5>(gr, d_R, ldr, N, c, n, d_w, per, part); break;
            default: launch_gram<6>(gr, d_R, ldr, N, c, n, d_w, per, part); break;
        }
        hipLaunchKernelGGL(design_gram_reduce_kernel, dim3((n * (n + 1) / 2 + 255) / 256), dim3(256), 0, stream(), part, (int)grid,
                           npair, n, dM);
        FIGH_HIP(hipGetLastError());
    }
    FIGH_HIP(hipMemcpyAsync(h_M, dM, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost, stream()));
    FIGH_HIP(hipStreamSynchronize(stream()));
    return FIGH_OK;
}

extern "C" int figh_design_scores(const double *d_R, int64_t ldr, int64_t N, int c, int n, const double *h_L, double *d_trace,
                                  double *d_det_add, double *d_det_rm) {
    if (int rc = ensure_device()) return rc;
    if (int rc = check_shape(d_R, ldr, N, c, n)) return rc;
    FIGH_REQUIRE(h_L, "NULL Cholesky factor");
    FIGH_REQUIRE(d_trace || d_det_add || d_det_rm, "all three outputs are NULL");
    for (int a = 0; a < n; ++a) {
        const double d = h_L[(size_t)a * n + a];
        FIGH_REQUIRE(d > 0.0 && d - d == 0.0, "a diagonal entry of L is not finite and positive");
    }
    const int np = (n + kChunk - 1) / kChunk * kChunk, nl = np * (np + 1) / 2;
    static std::vector<double> packed;  // row a of the lower triangle at a (a + 1) / 2; identity rows behind row n - 1
    packed.assign(nl, 0.0);
    for (int a = 0; a < np; ++a) {
        if (a < n)
            for (int b = 0; b <= a; ++b) packed[a * (a + 1) / 2 + b] = h_L[(size_t)a * n + b];
        else
            packed[a * (a + 1) / 2 + a] = 1.0;
    }
    double *dL = (double *)workspace(sizeof(double) * nl, kWsDesignFactor);
    if (!dL) return FIGH_ERR_ALLOC;
    const long ntiles = (N + 63) / 64, cap = 4L * cu_count();
    const unsigned grid = (unsigned)(ntiles < cap ? ntiles : cap);
    ProfileScope scope("design_scores");
    FIGH_HIP(hipMemcpyAsync(dL, packed.data(), sizeof(double) * nl, hipMemcpyHostToDevice, stream()));
    FIGH_HIP(hipStreamSynchronize(stream()));  // (packed is reused by the next call)
    switch (np / kChunk) {
        case 1: launch_scores<8>(grid, c, d_R, ldr, N, n, dL, d_trace, d_det_add, d_det_rm, ntiles); break;
        case 2: launch_scores<16>(grid, c, d_R, ldr, N, n, dL, d_trace, d_det_add, d_det_rm, ntiles); break;
        case 3: launch_scores<24>(grid, c, d_R, ldr, N, n, dL, d_trace, d_det_add, d_det_rm, ntiles); break;
        case 4: launch_scores<32>(grid, c, d_R, ldr, N, n, dL, d_trace, d_det_add, d_det_rm, ntiles); break;
        case 5: launch_scores<40>(grid, c, d_R, ldr, N, n, dL, d_trace, d_det_add, d_det_rm, ntiles); break;
        case 6: launch_scores<48>(grid, c, d_R, ldr, N, n, dL, d_trace, d_det_add, d_det_rm, ntiles); break;
        case 7: launch_scores<56>(grid, c, d_R, ldr, N, n, dL, d_trace, d_det_add, d_det_rm, ntiles); break;
        case 8: launch_scores<64>(grid, c, d_R, ldr, N, n, dL, d_trace, d_det_add, d_det_rm, ntiles); break;
        case 9: launch_scores<72>(grid, c, d_R, ldr, N, n, dL, d_trace, d_det_add, d_det_rm, ntiles); break;
        case 10: launch_scores<80>(grid, c, d_R, ldr, N, n, dL, d_trace, d_det_add, d_det_rm, ntiles); break;
        case 11: launch_scores<88>(grid, c, d_R, ldr, N, n, dL, d_trace, d_det_add, d_det_rm, ntiles); break;
        default: launch_scores<96>(grid, c, d_R, ldr, N, n, dL, d_trace, d_det_add, d_det_rm, ntiles); break;
    }
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}
