// K1 + K3 level 0 in ONE launch for serial chains (UR10: BASELINE configs[1]) -- W is written to HBM exactly as
// figh_regressor_build writes it, and every 64-row tile is factored while it is still in LDS: the TSQR no longer reads W
// back (the two-launch form moves 4.0 GB out and 3.4 GB back in for 10^6 UR10 samples).
//
// Replaces, in one pass over the samples, build_regressor_basic (src/figaroh/tools/regressor.py:20-194, the
// pin.computeJointTorqueRegressor loop :45-87), the column norms of get_index_eliminate (:258-279) and the np.linalg.qr
// of get_baseParams (src/figaroh/tools/qrdecomposition.py:205) on the kept columns [+ tau].
//
// One workgroup per CU, 2 + C waves with two roles (the roles never meet at a barrier inside the tile loop):
//
//   producers (waves 0, 1) regressor_chain_kernel's tile body, one sample per lane, every other sample tile of the workgroup
//                         each: forward recursion once per 64 samples, then for every joint row j the lane's 14 NJ row entries
//                         (+ the row's tau entry) go to the producer's OWN tile buffer in LDS [64][NC + 2]; the tile is
//                         announced (LDS counter), streamed to W as contiguous 1 KB runs of 16-byte stores, and its
//                         diag(W^T W) contribution is accumulated (LDS accumulators, fixed order).  256 registers (two waves
//                         per SIMD): the per-link rotations are re-formed from (cos, sin) where the two-launch kernel keeps
//                         them (431 registers there), q', q'' wait in LDS.
//   consumers (waves 2..)  tsqr2_kernel's wave: a private triangle, the 64 x 64 register tile in the MFMA C/D layout.  A free
//                         consumer claims the next announced tile of either buffer (LDS compare-and-swap: tiles go to
//                         whoever is free -- row blocks of joint 1 cost 10x those of joint 6), gathers the kept columns
//                         [+ tau] of the LDS tile into its registers, hands the buffer back and runs the column steps
//                         (figh_tsqr_narrow.h -- the code of the two-launch kernel, RLAST form: the last 16 columns of the
//                         triangle in registers, 7.4 instead of 13.8 KB of LDS per wave).
//
// Measured on the first form (one producer, seven consumers with 13.8 KB triangles; in-kernel s_memtime buckets, an
// instrumentation since removed): the producer needs
// 10 000 cycles per tile (row emission 3 900, stream-out 2 000, column norms 1 600, forward recursion 1 100 -- a single wave
// is latency-bound) where seven consumers finish a tile every 5 000, and everything that touches THE buffer is serial.
// Hence two producers with a buffer each: 2 x 44 KB tiles + 2 x 9 KB staging + C x 7.4 KB triangles = 152 KB (C = 6).
// All arithmetic is fp64.  The kept-column list is the caller's (the previous pass's, verified afterwards against the
// norms this launch produces -- the same speculation figh_tsqr_selected makes with the column count).
//
// ---- the batched, W-free form (figh_regressor_tsqr_batch_fused): the excitation objective np.linalg.cond(W_b) of
// examples/tiago/optimal_trajectory.py:100-133 at the B perturbed trajectories of one finite-difference gradient (:296-313)
// needs B small triangles and nothing else.  The same kernel, template flag TRAJ: grid (S, B), workgroup (s, b) owns the
// sample tiles s, s + S, ... of trajectory b (a tile never straddles two trajectories; the last one of a trajectory is the
// ragged tile body), the producers neither stream W out nor accumulate norms.  Every workgroup leaves its consumers'
// triangles; fused_batch_merge_kernel then factors the S x ncons triangles of every trajectory in one launch per level
// (grid (workgroups per trajectory, B): tsqr_coop_kernel's sweep, 512 stacked rows per workgroup), so the launch count is
// 1 + levels whatever B is -- one level up to 512 stacked rows (UR10: S <= 2), two up to 512 * 512 / nc, never more than
// three.  The triangle of the previous trajectories (d_R_stack) is APPENDED to every trajectory's stack: the first merge
// level reads it in place as the nc rows behind the trajectory's own -- no copy, no launch, and the level-0 kernel keeps
// one code path (seeding a consumer would need the triangle in the packed LDS + register form of Tsqr2State).
// Merging inside the level-0 kernel when S == 1 was not built: it would save one launch of ~40 column steps' latency but
// needs a workgroup barrier between roles that never meet at one.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "figh_internal.h"
#include "figh_spatial.h"
#include "figh_chain.h"
#include "figh_wave.h"
#include "figh_tsqr_narrow.h"

namespace figh {

typedef double f64x2 __attribute__((ext_vector_type(2)));

struct FusedCtrl {  // one per producer / tile buffer
    int produced;  // tiles announced so far (written by the producer only)
    int taken;     // tiles whose gather is finished (written by the consumer that claimed the tile)
    int claimed;   // tiles claimed so far (compare-and-swap by the consumers: only announced tiles are claimed)
    int pad[5];
};

__device__ __forceinline__ int lds_peek(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_post(int *p, int v) {
    // LDS executes one wave's instructions in order: everything this wave read or wrote in LDS before this store is done
    // when the store is.  Only the compiler has to be kept from moving accesses across it.
    asm volatile("" ::: "memory");
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    asm volatile("" ::: "memory");
}

// a wave-uniform double the optimiser may not look through: uniform products of the tree constants (a_i a_j of the
// Rodrigues formula) would otherwise be hoisted out of the sample loop into VECTOR registers, 2 per value
__device__ __forceinline__ double opaque_s(double x) {
    asm volatile("" : "+s"(x));
    return x;
}

// the same for a value that is to live in a vector register from here on: whatever is computed from it stays inside the loop
// iteration that computes it (hoisted, such values are spilled to scratch, and a scratch reload waits -- in-order vmcnt --
// for every global store the wave has in flight)
__device__ __forceinline__ double opaque_v(double x) {
    asm volatile("" : "+v"(x));
    return x;
}

// Row block of the jo-th row tile of a sample tile: 0, NJ-1, 1, NJ-2, ... -- a row block of joint 1 costs a consumer ten
// times what one of joint 6 costs (104 against 11 chunk-steps for UR10), and with only one tile of slack per producer the
// consumers would all be busy during the heavy half of a sample tile and all be waiting during the light half.
template <int NJ>
constexpr int fused_row_of(int jo) { return (jo & 1) ? NJ - 1 - (jo >> 1) : (jo >> 1); }

template <int NJ>
struct FusedGeom {
    static constexpr int NC = 14 * NJ;
    static constexpr int LDT = NC + 2;  // LDS row stride (doubles); column NC carries the row's tau entry
    static constexpr int CH = NC / 2;   // 16-byte store chunks per row
    static constexpr int NPROD = 2;
    // LDS map (doubles), per producer: tile | tau of the sample tile's NJ rows | q', q'' | column-norm accumulators | control
    static constexpr int TILE = 64 * LDT;
    static constexpr int TAU0 = TILE;
    static constexpr int QD0 = TAU0 + 64 * NJ;
    static constexpr int CS0 = QD0 + 2 * 64 * NJ;
    static constexpr int CTRL0 = CS0 + ((NC + 7) / 8) * 8;
    static constexpr int PSIZE = CTRL0 + (int)(sizeof(FusedCtrl) / sizeof(double));
    static constexpr int CONS0 = NPROD * PSIZE;
};

// TRAJ (figh_regressor_tsqr_batch_fused): grid (S, B) -- workgroup (s, b) walks the sample tiles s, s + S, ... of trajectory
// b, whose N samples start at sample b N of q, v, a.  The producers only emit and announce tiles: W, tau, colsq_part are
// unused (no stream-out, no column norms), nc == n.  Everything else -- tile order, claims, column steps -- is the code of
// the identification launch, which TRAJ = false leaves exactly as it was.
template <int NJ, bool TRAJ = false>
__global__ __launch_bounds__(512) void fused_chain_tsqr_kernel(
    const ChainParams<NJ> P, const int flags, const long N, const double *__restrict__ q, const double *__restrict__ v,
    const double *__restrict__ a, double *__restrict__ W, const double *__restrict__ tau, const int *__restrict__ col_idx,
    const int n, const int nc, double *__restrict__ colsq_part, double *__restrict__ Rws, const int ncons,
    const int tri_doubles, const double null2) {
    using G = FusedGeom<NJ>;
    constexpr int NC = G::NC, LDT = G::LDT, CH = G::CH;
    constexpr int NCC = 4, NRC = 4, RPL = 16;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long ntiles_s = (N + 63) / 64;  // sample tiles
    const long b = blockIdx.x, Gd = gridDim.x;
    long wg = b;  // this workgroup's place in Rws
    if constexpr (TRAJ) {
        const long first = (long)blockIdx.y * N * NJ;  // the trajectory's samples
        q += first;
        v += first;
        a += first;
        wg = (long)blockIdx.y * Gd + b;
    }
    // this workgroup's sample tiles: b, b + Gd, ...; producer p takes every other one, starting with its p-th
    const long count_s = b < ntiles_s ? (ntiles_s - b + Gd - 1) / Gd : 0;
    const int T0 = (int)(((count_s + 1) / 2) * NJ), T1 = (int)((count_s / 2) * NJ);  // row tiles of producer 0 / 1

    // zero: accumulators, control words, the consumers' triangles and scratch
    for (int pz = 0; pz < G::NPROD; ++pz)
        for (int e = pz * G::PSIZE + G::CS0 + threadIdx.x; e < (pz + 1) * G::PSIZE; e += blockDim.x) lds[e] = 0.0;
    for (int e = G::CONS0 + threadIdx.x; e < G::CONS0 + ncons * tri_doubles; e += blockDim.x) lds[e] = 0.0;
    __syncthreads();

    if (wave < G::NPROD) {
        // ================================================================================================== producers
        __builtin_amdgcn_s_setprio(3);
        const bool fric = flags & FIGH_FLAG_FRICTION, actin = flags & FIGH_FLAG_ACT_INERTIA, offs = flags & FIGH_FLAG_OFFSET;
        double *tile = lds + wave * G::PSIZE;
        FusedCtrl *ctrl = reinterpret_cast<FusedCtrl *>(tile + G::CTRL0);
        double *my = tile + lane * LDT;
        double *stau = tile + G::TAU0, *sqd = tile + G::QD0, *cacc = tile + G::CS0;
        int t = 0;
        auto sample_tile = [&](auto FAST_T, const long s) {
            constexpr bool FAST = decltype(FAST_T)::value;
            const long i0 = s * 64;
            const int nvalid = FAST ? 64 : (int)((N - i0) < 64 ? (N - i0) : 64);
            const bool live = FAST || lane < nvalid;
            const long is = i0 + (live ? lane : nvalid - 1);
            double cs[NJ], sn[NJ];
            double acc[NJ][3], dw[NJ][3], w[NJ][3];
            {
                double pq[NJ], pqd[NJ], pqdd[NJ];
#pragma unroll
                for (int k = 0; k < NJ; ++k) {
                    pq[k] = q[is * NJ + k];
                    pqd[k] = v[is * NJ + k];
                    pqdd[k] = a[is * NJ + k];
                }
                if (!TRAJ && tau) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const double tv = tau[(long)j * N + is];
                        stau[64 * j + lane] = live ? tv : 0.0;
                    }
                }
#pragma unroll
                for (int k = 0; k < NJ; ++k) {
                    sqd[64 * (2 * k) + lane] = pqd[k];
                    sqd[64 * (2 * k + 1) + lane] = pqdd[k];
                }
                // forward recursion (regressor_chain_kernel, statement for statement -- and kept as text in both kernels: as an
                // inlined helper it moved the register allocation of either, see the note at the row entries below)
                double vl[3] = {0, 0, 0}, om[3] = {0, 0, 0}, da[3] = {0, 0, 0};
                double al[3] = {opaque_v(-P.g[0]), opaque_v(-P.g[1]), opaque_v(-P.g[2])};
#pragma unroll
                for (int k = 0; k < NJ; ++k) {
                    double s_, c_;
                    sincos_angle(pq[k], &s_, &c_);
                    cs[k] = c_;
                    sn[k] = s_;
                    double Rj[9], R[9];
                    const double ax[3] = {opaque_s(P.axis[k][0]), opaque_s(P.axis[k][1]), opaque_s(P.axis[k][2])};
                    rodrigues(ax, c_, s_, Rj);
                    matmul3(P.Rp[k], Rj, R);
                    double t1[3], t2[3], nvl[3], nom[3], nal[3], nda[3];
                    cross3(P.pp[k], om, t1);
#pragma unroll
                    for (int d = 0; d < 3; ++d) t2[d] = vl[d] - t1[d];
                    rotT(R, t2, nvl);
                    rotT(R, om, nom);
                    cross3(P.pp[k], da, t1);
#pragma unroll
                    for (int d = 0; d < 3; ++d) t2[d] = al[d] - t1[d];
                    rotT(R, t2, nal);
                    rotT(R, da, nda);
                    double vj[3] = {P.axis[k][0] * pqd[k], P.axis[k][1] * pqd[k], P.axis[k][2] * pqd[k]};
#pragma unroll
                    for (int d = 0; d < 3; ++d) nom[d] += vj[d];
                    cross3(nvl, vj, t1);
                    cross3(nom, vj, t2);
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        nal[d] += t1[d];
                        nda[d] += P.axis[k][d] * pqdd[k] + t2[d];
                        vl[d] = nvl[d];
                        om[d] = nom[d];
                        al[d] = nal[d];
                        da[d] = nda[d];
                    }
                    cross3(om, vl, t1);
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        acc[k][d] = al[d] + t1[d];
                        dw[k][d] = da[d];
                        w[k][d] = om[d];
                    }
                }
            }
#pragma unroll
            for (int jo = 0; jo < NJ; ++jo) {
                const int j = fused_row_of<NJ>(jo), jprev = fused_row_of<NJ>(jo == 0 ? NJ - 1 : jo - 1);
                // the buffer is free once the previous tile has been gathered by its consumer (this wave's own reads of it
                // -- stream-out, column norms -- are behind it in program order)
                while (lds_peek(&ctrl->taken) < t) __builtin_amdgcn_s_sleep(1);
                asm volatile("" ::: "memory");
                // ---- this lane's row (j, i): 14 columns per link; links < j are structurally zero.  The buffer holds the row
                // of joint jprev (zeros below 14 jprev, values from there on; the kernel's very first tile is row 0, which
                // writes every column): only [14 jprev, 14 j) has to be cleared
                if (j > jprev) {
#pragma unroll
                    for (int c = 14 * jprev; c < 14 * j; c += 2) *reinterpret_cast<f64x2 *>(my + c) = f64x2{0.0, 0.0};
                }
                double Jl[3] = {0, 0, 0}, Ja[3] = {opaque_v(P.axis[j][0]), opaque_v(P.axis[j][1]), opaque_v(P.axis[j][2])};
#pragma unroll
                for (int k = j; k < NJ; ++k) {
                    if (k > j) {
                        // (opaque to the optimiser: the rotation is re-formed for every row instead of being kept for all
                        // rows -- 54 doubles this wave has no registers for)
                        asm volatile("" : "+v"(cs[k]), "+v"(sn[k]));
                        double Rj[9], R[9];
                        const double ax[3] = {opaque_s(P.axis[k][0]), opaque_s(P.axis[k][1]), opaque_s(P.axis[k][2])};
                        rodrigues(ax, cs[k], sn[k], Rj);
                        matmul3(P.Rp[k], Rj, R);
                        double t1[3], t2[3], nJl[3], nJa[3];
                        cross3(P.pp[k], Ja, t1);
#pragma unroll
                        for (int d = 0; d < 3; ++d) t2[d] = Jl[d] - t1[d];
                        rotT(R, t2, nJl);
                        rotT(R, Ja, nJa);
#pragma unroll
                        for (int d = 0; d < 3; ++d) {
                            Jl[d] = nJl[d];
                            Ja[d] = nJa[d];
                        }
                    }
                    // (not axis_times_body_regressor, figh_spatial.h, which regressor_chain_kernel calls: through it another
                    // product of each sum is contracted into the FMA here and W changes by one rounding.  The forward step and
                    // the row-block recursion are hand copies for a like reason: as shared inlined helpers they changed VGPR
                    // and spill counts of this kernel and of regressor_chain_kernel, profiles/dedupe_ab.txt)
                    double o[14];
                    o[9] = Jl[0] * acc[k][0] + Jl[1] * acc[k][1] + Jl[2] * acc[k][2];
                    double h1[3], h2[3], h3[3], h4[3];
                    cross3(Jl, dw[k], h1);
                    cross3(w[k], Jl, h2);
                    cross3(w[k], h2, h3);
                    cross3(acc[k], Ja, h4);
                    o[6] = h1[0] + h3[0] + h4[0];
                    o[7] = h1[1] + h3[1] + h4[1];
                    o[8] = h1[2] + h3[2] + h4[2];
                    double u[3];
                    cross3(w[k], Ja, u);
                    const double *x = dw[k], *z = w[k];
                    o[0] = x[0] * Ja[0] - z[0] * u[0];
                    o[1] = x[1] * Ja[0] + x[0] * Ja[1] - (z[1] * u[0] + z[0] * u[1]);
                    o[3] = x[1] * Ja[1] - z[1] * u[1];
                    o[2] = x[2] * Ja[0] + x[0] * Ja[2] - (z[2] * u[0] + z[0] * u[2]);
                    o[4] = x[2] * Ja[1] + x[1] * Ja[2] - (z[2] * u[1] + z[1] * u[2]);
                    o[5] = x[2] * Ja[2] - z[2] * u[2];
                    if (k == j) {  // Ia fv fs off: only on the link's own row (regressor.py:55-70,84-87)
                        const double qdk = sqd[64 * (2 * k) + lane], qddk = sqd[64 * (2 * k + 1) + lane];
                        o[10] = actin ? qddk : 0.0;
                        o[11] = fric ? qdk : 0.0;
                        o[12] = fric ? sgn(qdk) : 0.0;
                        o[13] = offs ? 1.0 : 0.0;
                    } else {
                        o[10] = o[11] = o[12] = o[13] = 0.0;
                    }
                    double *dst = my + 14 * k;
#pragma unroll
                    for (int c = 0; c < 14; ++c) dst[c] = live ? o[c] : 0.0;
                }
                if constexpr (!TRAJ) my[NC] = tau ? stau[64 * j + lane] : 0.0;  // (TRAJ: nc == n, the slot is never gathered)
                lds_post(&ctrl->produced, t + 1);
                ++t;
                if constexpr (TRAJ) continue;  // no W: the tile lives and dies in LDS

                // ---- stream the 64 x NC tile to W rows j*N+i0 .. : one contiguous run (the launcher guarantees ldw == NC and
                // 16-byte alignment).  Chunk id (16 B) sits at byte 16 id in W and at 16 (id + r) in the padded tile,
                // r = id / CH by a magic multiply
                double *dstW = W + ((long)j * N + i0) * NC;
                const char *tbase = reinterpret_cast<const char *>(tile);
                if constexpr (FAST) {
                    // R rows per two passes of the wave, R = 128 / CH (UR10: three rows = 126 chunks of 16 B; seven links: two rows
                    // = 98): pass A takes slots 0..63 of the R rows, pass B slots 64..127 -- the slots behind R CH are the first
                    // chunks of the NEXT row (written again, with the same bytes, by the next group's pass A; masked in the last
                    // group when no row is left over).  A slot's place in the padded tile is then one per-lane constant per pass
                    // + a compile-time offset per row group: two address registers for the whole stream-out and no branches,
                    // where chunk id -> (id + id / CH) needs one register per chunk (42 the producer does not have) or 5 VALU
                    // operations per chunk.  Every pass is one contiguous 1 KB run in W.  64 % R rows are left over: lanes < CH.
                    constexpr int RG = 128 / CH;           // rows per group
                    constexpr int NG = 64 / RG;            // groups
                    constexpr int LEFT = 64 - NG * RG;     // rows behind the last group
                    static_assert(CH <= 64 && RG * CH > 64 && 128 - RG * CH <= CH && LEFT <= 1, "R rows per two passes");
                    constexpr int ROWB = LDT * 8;
                    const unsigned sa = lane, sb = lane + 64;
                    const unsigned ra = sa / CH, rb = sb / CH;
                    const unsigned la = ra * ROWB + 16u * (sa - ra * CH);
                    const unsigned lb = rb * ROWB + 16u * (sb - rb * CH);
                    char *gbase = reinterpret_cast<char *>(dstW) + 16 * lane;
                    constexpr int GRP = RG * CH * 16;  // bytes of a row group in W
                    constexpr int BATCH = NG % 3 == 0 ? 3 : 4;  // 2 BATCH reads in flight, then 2 BATCH stores
                    static_assert(NG % BATCH == 0, "row groups per batch");
#pragma unroll
                    for (int g0 = 0; g0 < NG; g0 += BATCH) {
                        f64x2 va[BATCH], vb[BATCH];
#pragma unroll
                        for (int u = 0; u < BATCH; ++u) {
                            va[u] = *reinterpret_cast<const f64x2 *>(tbase + la + (g0 + u) * RG * ROWB);
                            vb[u] = *reinterpret_cast<const f64x2 *>(tbase + lb + (g0 + u) * RG * ROWB);
                        }
#pragma unroll
                        for (int u = 0; u < BATCH; ++u) {
                            *reinterpret_cast<f64x2 *>(gbase + (g0 + u) * GRP) = va[u];
                            // (the last group has no next row to run into unless one is left over)
                            if (LEFT > 0 || g0 + u + 1 < NG || sb < (unsigned)(RG * CH))
                                *reinterpret_cast<f64x2 *>(gbase + (g0 + u) * GRP + 1024) = vb[u];
                        }
                    }
                    if constexpr (LEFT > 0) {
                        if (lane < CH) {
                            const f64x2 vc = *reinterpret_cast<const f64x2 *>(tbase + 63 * ROWB + 16 * lane);
                            *reinterpret_cast<f64x2 *>(gbase + NG * GRP) = vc;
                        }
                    }
                } else {
                    constexpr unsigned MAGIC = ((1u << 20) + CH - 1) / CH;
                    static_assert(64 * CH <= 4096, "magic division range");
                    const int total = nvalid * CH;
                    for (int id = lane; id < total; id += 64) {
                        const unsigned r = ((unsigned)id * MAGIC) >> 20;
                        const double2 val = *reinterpret_cast<const double2 *>(tbase + 16u * (id + r));
                        *reinterpret_cast<double2 *>(reinterpret_cast<char *>(dstW) + 16 * id) = val;
                    }
                }
                // ---- diag(W^T W): on joint row j the live columns are 14 j ..; lane owns 14 j + lane (and + 64)
                {
                    const int lo = 14 * j, width = NC - lo;
                    // RB rows requested at a time (the LDS latency is paid 64 / RB times per pass, not 64 times); sixteen where
                    // the registers allow it -- with six links the producer is at the 256-register limit exactly here and
                    // sixteen cost two spilled registers whose reloads wait behind the stores in flight: eight
                    constexpr int RB = NJ >= 6 ? 8 : 16;
                    auto column_sum = [&](const double *col) {
                        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
#pragma unroll
                        for (int r0 = 0; r0 < 64; r0 += RB) {
                            double x[RB];
#pragma unroll
                            for (int r = 0; r < RB; ++r) x[r] = col[(r0 + r) * LDT];
#pragma unroll
                            for (int r = 0; r < RB; ++r) asm volatile("" : "+v"(x[r]));
#pragma unroll
                            for (int r = 0; r < RB; r += 4) {
                                t0 += x[r] * x[r];
                                t1 += x[r + 1] * x[r + 1];
                                t2 += x[r + 2] * x[r + 2];
                                t3 += x[r + 3] * x[r + 3];
                            }
                        }
                        return (t0 + t1) + (t2 + t3);
                    };
                    if (lane < width) cacc[lo + lane] += column_sum(tile + lo + lane);
                    if (width > 64 && lane + 64 < width) cacc[lo + 64 + lane] += column_sum(tile + lo + 64 + lane);
                }
            }
        };
        for (long s = b + wave * Gd; s < ntiles_s; s += G::NPROD * Gd) {
            if ((s + 1) * 64 <= N) sample_tile(std::true_type{}, s);
            else sample_tile(std::false_type{}, s);
        }
        asm volatile("" ::: "memory");
        if constexpr (!TRAJ)
            for (int c = lane; c < NC; c += 64) colsq_part[(b * G::NPROD + wave) * NC + c] = cacc[c];
        return;
    }
    // ======================================================================================================= consumers
    const int c_id = wave - G::NPROD;
    const int pad = 16 * NCC - nc;
    Tsqr2State<NCC, NRC, true> S;  // (RLAST form: the last chunk of the triangle in registers)
    tsqr2_state_init(S, lds + G::CONS0 + c_id * tri_doubles, lane, nc, null2);
    // per-lane column sources inside an LDS tile: kept column col_idx[col] for col < n, the tau slot (column NC) for
    // col == n == nc - 1; padding lane-columns stay exactly zero for the whole kernel
    bool wlive[NCC];
    int loff[NCC];
#pragma unroll
    for (int cc = 0; cc < NCC; ++cc) {
        const int col = 16 * cc + S.lane_c - pad;
        wlive[cc] = col >= 0 && col < nc;
        const int src = (col >= 0 && col < n) ? col_idx[col] : NC;
        loff[cc] = S.lane_g * LDT + src;
    }
    // structure of the joint-torque regressor of a chain (regressor.py:45-87): the row block of joint j has exact zeros in the
    // columns of the links in front of j -- the producer writes them as such -- so a tile's first kept column that can be
    // non-zero is known from its row block: fpos[j] = pad + #{kept columns < 14 j}.  Chunks in front of it are not gathered.
    int fpos[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) fpos[j] = pad;
    for (int e = 0; e < n; ++e) {
        const int c = col_idx[e];
#pragma unroll
        for (int j = 1; j < NJ; ++j) fpos[j] += (c < 14 * j) ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) fpos[j] = __builtin_amdgcn_readfirstlane(fpos[j]);  // (uniform: scalar registers)
    FusedCtrl *ctrl0 = reinterpret_cast<FusedCtrl *>(lds + G::CTRL0);
    FusedCtrl *ctrl1 = reinterpret_cast<FusedCtrl *>(lds + G::PSIZE + G::CTRL0);

    int pref = c_id & 1;  // the buffer this wave looks at first
    int absorbed = 0;     // tiles this wave has factored
    for (;;) {
        // claim the next announced tile of either buffer (lane 0 decides, the wave follows): -1 = everything is claimed
        int pick = -2, tpick = 0;
        while (pick == -2) {
            int res = -2, tres = 0;
            if (lane == 0) {
                bool done = true;
#pragma unroll
                for (int tr = 0; tr < 2; ++tr) {
                    const int pb = pref ^ tr;
                    FusedCtrl *cp = pb ? ctrl1 : ctrl0;
                    const int Tp = pb ? T1 : T0;
                    int cl = lds_peek(&cp->claimed);
                    if (cl < Tp) {
                        done = false;
                        if (res == -2 && lds_peek(&cp->produced) > cl &&
                            __hip_atomic_compare_exchange_strong(&cp->claimed, &cl, cl + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                 __HIP_MEMORY_SCOPE_WORKGROUP)) {
                            res = pb;
                            tres = cl;
                        }
                    }
                }
                if (done) res = -1;
            }
            pick = __builtin_amdgcn_readfirstlane(res);
            tpick = __builtin_amdgcn_readfirstlane(tres);
            if (pick == -2) __builtin_amdgcn_s_sleep(1);
        }
        if (pick < 0) break;
        pref = pick ^ 1;  // alternate between the buffers
        asm volatile("" ::: "memory");
        const double *tile = lds + pick * G::PSIZE;
        FusedCtrl *ctrl = pick ? ctrl1 : ctrl0;
        const int jrow = fused_row_of<NJ>(tpick % NJ);  // row block of the tile
        int first_nz = fpos[0];
#pragma unroll
        for (int j = 1; j < NJ; ++j) first_nz = jrow == j ? fpos[j] : first_nz;
        first_nz = __builtin_amdgcn_readfirstlane(first_nz);
#pragma unroll
        for (int cc = 0; cc < NCC; ++cc) {
            // (cleared first: what the previous tile left in the registers is dead, no merge with it)
#pragma unroll
            for (int i = 0; i < RPL; ++i) S.T[cc][i] = 0.0;
            // a chunk whose lane-columns all lie in front of first_nz holds structural zeros only (wave-uniform test)
            if (wlive[cc] && 16 * cc + 15 >= first_nz) {
#pragma unroll
                for (int i = 0; i < RPL; ++i) S.T[cc][i] = tile[(16 * (i >> 2) + 4 * (i & 3)) * LDT + loff[cc]];
            }
        }
        // the values are in registers before the buffer is handed back
#pragma unroll
        for (int cc = 0; cc < NCC; ++cc)
#pragma unroll
            for (int i = 0; i < RPL; ++i) asm volatile("" : "+v"(S.T[cc][i]));
        lds_post(&ctrl->taken, tpick + 1);
        S.null2 = tsqr2_null2_at(absorbed, 64, nc, null2);
        ++absorbed;
        tsqr2_panels<0, NCC, NRC, false, true>(S, first_nz, [](auto) {});
    }
    tsqr2_store_triangle(S, Rws + (wg * ncons + c_id) * (long)nc * nc, nc, pad, lane);
}

// One merge level of the batched form: workgroup (bl, b) factors the stacked rows [512 bl, 512 (bl + 1)) of trajectory b's
// input -- `rows` rows of its own triangles (Rs + b * rows * nc), then, when `extra` is given, the nc rows of that
// triangle, the same for every trajectory -- into triangle bl of the trajectory's gridDim.x outputs: tsqr_coop_factor<4, 8>
// over the two sources; the zero fill leaves exact zeros below the diagonal.
__global__ __launch_bounds__(512) void fused_batch_merge_kernel(const double *__restrict__ Rs, const long rows,
                                                                const double *__restrict__ extra, const int nc,
                                                                double *__restrict__ Rout) {
    const double *mine = Rs + (long)blockIdx.y * rows * nc;
    const long rows_all = rows + (extra ? nc : 0);
    double *Rg = Rout + ((long)blockIdx.y * gridDim.x + blockIdx.x) * nc * nc;
    tsqr_coop_factor<4, 8>((long)blockIdx.x, nc, Rg, [&](const long row, const int col) {
        const bool ok = row < rows_all && col >= 0;
        const double *src = row < rows ? mine + row * nc : extra + (row - rows) * nc;
        return ok ? src[col] : 0.0;
    });
}

// What both launchers need of the level-0 kernel: the chain constants, the LDS doubles per consumer (the RLAST triangle of
// four chunks, tsqr2_tri_doubles), the consumer waves per workgroup -- what fits behind the producers' doubles in 160 KB
// of LDS, at most six -- and the dynamic LDS of the launch, which the kernel is allowed once per instantiation.
template <int NJ>
struct FusedPlan {
    ChainParams<NJ> P;
    int tri, ncons;
    size_t lds;
};

template <int NJ, bool TRAJ>
static int fused_plan(const figh_model_s *m, int nc, FusedPlan<NJ> *plan) {
    constexpr size_t fixed = FusedGeom<NJ>::CONS0, budget = (160 * 1024) / sizeof(double);
    const size_t tri = (size_t)tsqr2_tri_doubles(4, nc, true);
    const int ncons = (int)std::min<size_t>(6, (budget - fixed) / tri);
    if (ncons < 3) {
        set_error(std::string(TRAJ ? "fused batch regressor + TSQR" : "fused regressor + TSQR") +
                  ": the triangles of three consumer waves do not fit next to the tile");
        return FIGH_ERR_UNSUPPORTED;
    }
    static bool attr_set = false;
    if (!attr_set) {
        FIGH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&fused_chain_tsqr_kernel<NJ, TRAJ>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    plan->P = chain_params<NJ>(m);
    plan->tri = (int)tri;
    plan->ncons = ncons;
    plan->lds = sizeof(double) * (fixed + (size_t)ncons * tri);
    return FIGH_OK;
}

template <int NJ>
static int launch_fused(const figh_model_s *m, int flags, long N, const double *q, const double *v, const double *a,
                        double *W, const double *tau, const int *d_kept, int n, double *d_colsq, double **Rws_out,
                        long *count_out, const double **part_out, int *nparts_out) {
    using G = FusedGeom<NJ>;
    const int nc = n + (tau ? 1 : 0);
    FusedPlan<NJ> pl;
    if (int rc = fused_plan<NJ, false>(m, nc, &pl)) return rc;
    const int cus = cu_count(), ncons = pl.ncons;
    const long ntiles_s = (N + 63) / 64;
    long grid = cus < ntiles_s / 2 ? cus : ntiles_s / 2;  // (at least two sample tiles = 12 row tiles per workgroup)
    double *part = static_cast<double *>(workspace(sizeof(double) * grid * G::NPROD * G::NC, kWsRegressorNorms));
    double *Rws = static_cast<double *>(workspace(sizeof(double) * (size_t)nc * nc * (grid * ncons + 1), kWsLevel0TriOrWrench));
    if (!part || !Rws) return FIGH_ERR_ALLOC;
    {
        ProfileScope scope("fused_chain_tsqr", true);
        FIGH_LAUNCH_TIMED((fused_chain_tsqr_kernel<NJ, false>), dim3((unsigned)grid), dim3(64 * (G::NPROD + ncons)), pl.lds,
                          pl.P, flags, N, q, v, a, W, tau, d_kept, n, nc, part, Rws, ncons, pl.tri, null_pivot_sq());
    }
    // (part_out: the caller sums the partials itself -- figh_chain_pass_fused, in its merge launch)
    if (part_out) {
        *part_out = part;
        *nparts_out = (int)(grid * G::NPROD);
    } else {
        launch_reduce_partials(part, (int)(grid * G::NPROD), G::NC, d_colsq);
    }
    FIGH_HIP(hipGetLastError());
    *Rws_out = Rws;
    *count_out = grid * ncons;
    return FIGH_OK;
}

// Slices per trajectory of the batched launch.  One workgroup occupies a CU (152 KB of LDS), so B workgroups fill the chip
// when B >= CUs: S = 1, a trajectory is one workgroup and its merge one level.  Below that a trajectory is cut into
// S = CUs / B slices (rounded down: one round of the chip), at most one per sample tile -- a slice of a single tile leaves
// producer 1 idle, which costs less than a CU that has no workgroup at all.  (tests/test_objective_batch_fused.py mirrors it.)
static long fused_batch_slices(long B, long n_per, int cus) {
    const long tiles = (n_per + 63) / 64;
    return std::max(1L, std::min(tiles, (long)cus / B));
}

template <int NJ>
static int launch_fused_batch(const figh_model_s *m, int flags, long B, long n_per, const double *q, const double *v,
                              const double *a, const int *d_cols, int n, const double *d_R_stack, double *d_R_out) {
    using G = FusedGeom<NJ>;
    const int nc = n;
    FusedPlan<NJ> pl;
    if (int rc = fused_plan<NJ, true>(m, nc, &pl)) return rc;
    const int ncons = pl.ncons;
    const long S = fused_batch_slices(B, n_per, cu_count());
    const size_t tsz = sizeof(double) * (size_t)nc * nc;
    double *Rws = static_cast<double *>(workspace(tsz * (size_t)(B * S * ncons), kWsFusedBatchTri));
    if (!Rws) return FIGH_ERR_ALLOC;
    {
        ProfileScope scope("fused_chain_tsqr_batch", true);
        FIGH_LAUNCH_TIMED((fused_chain_tsqr_kernel<NJ, true>), dim3((unsigned)S, (unsigned)B), dim3(64 * (G::NPROD + ncons)),
                          pl.lds, pl.P, flags, n_per, q, v, a, (double *)nullptr, (const double *)nullptr, d_cols, n, nc,
                          (double *)nullptr, Rws, ncons, pl.tri, null_pivot_sq());
    }
    FIGH_HIP(hipGetLastError());
    // merge levels: cnt triangles per trajectory (+ d_R_stack at the first level) -> ceil(rows / 512) -> ... -> 1
    const double *cur = Rws, *extra = d_R_stack;
    long cnt = S * ncons;
    WorkspaceSlot slot = kWsMergeA;
    for (;;) {
        ProfileScope scope("tsqr_reduce");
        const long rows = cnt * nc;
        const long nb = (rows + (extra ? nc : 0) + 511) / 512;
        double *dst = nb == 1 ? d_R_out : static_cast<double *>(workspace(tsz * (size_t)(B * nb), slot));
        if (!dst) return FIGH_ERR_ALLOC;
        hipLaunchKernelGGL(fused_batch_merge_kernel, dim3((unsigned)nb, (unsigned)B), dim3(512), 0, stream(), cur, rows, extra,
                           nc, dst);
        FIGH_HIP(hipGetLastError());
        if (nb == 1) return FIGH_OK;
        cur = dst;
        cnt = nb;
        extra = nullptr;
        slot = slot == kWsMergeA ? kWsMergeB : kWsMergeA;
    }
}

}  // namespace figh

using namespace figh;

// the checks and the launch of figh_regressor_tsqr_fused / figh_chain_pass_fused
static int fused_pass_launch(figh_model_t model, int flags, int64_t N, const double *d_q, const double *d_v, const double *d_a,
                             double *d_W, int64_t ldw, double *d_colsq, const int32_t *d_kept, int n, const double *d_tau,
                             double **Rws, long *count, const double **part = nullptr, int *nparts = nullptr) {
    FIGH_REQUIRE(N >= 0 && n >= 1, "bad shape");
    const DevModel &h = model->host;
    const int nc = n + (d_tau ? 1 : 0);
    const int ncols = 14 * h.nlinks;
    if (!model->is_chain || (flags & (FIGH_FLAG_TX40 | FIGH_FLAG_GENERIC | FIGH_FLAG_BLOCKED_INPUTS)) || ldw != ncols ||
        (reinterpret_cast<uintptr_t>(d_W) % 16) != 0 || nc > 64 || n > ncols || N < 4096) {
        set_error("fused regressor + TSQR: serial chain, joint-torque mode, packed 16-byte aligned W, at most 64 columns "
                  "(tau included) and at least 4096 samples");
        return FIGH_ERR_UNSUPPORTED;
    }
    if (int rc = ensure_device()) return rc;
    const int f = flags & 7;
    switch (h.nlinks) {
        case 5:
            return launch_fused<5>(model, f, (long)N, d_q, d_v, d_a, d_W, d_tau, d_kept, n, d_colsq, Rws, count, part, nparts);
        case 6:
            return launch_fused<6>(model, f, (long)N, d_q, d_v, d_a, d_W, d_tau, d_kept, n, d_colsq, Rws, count, part, nparts);
        case 7:
            return launch_fused<7>(model, f, (long)N, d_q, d_v, d_a, d_W, d_tau, d_kept, n, d_colsq, Rws, count, part, nparts);
        default:
            // (eight links: two 58 KB tile buffers leave 17 KB of the 160 KB of LDS, less than three consumer triangles)
            set_error("fused regressor + TSQR: serial chains of 5 to 7 joints (LDS: two tile buffers + three consumer triangles)");
            return FIGH_ERR_UNSUPPORTED;
    }
}

extern "C" int figh_regressor_tsqr_fused(figh_model_t model, int flags, int64_t N, const double *d_q, const double *d_v,
                                         const double *d_a, double *d_W, int64_t ldw, double *d_colsq,
                                         const int32_t *d_kept, int n, const double *d_tau, double tol_qr,
                                         double *d_R_out) {
    FIGH_REQUIRE(model && d_q && d_v && d_a && d_W && d_colsq && d_kept && d_R_out, "NULL pointer");
    double *Rws = nullptr;
    long count = 0;
    if (int rc = fused_pass_launch(model, flags, N, d_q, d_v, d_a, d_W, ldw, d_colsq, d_kept, n, d_tau, &Rws, &count))
        return rc;
    return tsqr_reduce_stack(Rws, count, n + (d_tau ? 1 : 0), n, tol_qr, d_R_out);
}

extern "C" int figh_chain_pass_fused(figh_model_t model, int flags, int64_t N, const double *d_q, const double *d_v,
                                     const double *d_a, double *d_W, int64_t ldw, const int32_t *d_kept, int n,
                                     const double *d_tau, double tol_qr, double tol_e, double *d_pack, double *h_pack,
                                     size_t pack_bytes, const uint8_t *h_kept_mask, int *changed, figh_host_tail_t *tail) {
    FIGH_REQUIRE(model && d_q && d_v && d_a && d_W && d_kept && d_pack && h_pack && h_kept_mask && changed && tail,
                 "NULL pointer");
    FIGH_REQUIRE(tol_qr >= 0.0, "figh_chain_pass_fused: the rank decision needs tol_qr >= 0");
    const int ncols = 14 * model->host.nlinks, nc = n + (d_tau ? 1 : 0);
    const size_t sel_words = (size_t)(2 + 2 * ncols + 1) / 2;
    const size_t words = (size_t)ncols + sel_words + (size_t)(nc > 0 ? (nc + 1) * nc : 0);
    FIGH_REQUIRE(n >= 1 && pack_bytes >= sizeof(double) * words, "figh_chain_pass_fused: the pack is [colsq | sel | rows]");
    FIGH_REQUIRE(tail->n == n && (tail->with_tau != 0) == (d_tau != nullptr), "figh_chain_pass_fused: tail of another shape");
    // Where the kernels store the pack: page-locked host memory (figh_host_alloc) has a device address, and the pack is
    // stored there directly -- nothing is copied, d_pack is not touched.  Pageable memory has none: d_pack, then one copy.
    double *pack = nullptr;
    const bool on_host = hipHostGetDevicePointer(reinterpret_cast<void **>(&pack), h_pack, 0) == hipSuccess && pack;
    if (!on_host) {
        (void)hipGetLastError();
        pack = d_pack;
    }
    double *Rws = nullptr;
    const double *part = nullptr;
    long count = 0;
    int nparts = 0;
    if (int rc = fused_pass_launch(model, flags, N, d_q, d_v, d_a, d_W, ldw, d_pack, d_kept, n, d_tau, &Rws, &count, &part, &nparts))
        return rc;
    // One stream, two launches: the fused kernel, then the merge launch, which starts when the fused kernel has ended (plain
    // stream order) and whose last workgroup sums the norms and selects the columns beside the tree -- neither depends on
    // the other, and nothing on the device waits for another launch.  The end of the merge launch is the end of the pass.
    StreamEpilogue ep{};
    ep.part = part;
    ep.nblocks = nparts;
    ep.ncols = ncols;
    ep.tol_e = tol_e;
    ep.link_stride = 14;
    ep.colsq = pack;
    ep.sel = reinterpret_cast<int32_t *>(pack + ncols);
    ep.rows_on_host = on_host ? 1 : 0;
    int rc = tsqr_reduce_stack_epilogue(Rws, count, nc, n, tol_qr, pack + ncols + sel_words, ep);
    if (rc == FIGH_ERR_UNSUPPORTED && on_host) {
        // the tree is not resident in one launch with that workgroup: the separate steps, through d_pack
        pack = d_pack;
        ep.colsq = pack;
        ep.sel = reinterpret_cast<int32_t *>(pack + ncols);
        ep.rows_on_host = 0;
        rc = tsqr_reduce_stack_epilogue(Rws, count, nc, n, tol_qr, pack + ncols + sel_words, ep);
    }
    if (rc) return rc;
    if (pack == d_pack) FIGH_HIP(hipMemcpyAsync(h_pack, d_pack, sizeof(double) * words, hipMemcpyDeviceToHost, stream()));
    FIGH_HIP(hipStreamSynchronize(stream()));
    const int32_t *mask_now = reinterpret_cast<const int32_t *>(h_pack + ncols) + 2 + ncols;
    *changed = 0;
    for (int c = 0; c < ncols; ++c)
        if ((mask_now[c] != 0) != (h_kept_mask[c] != 0)) {
            *changed = 1;
            return FIGH_OK;
        }
    tail->rows_k = h_pack + ncols + sel_words;
    return figh_chain_host_tail(tail);
}

// The smallest trajectory the batched launch takes: one full sample tile.  64 samples are at least 320 rows, more than the
// nc + 8 <= 72 rows from which level 0 applies the null-pivot rule, so a trajectory's triangle never depends on whether a
// consumer happened to see enough of its rows; shorter trajectories are mostly masked lanes and keep the two-launch path.
static constexpr int64_t kFusedBatchMinSamples = 64;

extern "C" int figh_regressor_tsqr_batch_fused(figh_model_t model, int flags, int64_t B, int64_t n_per, const double *d_q,
                                               const double *d_v, const double *d_a, const int32_t *d_col_idx, int n,
                                               const double *d_R_stack, double *d_R_out) {
    FIGH_REQUIRE(model && d_q && d_v && d_a && d_col_idx && d_R_out, "NULL pointer");
    FIGH_REQUIRE(B >= 1 && n_per >= 1 && n >= 1, "figh_regressor_tsqr_batch_fused: at least one trajectory, sample and column");
    const DevModel &h = model->host;
    if (!model->is_chain || h.nlinks < 5 || h.nlinks > 7) {
        // (eight links: two 58 KB tile buffers leave 17 KB of the 160 KB of LDS, less than three consumer triangles)
        set_error("fused batch regressor + TSQR: serial chains of 5 to 7 joints (LDS: two tile buffers + three consumer triangles)");
        return FIGH_ERR_UNSUPPORTED;
    }
    if (flags & (FIGH_FLAG_TX40 | FIGH_FLAG_GENERIC | FIGH_FLAG_BLOCKED_INPUTS)) {
        set_error("fused batch regressor + TSQR: joint-torque mode of the chain kernel only (no TX40 coupling, generic kernel or "
                  "tile-blocked inputs)");
        return FIGH_ERR_UNSUPPORTED;
    }
    if (n > 64) {
        set_error("fused batch regressor + TSQR: at most 64 columns");
        return FIGH_ERR_UNSUPPORTED;
    }
    if (n_per < kFusedBatchMinSamples) {
        set_error("fused batch regressor + TSQR: at least 64 samples (one full sample tile) per trajectory");
        return FIGH_ERR_UNSUPPORTED;
    }
    if (B > 65535) {
        set_error("fused batch regressor + TSQR: at most 65535 trajectories (one grid row each)");
        return FIGH_ERR_UNSUPPORTED;
    }
    if (int rc = ensure_device()) return rc;
    const int f = flags & 7;
    switch (h.nlinks) {
        case 5:
            return launch_fused_batch<5>(model, f, (long)B, (long)n_per, d_q, d_v, d_a, d_col_idx, n, d_R_stack, d_R_out);
        case 6:
            return launch_fused_batch<6>(model, f, (long)B, (long)n_per, d_q, d_v, d_a, d_col_idx, n, d_R_stack, d_R_out);
        case 7:
            return launch_fused_batch<7>(model, f, (long)B, (long)n_per, d_q, d_v, d_a, d_col_idx, n, d_R_stack, d_R_out);
        default:  // (refused above)
            return FIGH_ERR_UNSUPPORTED;
    }
}
