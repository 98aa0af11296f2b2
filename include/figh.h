/* figh.h -- C-ABI of libfigh.so: the MI355X (gfx950) regressor + QR/LS hot path of FIGAROH.
 *
 * The reference (thanhndv212/figaroh-plus) is pure Python and has no FFI; its boundary for this path is
 * the set of module-level functions listed below.  Each entry point names the
 * reference statement(s) it replaces (paths relative to the reference root).  The Python shim in
 * figaroh_plus_amd/ binds exactly these symbols with ctypes; INTEGRATION.md shows the stub a FIGAROH
 * maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative figh_status; figh_last_error() gives the text;
 *   - all matrices are float64, row-major ("C order"), leading dimension in elements;
 *   - pointers named d_* are DEVICE pointers obtained from figh_malloc (or any hipMalloc), pointers named
 *     h_* are host pointers; buffers are caller-owned, inputs are never written;
 *   - the library keeps one HIP stream per process (figh_stream); calls are asynchronous on it unless they
 *     return data to the host; it is not thread-safe;
 *   - there is NO CPU implementation behind this ABI: without a HIP device every compute entry fails
 *     with FIGH_ERR_NO_DEVICE.
 */
#ifndef FIGH_H
#define FIGH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    FIGH_OK = 0,
    FIGH_ERR_INVALID = -1,    /* bad argument (the reference would raise ValueError / AssertionError) */
    FIGH_ERR_NO_DEVICE = -2,  /* no HIP device / HIP runtime error */
    FIGH_ERR_ALLOC = -3,
    FIGH_ERR_UNSUPPORTED = -4,
    FIGH_ERR_COMM = -5
} figh_status;

/* joint types of figh_model_create (Pinocchio joint models reached through URDF) */
enum { FIGH_JT_REVOLUTE = 0, FIGH_JT_PRISMATIC = 1, FIGH_JT_CONTINUOUS = 2, FIGH_JT_FREEFLYER = 3, FIGH_JT_UNIVERSE = -1 };
/* regressor modes: param["is_joint_torques"] / param["is_external_wrench"] (regressor.py:45, :89) */
enum { FIGH_MODE_JOINT_TORQUE = 0, FIGH_MODE_EXT_WRENCH = 1 };
/* flags: param["has_friction"], ["has_actuator_inertia"], ["has_joint_offset"] (regressor.py:55-70, :144-169);
 * FIGH_FLAG_TX40 appends the 3 coupling columns of add_coupling_TX40 (regressor.py:198-227);
 * FIGH_FLAG_GENERIC forces the generic-tree kernel even when the serial-chain kernel applies (tests). */
enum { FIGH_FLAG_FRICTION = 1, FIGH_FLAG_ACT_INERTIA = 2, FIGH_FLAG_OFFSET = 4, FIGH_FLAG_TX40 = 8, FIGH_FLAG_GENERIC = 256,
       /* d_q / d_v / d_a are TILE-BLOCKED copies made by figh_repack_samples ([tile of 64 samples][value][lane]) instead of
        * the reference's sample-major arrays: the generic-tree kernel then reads one 512-byte line per value and wave
        * (sample-major, a lane's values lie nq * 8 bytes from its neighbour's and every 8-byte load pulls a line of its
        * own: 7.4x the algorithmic input bytes on TALOS).  Tree models only. */
       FIGH_FLAG_BLOCKED_INPUTS = 512,
       /* figh_regressor_build_padded only, OPT-IN: the caller guarantees that the structural zeros of W (the entries of a
        * row block outside its joint's subtree, joint-torque mode of a tree) already ARE zero in d_W -- a buffer it
        * zero-filled once and that nothing but this function writes -- so the kernel does not stream them again; every
        * entry that depends on q, v, a is written as always.  90 % of TIAGo's 73.7 GB are such zeros.  Not the default
        * of anything: a pass that re-creates every byte of W each time is what the pipeline and bench.py measure unless
        * asked otherwise. */
       FIGH_FLAG_ZEROS_PRESENT = 1024,
       /* figh_regressor_build_padded only: d_W is BLOCK-COMPACT -- the joint-torque regressor of a tree of single-dof joints
        * stored row block by row block, block j (the N rows of joint j + 1) as its own N x ld_j matrix holding the columns
        * of that joint's subtree (links j + 1 .. j + size_j, depth-first numbering: a contiguous window of the dense
        * link-padded row, ld_j = 16 size_j) at element offset N * (ld_0 + .. + ld_{j-1}).  Everything outside the window is
        * a structural zero that is neither stored nor read (figh_tsqr_selected_blocks with block offsets).  ldw is ignored;
        * d_colsq keeps the reference's column numbering.  TIAGo: 7.9 instead of 73.7 GB per 1e6 samples. */
       FIGH_FLAG_COMPACT_BLOCKS = 2048,
       /* figh_regressor_build_padded only, external-wrench regressor of a model with a free-flyer root: d_W is LINK-COMPACT --
        * only the links that can have a non-zero entry at all keep their 16-column segment (a body with mass and a selected
        * wrench component, or every link when a friction / inertia / offset flag is set; regressor.py:36-39, :142-169), in
        * link order: segment of link l at column 16 pos[l], ldw >= 16 * (number of such links), pos from
        * figh_regressor_link_layout.  The other links' columns -- structural zeros in all six row blocks, eliminated by
        * get_index_eliminate (regressor.py:258-279) whatever the samples -- are neither written nor read: human model
        * 19 x 16 = 304 instead of 40 x 16 = 640 columns (146 instead of 307 GB for 1e7 samples).  d_colsq keeps the
        * reference's numbering (exact zeros for the dropped links).  Consumers take the map as d_link_pos
        * (figh_tsqr_selected_wrench). */
       FIGH_FLAG_LINK_COMPACT = 4096,
       /* figh_regressor_build_padded only, external-wrench regressor of a model with a free-flyer root, no friction /
        * actuator-inertia / offset columns: d_W is FORCE-COMPACT -- the three FORCE row blocks (regressor.py:89-192: rows
        * c N + i, c = Fx Fy Fz) are stored in a region of their own, 3 N rows of ldf columns IN FRONT of the three torque
        * row blocks, one 128-byte line per FOUR links: the force rows of link l hold mx my mz m (reference columns 14 l + 6
        * .. 14 l + 9) at columns 16 (p / 4) + 4 (p % 4) + (s - 6) of that region, p = the link's position among the links
        * with entries (figh_regressor_link_layout), ldf from figh_regressor_force_layout -- everything a force row has:
        * the six rotational-inertia entries are exact zeros (a force does not depend on them).  The torque row blocks
        * follow at d_W + 3 N ldf: 3 N rows of ldw columns, link-padded (or link-compact with FIGH_FLAG_LINK_COMPACT).  A
        * quarter of the force-row lines: TALOS 101 -> 64 GB, human 146 -> 92 GB per pass.  Consumer:
        * figh_tsqr_selected_wrench(..., ld_force). */
       FIGH_FLAG_FORCE_COMPACT = 8192 };

typedef struct figh_model_s *figh_model_t;

/* ------------------------------------------------------------------ runtime plumbing (no reference equivalent) */
/* The ABI this header declares.  Bumped whenever an entry point changes its argument list or the meaning of an argument
 * (round 5 did so for figh_tsqr_selected_wrench / figh_regressor_build_padded without a bump: a library of the older ABI
 * accepts the longer argument list under cdecl and silently ignores the new arguments).  figaroh_plus_amd/_lib.py refuses a
 * library -- in-tree or FIGH_LIB_PATH -- whose figh_version() differs from the value it was written against. */
#define FIGH_ABI_VERSION 117
int figh_version(void);
const char *figh_last_error(void);
int figh_device_count(int *count);
int figh_device_set(int device);
/* How the host waits for the device in this process: 0 (default) = the runtime's spinning wait, lowest latency, one busy
 * CPU per process; 1 = interrupt-driven (hipDeviceScheduleBlockingSync).  For several ranks per node under a CPU quota
 * (figaroh_plus_amd/dist.py launches): eight spinning ranks plus their runtime threads reach a 16-CPU cgroup quota, and a
 * process that exhausts it is frozen until the next 100 ms accounting period.  Call before figh_device_set / any
 * device call.  No reference analogue (the reference has no device). */
int figh_host_wait_mode(int blocking);
/* Null-pivot rule of the Householder TSQR kernels (figh_tsqr*, figh_regressor_tsqr*): a pivot column whose norm at and below
 * the diagonal is <= tol -- sqrt(R_kk^2 + |x|^2) <= tol for the tile's part x of the column -- gets H = I (LAPACK dlarfg's
 * rule for an exactly zero x, with a threshold): its norm is folded into R_kk, the column leaves the tile, no reflector
 * is formed and no trailing update is made.  R_kk therefore carries the running residual norm of the column and the test
 * includes it, so that INSIDE ONE LEVEL-0 TRIANGLE at most tol of a column's norm is ever folded.  Every level-0 triangle
 * -- one per wave (register-tile kernel), per workgroup (blocked kernel), per consumer wave (fused launch) and per sample
 * chunk of a streamed run -- starts from R_kk = 0 and makes the test on its own rows; the merge levels fold nothing.  With
 * T level-0 triangles R is therefore the exact R factor of W + E with |E[:, k]|_2 <= sqrt(T) tol for such columns (the
 * folded parts lie in disjoint rows), E = 0 elsewhere: T = 1536 for the fused UR10 launch, 512 for the blocked kernel,
 * i.e. up to 0.35 - 0.6 tol_qr at tol = tol_qr / 64 -- reached only by a column whose residual really is that large in
 * every triangle, and even then |R_kk| itself is exact (the norm moves into R_kk, it is not dropped); what E perturbs is
 * the component of the LATER columns along that direction.  The linearly dependent columns of a regressor
 * (qrdecomposition.py:208-221: |R_kk| <= tol_qr, 27 % of the kept columns of UR10 and 29 % of TALOS) are null in every
 * tile -- their residual is rounding noise, 1e-13 .. 1e-12 -- and cost a norm instead of a column step.  tol = 0 (the
 * default): exact zeros only.  The pipeline and the qrdecomposition mirrors set tol_qr / 64 unless told otherwise
 * (null_pivots=False: plain Householder, the reference's arithmetic step for step).  Process-wide, takes effect at the
 * next launch. */
int figh_tsqr_null_pivot_tol(double tol);
/* PCI bus id ("0000:c1:00.0") of HIP device `device`: the physical device a rank drives, whatever logical index the
 * launcher's HIP_VISIBLE_DEVICES left it with (figaroh_plus_amd/dist.py: two ranks on one GPU cannot form an RCCL
 * communicator).  Creates no context.  No reference analogue. */
int figh_device_pci_bus_id(int device, char *out, int out_len);
int figh_device_info(char *name, int name_len, int *cu_count, size_t *hbm_bytes);
int figh_malloc(void **d_ptr, size_t bytes);
int figh_free(void *d_ptr);
/* Host <-> HBM copies on the library stream; both return when the data has arrived (h2d below 1 MB: when it is queued in
 * stream order).  This is where the reference's host-resident NumPy arrays cross the boundary: q, v, a in, and the stacked
 * regressor out when a caller keeps W = build_regressor_basic(...) as an ndarray (regressor.py:20-194: 4.03 GB for UR10 at 1e6
 * samples).  Transfers of 24 MB and more between PAGEABLE memory and HBM run in 32 MB chunks through two page-locked staging
 * buffers -- the DMA of chunk k + 1 beside the host copy of chunk k, shared by eight threads (which also take a fresh
 * destination's page faults in parallel): D2H 50 GB/s, H2D 27 - 55 GB/s on the GPU box (round 5, one hipMemcpyAsync per array:
 * 24 and 7.5).  A figh_host_alloc buffer is copied by plain DMA (57 GB/s).  Smaller transfers stage through one 1 MB buffer. */
int figh_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes);
int figh_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes);
/* Page-locked host memory for results that come back every pass (the (nc + 1) x nc rows of the rank step: 0.9 MB for
 * TALOS): figh_memcpy_d2h into such a buffer is one DMA, without the staging copy and without first-touch page faults of a
 * fresh NumPy array.  No reference analogue (the reference's arrays never leave the host). */
int figh_host_alloc(void **h_ptr, size_t bytes);
int figh_host_free(void *h_ptr);
int figh_memcpy_d2d(void *d_dst, const void *d_src, size_t bytes);
int figh_memset(void *d_dst, int value, size_t bytes);
int figh_synchronize(void);
/* per-kernel live timing with hipEvents on the library stream (bench.py roofline): enable, run, then query.
 * figh_profile_enable(level): 0 off; 1 times only the dominant kernels ("regressor_chain" / "regressor_tree" /
 * "tsqr": a few event records per pass, cheap enough to stay on inside a timed region); 2 times every launch.
 * figh_profile_get: name is the kernel family ("regressor_chain", "regressor_tree", "tsqr", "colsq", ...);
 * returns launches and total milliseconds since the last figh_profile_reset(). */
int figh_profile_enable(int level);
int figh_profile_reset(void);
int figh_profile_get(const char *name, int *launches, double *total_ms);

/* ------------------------------------------------------------------ model
 * Replaces what regressor.py reads from `robot.model` (regressor.py:36-42) and what
 * pin.computeJointTorqueRegressor reads from the Pinocchio Model (call sites regressor.py:49-51, :93-95).
 * Arrays have njoints entries, joint 0 = universe.  placement: 12 doubles per joint, row-major rotation (9)
 * then translation (3), child coords -> parent coords.  body_mask[j] != 0 iff inertias[j].mass != 0
 * (id_inertias, regressor.py:36-39).  The standard-parameter VALUES are not needed by the kernels. */
int figh_model_create(int njoints, const int32_t *parents, const int32_t *jtype, const double *axis,
                      const double *placement, const int32_t *idx_q, const int32_t *idx_v, const double *gravity,
                      const int32_t *body_mask, figh_model_t *out);
int figh_model_destroy(figh_model_t model);
/* ACTIVE JOINTS (examples/tiago/identification.py:148-187, :406-424: the script builds the regressor of all 24 dofs,
 * eliminates columns on the norms of the full matrix, and then decimates, stacks and factors only the row blocks of the
 * eight joints that carry measurements, act_idxv).  h_rows: the n dof indices whose row blocks figh_regressor_build_padded
 * STORES from now on (joint-torque mode of a tree of single-dof joints; link-padded or block-compact layout -- in the
 * block-compact one the other blocks take no memory at all, ld_j = 0); d_colsq keeps covering every row block, so
 * get_index_eliminate sees the reference's norms.  n <= 0 / NULL: every row block again (the default).  The chain kernel,
 * figh_regressor_build and the external-wrench mode ignore the setting. */
int figh_model_set_active_rows(figh_model_t model, const int32_t *h_rows, int n);
/* number of rows per sample and number of columns of the stacked regressor for (mode, flags) */
int figh_regressor_shape(figh_model_t model, int mode, int flags, int *rows_per_sample, int *ncols);

/* ------------------------------------------------------------------ K1: regressor assembly
 * Replaces build_regressor_basic (regressor.py:20-194) and, with FIGH_FLAG_TX40, add_coupling_TX40
 * (regressor.py:198-227): d_W[(j*N + i)*ldw + col] in the reference's joint-major row order and FIGAROH
 * column order (14 columns per link: Ixx Ixy Ixz Iyy Iyz Izz mx my mz m Ia fv fs off).
 * d_q: N x nq, d_v / d_a: N x nv, row-major.  ft_mask: bit c set <=> wrench component c (Fx Fy Fz Mx My Mz)
 * is named in param["force_torque"] ('All' = 63); ignored in joint-torque mode.
 * d_colsq (nullable): ncols doubles, receives diag(W^T W) of this call (the quantity of regressor.py:243,271). */
int figh_regressor_build(figh_model_t model, int mode, int flags, int ft_mask, int64_t N, const double *d_q,
                         const double *d_v, const double *d_a, double *d_W, int64_t ldw, double *d_colsq);

/* figh_regressor_build_padded: the same regressor for W that STAYS ON THE DEVICE (IdentificationPipeline, the streamed
 * entry points), tree models only.  Link-padded layout: 16 columns per link -- the 14 of the reference followed by two
 * zero columns -- so reference column 14 l + s is column 16 l + s; ldw must be a multiple of 16 (>= 16 (njoints-1)) and
 * d_W 128-byte aligned: every (row, link) segment is then exactly one cache line and the kernel writes whole lines
 * (4.4-5.0 TB/s against 2.3-2.6 TB/s for the 112-byte segments of the dense layout, rows of which are not line
 * aligned).  d_W may be NULL: column norms only.  d_colsq (nullable) is in the REFERENCE's column numbering
 * (14 (njoints-1) entries).  figh_tsqr / figh_matvec / figh_gather_cols take such a W through their column lists. */
int figh_regressor_build_padded(figh_model_t model, int mode, int flags, int ft_mask, int64_t N, const double *d_q,
                                const double *d_v, const double *d_a, double *d_W, int64_t ldw, double *d_colsq);
/* The link -> segment map of FIGH_FLAG_LINK_COMPACT for (model, mode, flags, ft_mask): h_link_pos[l] (njoints - 1 entries,
 * host) = position of link l + 1's segment, -1 for a link without one; *nlive = number of links with a segment.
 * FIGH_ERR_UNSUPPORTED when the layout does not apply (not an external-wrench regressor on a free-flyer root).  Which
 * links drop out follows from the model alone -- id_inertias of regressor.py:36-39 -- not from the samples. */
int figh_regressor_link_layout(figh_model_t model, int mode, int flags, int ft_mask, int32_t *h_link_pos, int *nlive);
/* Leading dimension of the force region of FIGH_FLAG_FORCE_COMPACT for (model, mode, flags, ft_mask): 16 * ceil(nlive / 4).
 * FIGH_ERR_UNSUPPORTED when the layout does not apply (see the flag). */
int figh_regressor_force_layout(figh_model_t model, int mode, int flags, int ft_mask, int64_t *ld_force);

/* figh_regressor_apply: d_tau_out = W(q, v, a) . phi WITHOUT W -- by definition np.dot(W, phi) for the W that
 * figh_regressor_build returns for the same (model, mode, flags, ft_mask, q, v, a), row j*N + i, rows_per_sample * N entries;
 * d_phi holds the ncols entries of figh_regressor_shape in the reference's column numbering.  Replaces the pin.rnea loops
 * and the friction / actuator-inertia / offset statements of get_torque_rand (src/figaroh/tools/randomdata.py:93-147), of
 * calc_torque (examples/tiago/utils/cubic_spline.py:448-455: the effort constraints of every trajectory that
 * examples/tiago/optimal_trajectory.py:154 and :288 evaluate) and tau_base = np.dot(W_b, phi_b) on a fresh trajectory
 * (examples/staubli_TX40/identification.py:244).  Recursive Newton-Euler with the link wrench in body-regressor form, O(links)
 * per sample: 192 B per UR10 sample instead of 2 x 4032 B through W.  The quirks of build_regressor_basic are part of the
 * definition: the FIGH_FLAG_TX40 coupling columns; np.sign(0) = 0; in external-wrench mode massless bodies and the rows
 * outside ft_mask carry no inertial term, and the Ia / fv / fs / off columns act on all six rows with v[i, k], a[i, k] of link
 * index k (regressor.py:142-169).  The entries of d_phi that belong to a flag that is off are not read.  No atomics: two calls
 * give the same bits.  FIGH_ERR_UNSUPPORTED (nothing launched, figh_last_error says why): external-wrench mode on a model
 * whose first joint is not a free-flyer; FIGH_FLAG_BLOCKED_INPUTS.  Without a HIP device: FIGH_ERR_NO_DEVICE, before any
 * argument is looked at. */
int figh_regressor_apply(figh_model_t model, int mode, int flags, int ft_mask, int64_t N, const double *d_q,
                         const double *d_v, const double *d_a, const double *d_phi, double *d_tau_out);

/* figh_repack_samples: d_dst[(t * width + k) * 64 + l] = d_src[min(64 t + l, N - 1) * width + k] -- a sample-major N x width
 * array (q, v or a exactly as the reference holds them) re-laid per tile of 64 samples, value-major inside the tile, the
 * last tile padded with its last sample.  d_dst: ceil(N / 64) * 64 * width doubles.  The copies are what
 * FIGH_FLAG_BLOCKED_INPUTS announces; a chunk of samples [lo, lo + n) with lo % 64 == 0 starts at d_dst + lo * width, like
 * in the original. */
int figh_repack_samples(const double *d_src, int64_t N, int width, double *d_dst);

/* add_coupling_TX40 as a separate call (regressor.py:198-227), for callers that append the three columns
 * [Iam6 fvm6 fsm6] to an existing W: d_out is (6N x 3) row-major, rows in the same joint-major order; only the
 * rows of joints 5 and 6 are non-zero: [a6 v6 sign(v5+v6)] and [a5 v5 sign(v5+v6)].  d_v, d_a: N x nv, nv >= 6. */
int figh_coupling_tx40(int64_t N, int nv, const double *d_v, const double *d_a, double *d_out);

/* ------------------------------------------------------------------ K2: column norms / gathers / residuals
 * figh_colsq: diag(W^T W) of a materialised matrix -- np.diag(np.dot(W.T, W)) at regressor.py:243 and :271. */
int figh_colsq(const double *d_W, int64_t rows, int cols, int64_t ldw, double *d_out);
/* figh_gather_cols: out[:, c] = W[:, col_idx[c]] -- np.delete(W, idx_e, 1) (regressor.py:254,292) and the
 * column copies of build_baseRegressor / get_baseParams (qrdecomposition.py:223-236, :299-313). */
int figh_gather_cols(const double *d_W, int64_t rows, int64_t ldw, const int32_t *d_col_idx, int n, double *d_out,
                     int64_t ldo);
/* figh_place_block: dst[r][c] = scale * src[r][c], a rows x cols block between two row-major device matrices (the
 * caller offsets the pointers) -- the np.concatenate / unary-minus / np.zeros statements that assemble W_tot in
 * build_total_regressor_current / _wrench (regressor.py:316-412, :446-490). */
int figh_place_block(const double *d_src, int64_t ld_src, int64_t rows, int64_t cols, double scale, double *d_dst,
                     int64_t ld_dst);
/* figh_matvec: y = W[:, col_idx] . x  (tau_base = np.dot(W_b, phi_b), e.g. staubli_TX40/identification.py:244) */
int figh_matvec(const double *d_W, int64_t rows, int64_t ldw, const int32_t *d_col_idx, int n, const double *d_x,
                double *d_y);
/* figh_block_sqnorm: out[b] = sum over the b-th block of `rows/nblocks` consecutive entries of (a - b)^2;
 * the per-joint residual norms of the WLS weights (identification_tools.py:312-315,
 * staubli_TX40/identification.py:310-313) and the residual of relative_stdev (identification_tools.py:222). */
int figh_block_sqnorm(const double *d_a, const double *d_b, int64_t rows, int nblocks, double *d_out);

/* ------------------------------------------------------------------ K3: tall-skinny Householder QR
 * Replaces the np.linalg.qr calls of qrdecomposition.py:105,205,238,286 for everything the reference uses
 * them for (|diag R| rank test, R1/R2 regrouping, Q1^T tau): Householder TSQR of the gathered columns
 * W[:, col_idx] (n of them), optionally with tau appended as one more column and with per-row-block weights
 * (row r is scaled by h_block_weight[r / (rows/nblocks)]; NULL = unweighted) -- the weighted LS of
 * staubli_TX40/identification.py:305-327 and identification_tools.py:317-325 is the QR of the scaled rows.
 * d_R_out: nc x nc row-major upper triangle, nc = n + (d_tau ? 1 : 0); with tau its last column holds
 * Q^T tau (first n entries) and the residual norm (entry nc-1).  R is defined up to row signs, like LAPACK's. */
int figh_tsqr(const double *d_W, int64_t rows, int64_t ldw, const int32_t *d_col_idx, int n, const double *d_tau,
              const double *h_block_weight, int nblocks, double *d_R_out);
/* figh_tsqr with a structure hint: the rows are nfirst consecutive blocks of rows/nfirst rows, and in block b the
 * gathered columns 0 .. h_first_col[b]-1 are EXACTLY zero (the caller's guarantee; 0 <= h_first_col[b] <= n).  That is
 * the shape of build_regressor_basic's W in joint-torque mode (regressor.py:45-87): row block j (the rows of joint j)
 * only involves the links of j's subtree, i.e. the columns from 14 j on.  The register-tile kernel (n <= 79) then does
 * not read those entries at all (41 % of the reads for UR10).  Same result as figh_tsqr. */
int figh_tsqr_structured(const double *d_W, int64_t rows, int64_t ldw, const int32_t *d_col_idx, int n,
                         const double *d_tau, const double *h_block_weight, int nblocks, const int32_t *h_first_col,
                         int nfirst, double *d_R_out);
/* Order-preserving row rejection (examples/staubli_TX40/identification.py:207-233, examples/tiago/identification.py:170-187:
 * samples whose joint velocity is below a threshold are removed from a joint's block of W and tau): the rows r of d_W
 * (rows x cols, leading dimension ldw) with |d_W[r, key_col]| >= threshold are copied, in order, to d_W_out (leading
 * dimension ld_out; room for `rows` rows) and, if given, d_tau[r] to d_tau_out; *h_count_out = the number of kept rows
 * (the call synchronises to return it). */
int figh_compact_rows(const double *d_W, int64_t rows, int cols, int64_t ldw, const double *d_tau, int key_col,
                      double threshold, double *d_W_out, int64_t ld_out, double *d_tau_out, int64_t *h_count_out);
/* The rank decision and the regrouped column order on the device (qrdecomposition.py:215-236): d_perm receives
 * [i : |R_ii| > tol_qr, ascending] followed by the remaining i < n, followed by n .. nc-1 (the tau column); the regrouped
 * factorisation qr([W1 W2 tau]) is then figh_tsqr(d_R, nc, nc, d_perm, nc, NULL, ...) with no host round trip. */
int figh_base_permutation(const double *d_R, int nc, int n, double tol_qr, int32_t *d_perm);
/* Sample-sharded reduction step: QR of `count` stacked nc x nc R factors (d_Rs: count*nc x nc) into one. */
int figh_tsqr_merge(const double *d_Rs, int count, int nc, double *d_R_out);

/* ---- the elimination and the base-parameter factorisation without a host round trip (IdentificationPipeline)
 * figh_select_columns: get_index_eliminate (regressor.py:258-279) on the device.  d_sel (2 + 2 ncols int32):
 * [0] the number of kept columns {c : not (colsq[c] < tol_e)}, [1] ncols, [2 .. 2+ncols) the kept columns in W's own
 * numbering (link_stride 14: the reference layout; 16: the link-padded layout, column 16 (c / 14) + c % 14), zeros behind
 * them, [2+ncols .. 2+2 ncols) the 0/1 mask in the reference's numbering. */
int figh_select_columns(const double *d_colsq, int ncols, double tol_e, int link_stride, int32_t *d_sel);
/* figh_tsqr_selected: figh_select_columns followed by the TSQR of W[:, kept] (+ tau), launched back to back: the column
 * list never visits the host.  The launch shape needs the column COUNT, which the caller supplies as n_expected (the
 * count of the previous pass; <= 0: selection only) and verifies afterwards against d_sel[0] -- on a mismatch the result
 * is to be discarded and the call repeated with the right count (entries of the list behind the device's count are 0,
 * so a stale count reads valid columns).  nblocks > 0: the structure hint of figh_tsqr_structured, derived from the list
 * on the device (row block b of rows/nblocks rows only involves the reference columns >= 14 b).
 * tol_qr < 0: d_R_out is the plain nc x nc triangle of figh_tsqr.
 * tol_qr >= 0: the rank decision and the regrouped factorisation of get_baseParams / double_QR
 * (qrdecomposition.py:205-244, :105-160) follow in the same launch as the last merge level.  d_R_out then is
 * (nc + 1) x nc: rows 0 .. nc-1 hold, in the ORIGINAL column order, row k = the row of qr([W1 W2 tau]) that belongs to
 * base column k (W1 = the columns with |R_kk| > tol_qr in the plain factorisation qr([W_e tau]), W2 the others), i.e.
 * R1 = out[base][:, base] (its upper triangle), R2 = out[base][:, rest], Q1^T tau = out[base][:, n]; the rows of
 * dependent columns are zero, and with exactly one extra column (tau) out[n][n] = || tau - W1 phi ||, the residual of the
 * least-squares problem in base coordinates.  Row nc is the diagonal of the plain factorisation: the numbers the rank
 * decision was taken on. */
int figh_tsqr_selected(const double *d_W, int64_t rows, int64_t ldw, const double *d_colsq, int ncols, double tol_e,
                       int link_stride, int nblocks, int n_expected, const double *d_tau, double tol_qr, int32_t *d_sel,
                       double *d_R_out);
/* figh_regressor_build (+ column norms) and the level-0 TSQR of W[:, d_kept] [+ tau] in ONE launch, for fixed-base serial
 * chains in joint-torque mode (UR10; regressor.py:20-194 with the pin.computeJointTorqueRegressor loop :45-87,
 * get_index_eliminate's norms :258-279, np.linalg.qr of get_baseParams qrdecomposition.py:205): W is written to HBM exactly
 * as figh_regressor_build writes it (ldw must equal the column count, d_W 16-byte aligned), d_colsq receives diag(W^T W),
 * and every 64-row tile is factored while it is still in the LDS of the CU that produced it -- the TSQR does not read W
 * back.  d_kept: the n kept columns (reference numbering, ascending) the caller expects -- those of the previous pass; the
 * caller verifies them afterwards against d_colsq (figh_select_columns) and repeats the pass through figh_regressor_build +
 * figh_tsqr_selected on a mismatch.  d_R_out as in figh_tsqr_selected (tol_qr < 0: the plain nc x nc triangle; tol_qr >= 0:
 * (nc + 1) x nc rows of the regrouped factorisation + the plain diagonal).  The tiles of a CU are handed to whichever
 * consumer wave is free, so R is reproduced up to rounding (not bit for bit) from run to run; W and d_colsq are
 * bit-reproducible.  FIGH_ERR_UNSUPPORTED (nothing launched): not a 6-joint chain, TX40 coupling columns, more than 64
 * columns with tau, fewer than 4096 samples, padded or unaligned W. */
int figh_regressor_tsqr_fused(figh_model_t model, int flags, int64_t N, const double *d_q, const double *d_v,
                              const double *d_a, double *d_W, int64_t ldw, double *d_colsq, const int32_t *d_kept, int n,
                              const double *d_tau, double tol_qr, double *d_R_out);
/* ---- the host tail of a pass on the numbers the device returns (get_baseParams, qrdecomposition.py:215-244, for at most
 * 80 kept columns), HOST ONLY: no device is needed, opened or touched.
 * In: rows_k = the (nc + 1) x nc output of figh_tsqr_selected / figh_regressor_tsqr_fused with tol_qr >= 0 (layout
 * above; nc = n + with_tau), tol_qr, total_rows and pieces (the rows of the factored matrix and its separately launched
 * parts: the certificate's margin grows with sqrt(T), T <= total_rows / 32 + pieces level-0 triangles), null_rule != 0:
 * the pass ran under figh_tsqr_null_pivot_tol(tol_qr) and is to be certified.
 * Out: idx = the base columns {k < n : |diag_k| > tol_qr} ascending (n_base of them; a NaN pivot is not base) followed
 * by the others ascending; absdiag (n) = |diag|; beta (n_base x (n - n_base), packed) = R1^-1 R2 rounded to six
 * decimals as np.around rounds (round-half-even of x 1e6, divided back); with_tau: phi_ls = R1^-1 Q1^T tau, phi_b = phi_ls
 * rounded likewise, residual_norm = |rows_k[n][n]|.  R1^-1 comes from back substitution on the UPPER triangle of
 * rows_k[base][:, base] (below it the device leaves rounding residues).  status = FIGH_TAIL_SINGULAR when R1 has an exactly
 * zero pivot (beta, phi_* are then not written; np.linalg.inv of the reference raises LinAlgError).
 * Certificate (null_rule): certified = 1 when the classification is provably plain Householder's -- every base pivot
 * further above tol_qr than 2 (1 + A_base[k]) sqrt(T) tol_qr / 64, every other pivot finite, at most tol_qr / 8 and
 * further below tol_qr than 2 (1 + A_dep[c]) tol_qr / 64, and (with_tau) |R1^-1|_inf (tol_qr / 64) |phi|_1 <=
 * 1e-7 max(1, |phi|_inf).  bounds (n + 2 doubles, in / out) = [A_base (n_base) | A_dep (n - n_base) | |R1^-1|_inf | valid]:
 * A_base[k] = |R1_kk| sum_{i<k} |(R1^-1)_ik|, A_dep[c] = sum_i |(R1^-1 R2)_ic|; valid = 0 when R1 is singular or its inverse
 * not finite (never certified).  They are properties of the model far more than of the samples: when the caller hands
 * back the base columns they were computed for (cached_base, n_cached_base; -1: none) and those are this pass's, bounds is
 * used as it is; otherwise it is recomputed and bounds_recomputed = 1. */
enum { FIGH_TAIL_OK = 0, FIGH_TAIL_SINGULAR = 1 };
typedef struct figh_host_tail_s {
    const double *rows_k;        /* in (figh_chain_pass_fused: set by the entry to the staged rows) */
    int32_t n, with_tau;         /* in */
    double tol_qr;               /* in */
    int64_t total_rows, pieces;  /* in */
    int32_t null_rule;           /* in */
    int32_t n_cached_base;       /* in */
    const int32_t *cached_base;  /* in */
    double *bounds;              /* in / out: n + 2 */
    int32_t *idx;                /* out: n */
    double *absdiag;             /* out: n */
    double *beta;                /* out: up to n * n / 4 */
    double *phi_ls, *phi_b;      /* out: n_base each (with_tau) */
    double residual_norm;        /* out */
    int32_t n_base, status, certified, bounds_recomputed; /* out */
} figh_host_tail_t;
int figh_chain_host_tail(figh_host_tail_t *tail);
/* One call for a whole fused pass of a single rank: figh_regressor_tsqr_fused (same arguments, same launches, tol_qr >= 0),
 * figh_select_columns(d_colsq, 14 nlinks, tol_e, 14, d_sel), the pack on the host, the wait, the check of the selection and
 * figh_chain_host_tail on the staged rows.  Two launches: the merge launch sums the norms and selects the columns beside
 * its tree (figh_tsqr_merge_base_norms).  The pack = [colsq (ncols f64) | sel (2 + 2 ncols i32, padded to 8 bytes) | rows
 * ((nc + 1) nc f64)], ncols = 14 nlinks: d_colsq, d_sel and d_R_out of the separate entries are its three parts.  h_pack
 * (pack_bytes) receives it: page-locked memory (figh_host_alloc) is stored to directly by the kernels -- no copy, d_pack is
 * left as it is --, any other memory through d_pack and one copy.  h_kept_mask (ncols bytes): the 0 / 1 mask of
 * d_kept.  *changed = 1 when the device's selection is another one: the pass is to be discarded and repeated through
 * figh_regressor_build + figh_tsqr_selected, tail is not touched.  col_norm and sel are bit for bit those of the separate
 * entries (same kernels, same order of the sums).  FIGH_ERR_UNSUPPORTED as for figh_regressor_tsqr_fused. */
int figh_chain_pass_fused(figh_model_t model, int flags, int64_t N, const double *d_q, const double *d_v, const double *d_a,
                          double *d_W, int64_t ldw, const int32_t *d_kept, int n, const double *d_tau, double tol_qr,
                          double tol_e, double *d_pack, double *h_pack, size_t pack_bytes, const uint8_t *h_kept_mask,
                          int *changed, figh_host_tail_t *tail);
/* figh_tsqr_selected for the external-wrench regressor of a model with a free-flyer root (regressor.py:89-192: six row
 * blocks of rows / 6 rows, force components first): in the force rows the six rotational-inertia columns of every link
 * are exact zeros, so those rows are factored over the nf_expected kept columns with slot >= 6 only (2 m nf^2 instead of
 * 2 m n^2 flops for half of W), and the torque rows by a launch whose first workgroup starts from the force rows'
 * triangle.  Same outputs as figh_tsqr_selected (R is the R factor of the whole W[:, kept | tau]); nf_expected is the
 * number of kept columns c with c % 14 >= 6 -- the caller derives it from the same mask as n_expected and verifies both
 * afterwards.  nf_expected <= 0, at most 80 columns or rows % 6 != 0: plain figh_tsqr_selected.  d_link_pos (nullable,
 * device, njoints - 1 int32): d_W is link-compact (FIGH_FLAG_LINK_COMPACT), reference column 14 l + s is column
 * 16 d_link_pos[l] + s.  ld_force > 0: d_W is force-compact (FIGH_FLAG_FORCE_COMPACT) -- rows / 2 force rows of ld_force columns
 * at d_W, the torque rows of ldw columns behind them; needs the split (nf_expected > 0, more than 80 columns). */
int figh_tsqr_selected_wrench(const double *d_W, int64_t rows, int64_t ldw, const double *d_colsq, int ncols, double tol_e,
                              int link_stride, int n_expected, int nf_expected, const double *d_tau, double tol_qr,
                              int32_t *d_sel, double *d_R_out, const int32_t *d_link_pos, int64_t ld_force);
/* figh_tsqr_selected for the joint-torque regressor of a tree of single-dof joints (regressor.py:45-87, rows j*N + i): row
 * block j only involves the links of joint j's subtree and the Ia / fv / fs / off columns of link j itself; all other
 * entries are structural zeros.  Row block j (rows / nblocks rows) is factored over its own column list -- h_counts[j]
 * entries of d_cols (device column numbering) and d_pos (positions in the kept list), concatenated block after block,
 * built by the caller from the kept mask it expects (and verified against d_sel afterwards) -- reduced, embedded into the
 * kept column set, and the nblocks triangles are merged.  Same outputs as figh_tsqr_selected.  h_block_off / h_block_ld
 * (host, nblocks entries each, both or neither): the block-compact W of FIGH_FLAG_COMPACT_BLOCKS -- row block j is the
 * rows / nblocks x h_block_ld[j] matrix at d_W + h_block_off[j] and d_cols index ITS columns; ldw is then unused.
 * The nblocks embedded triangles are stacked compactly -- block j contributes its h_counts[j] (+ 1 with tau) rows over the
 * nc kept columns [+ tau] -- and factored as one small tall matrix.  d_block_tri (nullable; room for
 * (sum_j (h_counts[j] + 1) + nc + 1) nc doubles) receives that stack, for a weighted solve afterwards
 * (figh_block_rows_residuals, then figh_tsqr over its rows with one weight per row: W itself is not read again).
 * h_counts[j] == -1: row block j is INACTIVE -- neither its rows of W nor its rows of tau take part (the joints without
 * measurements of examples/tiago/identification.py:148-187; figh_model_set_active_rows keeps them out of W as well); it has
 * no entries in d_cols / d_pos and no rows in the stack. */
int figh_tsqr_selected_blocks(const double *d_W, int64_t rows, int64_t ldw, const double *d_colsq, int ncols, double tol_e,
                              int link_stride, int n_expected, int nblocks, const int32_t *h_counts, const int32_t *d_cols,
                              const int32_t *d_pos, const int64_t *h_block_off, const int32_t *h_block_ld,
                              const double *d_tau, double tol_qr, int32_t *d_sel, double *d_R_out, double *d_block_tri);
/* Per-row-block residual norms from the compact stack figh_tsqr_selected_blocks leaves in d_block_tri: block b occupies the
 * rows [h_row_off[b], h_row_off[b+1]) (h_row_off[b] = sum over the blocks in front of b of their column count + 1 for tau;
 * nblocks + 1 entries), every row over the nc = n + 1 kept columns [+ tau].  With v = [phi over the kept columns; -1],
 * d_r2[b] = sum of (row . v)^2 = || tau_b - W_b phi ||^2 -- the per-joint variances of the weighted least squares
 * (examples/staubli_TX40/identification.py:305-316, identification_tools.py:291-331) without another pass over W. */
int figh_block_rows_residuals(const double *d_rows, int nblocks, const int32_t *h_row_off, int nc, const double *d_v,
                              double *d_r2);
/* figh_tsqr_merge followed by the rank decision and the regrouped factorisation as in figh_tsqr_selected (the cross-rank
 * reduction of the all-gathered per-rank triangles): columns k < n_free take part in the rank decision, the others (tau)
 * always count as base columns.  d_rows_out: (nc + 1) x nc. */
int figh_tsqr_merge_base(const double *d_Rs, int count, int nc, int n_free, double tol_qr, double *d_rows_out);
/* figh_tsqr_merge_base with the tail of a fused pass: d_part (nblocks x ncols partial sums of diag(W^T W), one row per
 * producer) is summed over the blocks into d_colsq (ncols) in the library's fixed order, and d_sel (2 + 2 ncols int32) is
 * figh_select_columns(d_colsq, ncols, tol_e, 14, d_sel).  With more than one triangle, at most 80 columns, ncols <= 128
 * and a merge tree that is resident in one launch with a workgroup to spare, that launch does all three, the sums and the
 * selection beside the tree; otherwise they are three steps.  d_colsq, d_sel and d_rows_out are bit for bit the same
 * either way (one copy of the code, the same order of the sums). */
int figh_tsqr_merge_base_norms(const double *d_Rs, int count, int nc, int n_free, double tol_qr, const double *d_part,
                               int nblocks, int ncols, double tol_e, double *d_colsq, int32_t *d_sel, double *d_rows_out);

/* ------------------------------------------------------------------ streamed entry points (W never stored in full)
 * The "fused" forms of SURVEY.md section 8b: the samples are processed in chunks of `chunk_samples` (0 = library
 * default, about 2 GB of W); each chunk's W lives in a library workspace only until the next kernel has consumed it.
 * Same mode / flags / ft_mask / q, v, a conventions as figh_regressor_build.  d_tau keeps the reference's layout
 * (rows_per_sample * N entries, row j*N + i).
 *
 * figh_regressor_colsq: diag(W^T W) of the W that build_regressor_basic would return (regressor.py:243,271). */
int figh_regressor_colsq(figh_model_t model, int mode, int flags, int ft_mask, int64_t N, const double *d_q,
                         const double *d_v, const double *d_a, int64_t chunk_samples, double *d_colsq);
/* figh_regressor_tsqr: the R factor that figh_tsqr would return for that W (columns d_col_idx, optional tau column and
 * per-row-block weights; nblocks must divide rows_per_sample, e.g. one weight per joint) -- qrdecomposition.py:105,
 * 205,238,286 on top of regressor.py:20-227 without the 6N x ncols intermediate. */
int figh_regressor_tsqr(figh_model_t model, int mode, int flags, int ft_mask, int64_t N, const double *d_q,
                        const double *d_v, const double *d_a, const int32_t *d_col_idx, int n, const double *d_tau,
                        const double *h_block_weight, int nblocks, int64_t chunk_samples, double *d_R_out);
/* figh_regressor_tsqr_norms: figh_regressor_tsqr that also returns diag(W^T W) of ALL columns (d_colsq_out, ncols doubles,
 * the reference's numbering) from the same pass -- the norms are fused into the regressor kernel of every chunk.  For a
 * caller that factors the columns it expects get_index_eliminate (regressor.py:258-279) to keep, e.g. the set of the
 * previous pass, and verifies the set afterwards: one pass over the samples instead of two. */
int figh_regressor_tsqr_norms(figh_model_t model, int mode, int flags, int ft_mask, int64_t N, const double *d_q,
                              const double *d_v, const double *d_a, const int32_t *d_col_idx, int n, const double *d_tau,
                              const double *h_block_weight, int nblocks, int64_t chunk_samples, double *d_R_out,
                              double *d_colsq_out);
/* figh_regressor_tsqr_batch: B independent trajectories of n_per samples each (d_q, d_v, d_a hold the B * n_per samples
 * back to back) -> B triangles, d_R_out[b] = the n x n R factor of W[:, d_col_idx] of trajectory b.  With d_R_stack (one
 * n x n triangle, nullable) every result is the R factor of vstack((W_stack, W_b)) instead, R_stack being the triangle
 * of W_stack.  This is one finite-difference gradient of the excitation objective, np.linalg.cond(W_b) per perturbed
 * trajectory (examples/tiago/optimal_trajectory.py:100-133, 296-313), in one K1 launch + one batched TSQR launch + the
 * pair-merge levels for more than 80 columns (trajectory by trajectory through figh_regressor_tsqr otherwise). */
int figh_regressor_tsqr_batch(figh_model_t model, int mode, int flags, int ft_mask, int64_t B, int64_t n_per,
                              const double *d_q, const double *d_v, const double *d_a, const int32_t *d_col_idx, int n,
                              const double *d_R_stack, double *d_R_out);
/* figh_regressor_tsqr_batch_fused: figh_regressor_tsqr_batch (same inputs, same B plain n x n triangles with zeros below the
 * diagonal, d_R_stack folded in when given) for fixed-base serial chains in joint-torque mode, in ONE launch that never
 * writes W: workgroup (slice s, trajectory b) builds the regressor rows of its 64-sample tiles of trajectory b in LDS
 * (build_regressor_basic, regressor.py:20-194, the pin.computeJointTorqueRegressor loop :45-87) and factors the columns
 * d_col_idx (build_regressor_reduced + build_baseRegressor) there -- the np.linalg.cond(W_b) of objective_func
 * (examples/tiago/optimal_trajectory.py:100-133) needs only the triangle of W_b -- then one launch per merge level (at most
 * three, one when a trajectory is one workgroup) turns every trajectory's triangles + d_R_stack (np.vstack((W_stack, W_b)))
 * into d_R_out[b].  The launch count does not depend on B; the slices per trajectory are chosen so that B * S workgroups
 * fill the chip.  d_col_idx is required.  Tiles go to whichever consumer wave is free: the triangles are reproduced up to
 * rounding from run to run.  FIGH_ERR_UNSUPPORTED (nothing launched, figh_last_error says which): not a serial chain of
 * 5 to 7 joints; FIGH_FLAG_TX40, FIGH_FLAG_GENERIC or FIGH_FLAG_BLOCKED_INPUTS; n > 64, or n = 64 with 7 joints (LDS: two
 * tile buffers leave room for fewer than three consumer triangles); n_per < 64 (one full sample tile:
 * 64 samples are more rows than the nc + 8 from which level 0 applies the null-pivot rule); B > 65535. */
int figh_regressor_tsqr_batch_fused(figh_model_t model, int flags, int64_t B, int64_t n_per, const double *d_q,
                                    const double *d_v, const double *d_a, const int32_t *d_col_idx, int n,
                                    const double *d_R_stack, double *d_R_out);
/* figh_regressor_gram: h_G = W_e^T W_e (n x n, row-major, host), h_g = W_e^T tau (n), *h_tau_sq = tau^T tau, formed
 * from the Householder R (G = R1^T R1): the normal-equation quantities of the SIP QP (identification_tools.py:528-531)
 * and of the weighted LS statements (staubli_TX40/identification.py:320-327).  h_g / h_tau_sq may be NULL iff d_tau
 * is NULL. */
int figh_regressor_gram(figh_model_t model, int mode, int flags, int ft_mask, int64_t N, const double *d_q,
                        const double *d_v, const double *d_a, const int32_t *d_col_idx, int n, const double *d_tau,
                        int64_t chunk_samples, double *h_G, double *h_g, double *h_tau_sq);

/* ------------------------------------------------------------------ zero-phase filtering / decimation
 * The step on either side of the hot path on real data: scipy.signal.decimate(x, q, zero_phase=True) over every
 * column of W_b and over tau, joint block by joint block (examples/staubli_TX40/identification.py:186-204,
 * examples/tiago/identification.py:142-187), and signal.filtfilt of the joint positions (identification_tools.py:
 * 390-424).  d_X is rows x cols (ldx), made of nblocks row blocks of rows/nblocks samples; every (block, column)
 * sequence is filtered forward and backward with odd padding of `padlen` samples (SciPy's method='pad') and every
 * q-th sample is kept: d_Y receives nblocks blocks of ceil(L/q) rows (*rows_out in total).
 * form 0: second-order sections -- h_b / h_a are nsec x 3 (sos[:, :3] and sos[:, 3:]), order = 2, h_zi = sosfilt_zi
 * (nsec x 2).  form 1: transfer function -- nsec = 1, h_b / h_a have order + 1 entries (a[0] = 1), h_zi = lfilter_zi.
 * The recurrences follow SciPy's loops operation by operation (no FMA contraction). */
int figh_filtfilt_cols(const double *d_X, int64_t rows, int cols, int64_t ldx, int nblocks, int form, const double *h_b,
                       const double *h_a, int nsec, int order, const double *h_zi, int padlen, int q, double *d_Y,
                       int64_t ldy, int64_t *rows_out);

/* ------------------------------------------------------------------ median filter and finite differences
 * The device front end of the real-data chain: raw joint positions go in once, (q, dq, ddq) come out resident in the
 * layouts K1 reads.  All three entries are parallel in time; the translation unit is compiled without FMA contraction.
 *
 * figh_medfilt_cols: scipy.signal.medfilt(x, kernel_size) of every (row block, column) sequence of d_X (rows x cols, ldx;
 * nblocks row blocks of rows / nblocks samples) -- the first statement of the TIAGo script's apply_filters
 * (examples/tiago/identification.py:63-90).  Zero padding at both ends OF EACH BLOCK, the median is an element of the
 * window: equal to SciPy on data without NaN (np.array_equal; where the window holds zeros of both signs the median may
 * be the other signed zero than SciPy's sort picks).  kernel_size: odd, 1 .. 63 (1 - 9 sort the window in registers, larger
 * ones in a run-time loop); an even size, a size outside [1, 63], a leading dimension below cols or rows % nblocks != 0:
 * FIGH_ERR_INVALID, nothing launched. */
int figh_medfilt_cols(const double *d_X, int64_t rows, int cols, int64_t ldx, int nblocks, int kernel_size, double *d_Y,
                      int64_t ldy);
/* figh_joint_difference: d_dq[i, :] = pin.difference(model, q[i], q[i + 1]) / (d_dt ? d_dt[i] : ts), i = 0 .. N - 2 -- the
 * loop of calculate_first_second_order_differentiation (identification_tools.py:366-376; call sites
 * examples/ur10/identification.py:122, examples/staubli_TX40/identification.py:145, examples/human/identification.py:424).
 * d_q: N x nq row-major, d_dq: (N - 1) x nv row-major, d_dt: NULL or N - 1 doubles.  Revolute / prismatic: q1 - q0
 * (bit-equal to np.diff(q) / ts); continuous (cos, sin): atan2(s1 c0 - c1 s0, c1 c0 + s1 s0); free-flyer (p, quaternion
 * xyzw): log6(R0^T R1, R0^T (p1 - p0)), (linear, angular), with the branches theta < 1e-8, pi - theta < 1e-6 (log3) and
 * t < 1e-4 (log6) and the operation order of the package's host mirror, so that the device differs from it only through
 * acos, atan2, sin, cos, sqrt.  Tiles of 64 k sample pairs (k = the largest of 1 .. 4 for which (64 k + 1) rows of q and
 * 64 k rows of dq, row strides padded to odd, fit 64 KB of LDS) are staged in LDS; a chain model never runs the per-pair
 * pass.  Row N of d_q is never read.  N >= 2. */
int figh_joint_difference(figh_model_t model, int64_t N, const double *d_q, double ts, const double *d_dt, double *d_dq);
/* figh_gradient_cols: d_G[:, c] = np.gradient(d_F[:, c], edge_order=1) / (d_h ? d_h[row] : h) for c < ncols_active
 * (identification_tools.py:378-384; np.gradient(dq) / np.gradient(t) of examples/tiago/identification.py:92-99 with
 * d_h = np.gradient(t)): (F[i+1] - F[i-1]) / 2.0 inside, F[1] - F[0] and F[n-1] - F[n-2] at the ends, then one division --
 * bit-equal to NumPy.  Columns c >= ncols_active of d_G are written as +0.0 (the reference's range(model.nq - 1): the last
 * joint of a fixed-base robot keeps a zero acceleration).  rows >= 2 (np.gradient raises below that), d_h: NULL or rows
 * doubles. */
int figh_gradient_cols(const double *d_F, int64_t rows, int cols, int64_t ld, int ncols_active, double h, const double *d_h,
                       double *d_G, int64_t ldg);

/* ------------------------------------------------------------------ free-flyer real data: orientation filter, wrench transport
 * The three per-sample Python loops of examples/human/identification.py around the filters and the regressor.  One lane per
 * sample, fp64, no atomics (two calls give the same bits), compiled without FMA contraction; the operation order is fixed in
 * the header comment of csrc/figh_freeflyer.hip and repeated element by element by the NumPy mirrors
 * (identification/identification_tools.py).  Nothing outside [rows, cols) of a padded buffer is written.  Quaternions are
 * (x y z w), 6-vectors (linear, angular).  All three: N < 1, a leading dimension below the width, a joint id outside the
 * model, an unknown layout, a NULL pointer or an output that overlaps an input (but see d_out == d_ref below) return
 * FIGH_ERR_INVALID before anything is launched, figh_last_error says why.
 *
 * figh_quat_log: d_rotvec[i, 0:3] = pin.log3(pin.Quaternion(q[i, 3:7])) (examples/human/identification.py:330-339).  d_quat
 * points at the x of row 0 (q + idx_q + 3 with ld_quat = nq).  The principal rotation vector from the quaternion, not through
 * a matrix: n = sqrt(x^2 + y^2 + z^2), theta = 2 atan2(n, |w|), r = sgn(w) (theta / n) (x, y, z) with sgn(0) = +1; q and -q
 * give the same vector; the quaternion is not renormalised (atan2 does not need it).  For n < 2^-13 |w| the series
 * theta / n = 2 (1 - t^2 / 3 + t^4 / 5) / |w|, t = n / |w|; n = 0 gives three +0.0.  The same function as Pinocchio's, not the
 * same bits.  Where w changes sign at theta = pi the vector jumps, as the reference's does: it filters the raw vector, and
 * nothing here unwraps it. */
int figh_quat_log(const double *d_quat, int64_t N, int64_t ld_quat, double *d_rotvec, int64_t ld_rotvec);
/* figh_rotvec_to_quat: d_out[i, 0:4] = +-pin.Quaternion(pin.exp3(r_i)) with the sign chosen against d_ref[i, 0:4], the raw
 * quaternion of the same row (examples/human/identification.py:349-364).  With theta = |r| the canonical quaternion is
 * q^ = (sin(theta / 2) / theta r, cos(theta / 2)); for theta < 2^-13 the series sin(theta / 2) / theta = 1/2 - theta^2 / 48 +
 * theta^4 / 3840 and cos(theta / 2) = 1 - theta^2 / 8 + theta^4 / 384.  (1) Eigen's representative sE q^ is what its
 * matrix-to-quaternion conversion returns for exp3(r): |w^| > 1/2: w > 0; otherwise the vector component of largest
 * magnitude is positive, the first of equal ones (Eigen's comparisons are strict).  (2) The reference's test: with
 * d = (sE q^) . ref it keeps the representative when 2 acos(d) < pi / 2 -- here: keep iff d > 0.7071067811865476 -- and negates
 * it otherwise.  (3) THE ONE DELIBERATE DIFFERENCE: when rounding makes d > 1 the reference's acos is NaN and it negates; here
 * that case keeps.  Rounding noise decides it, so it cannot be mirrored across math libraries, and -q is the same rotation:
 * the physical result is unchanged.  d_out may be d_ref itself (same pointer, same leading dimension): a lane reads its row
 * before it writes it.  Any other overlap is refused. */
int figh_rotvec_to_quat(const double *d_rotvec, int64_t N, int64_t ld_rotvec, const double *d_ref, int64_t ld_ref,
                        double *d_out, int64_t ld_out);
/* figh_wrench_transport: a wrench per sample carried through (R, p) = oMi[joint](q_i), the placement of any joint of the
 * model.  inverse = 0, pin.Force.se3Action (world <- joint, examples/human/identification.py:471-555): f' = R f,
 * n' = R n + p x f'.  inverse = 1, se3ActionInverse (joint <- world, :434-453): f' = R^T f, n' = R^T (n - p x f).  d_q: N x nq
 * sample-major, leading dimension ldq.  Each layout is FIGH_WRENCH_SAMPLE (N x 6, leading dimension 6) or
 * FIGH_WRENCH_STACKED (component k of sample i at [k N + i]: the order of tau and of figh_regressor_apply).  The support path
 * of the joint travels by value in the kernel arguments and is walked root first, (R, p) <- (R, p) . placement_j . M_j(q_j)
 * with the joint model of the regressor kernels (csrc/figh_spatial.h); only the q of the joints on the path is read (the root
 * free-flyer of the human model: 7 of the 46 doubles of a row).  joint = 0 is the universe (identity).  Both layouts are read
 * and written with consecutive lanes on consecutive addresses.  FIGH_ERR_UNSUPPORTED (nothing launched): a support path
 * longer than the kernel arguments hold. */
enum { FIGH_WRENCH_SAMPLE = 0, FIGH_WRENCH_STACKED = 1 };
int figh_wrench_transport(figh_model_t model, int joint, int64_t N, const double *d_q, int64_t ldq, const double *d_F,
                          int layout_in, int inverse, double *d_out, int layout_out);

/* ------------------------------------------------------------------ excitation trajectories
 * The front and the back of the excitation loop: waypoints in, resident (q, v, a) out, constraint vectors out; in between
 * figh_regressor_tsqr_batch[_fused] and figh_regressor_apply read the same buffers, so no sample array crosses the bus.
 * The translation unit is compiled without FMA contraction; its header states the operation order.
 *
 * figh_spline_sample: CubicSpline.get_full_config (examples/tiago/utils/cubic_spline.py:82-181) with velocity and
 * acceleration waypoints, for B waypoint sets at once: between neighbouring waypoints the unique quintic through position,
 * velocity and acceleration at both ends (what ndcurves.exact_cubic builds from two waypoints and
 * init_vel / end_vel / init_acc / end_acc, :110-122 -- the same polynomial, not the same bits), sampled at
 * t_i = h_tps[0] + i * delta_t, delta_t = 1 / freq, i < n_per (:133-153; the reference's N is
 * int((tps[-1] - tps[0]) / delta_t) + 1, a division by the rounded delta_t), and scattered
 * into full configurations (:171-178): trajectory b fills rows [b n_per, (b + 1) n_per) of d_q (B n_per x nq, ldq), d_v and
 * d_a (B n_per x nv, ldv) -- the layout figh_regressor_tsqr_batch[_fused] and figh_regressor_apply read.  h_act_idxq /
 * h_act_idxv: the n_act active joints' idx_q / idx_v.  h_tps: n_wps >= 2 strictly increasing time points shared by the batch.
 * d_wps: B x n_act x n_wps (the reference's (n_act, n_wps) array per trajectory); d_vel_wps / d_acc_wps: the same layout,
 * trajectory b at offset b * vel_stride / b * acc_stride (0: one set for all trajectories).  d_q0: nq doubles, robot.q0, the
 * fill of the position columns no active joint owns; such columns of d_v / d_a are written as +0.0.  Nothing is written
 * outside the B n_per x width part of a padded buffer.  The segment of t_i is the largest k with h_tps[k] <= t_i, at most
 * n_wps - 2, and the local time is min(t_i - h_tps[k], h_tps[k+1] - h_tps[k]): where rounding puts the last sample behind
 * h_tps[n_wps - 1] ndcurves raises, this entry evaluates the end of the last segment.  Two launches whatever B is (segment
 * coefficients into a workspace table, then one thread per output element); bit-equal to the package's NumPy mirror.
 * FIGH_ERR_INVALID: time points not strictly increasing, a stride between 1 and n_act n_wps - 1, n_per max(nq, nv) >= 2^31
 * (a trajectory is indexed in 32 bits; B is not limited), an index pair that is no
 * joint.  FIGH_ERR_UNSUPPORTED (nothing launched, figh_last_error says why): an active joint that is not one revolute or
 * prismatic degree of freedom; inactive joints may be anything.  Without a HIP device: FIGH_ERR_NO_DEVICE, before any
 * argument is looked at. */
int figh_spline_sample(figh_model_t model, int64_t B, int n_wps, int n_act, int64_t n_per, double freq,
                       const int32_t *h_act_idxq, const int32_t *h_act_idxv, const double *h_tps, const double *d_wps,
                       const double *d_vel_wps, int64_t vel_stride, const double *d_acc_wps, int64_t acc_stride,
                       const double *d_q0, double *d_q, int64_t ldq, double *d_v, double *d_a, int64_t ldv);
/* figh_excitation_constraints: the constraint vector of get_constraints_all_samples
 * (examples/tiago/optimal_trajectory.py:156-174, :185-187) without the collision distances, for B trajectories: row b of d_out
 * (B x n_con, ld_out; n_con = n_idx n_act + 2 n_per n_act) is np.concatenate((q_wp, v_act, tau_act), axis=None) with
 * q_wp = p_f[idx_waypoints][:, act_idxq] (n_idx x n_act), v_act = v_f[:, act_idxv] (n_per x n_act) and tau_act[i, k] =
 * tau[act_idxv[k] * n_per + i].  d_q / d_v: the batched samples as figh_spline_sample leaves them; d_tau: the batched layout
 * of figh_regressor_apply over all B n_per samples (row j B n_per + b n_per + i).  h_idx_waypoints: n_idx sample indices in
 * [0, n_per), found by the host (the reference compares t_f[i] with tps[1:] for exact equality).  Pure copies; n_con < 2^31.
 * The active
 * joints are checked as in figh_spline_sample; without a HIP device: FIGH_ERR_NO_DEVICE, before any argument is looked at. */
int figh_excitation_constraints(figh_model_t model, int64_t B, int64_t n_per, int n_act, const int32_t *h_act_idxq,
                                const int32_t *h_act_idxv, int n_idx, const int32_t *h_idx_waypoints, const double *d_q,
                                int64_t ldq, const double *d_v, int64_t ldv, const double *d_tau, double *d_out,
                                int64_t ld_out);

/* figh_collision_distances: the fourth part of that constraint vector, the self-collision distances of the simplified
 * collision model (examples/tiago/optimal_trajectory.py:176-186: CollisionWrapper.computeCollisions + getDistances,
 * src/figaroh/tools/robotcollisions.py:62-72, :108-113, over the objects and pairs of
 * examples/tiago/utils/simplified_colission_model.py:55-180), for samples of B trajectories of n_per configurations
 * (d_q: B n_per x nq, leading dimension ldq).  h_idx: n_idx sample indices in [0, n_per) at which to evaluate; NULL: every
 * sample (n_idx is ignored and counts as n_per below).
 * The geometry table, launch-uniform HOST arrays over n_geom <= FIGH_COLLISION_MAX_GEOMETRIES objects: h_kind (FIGH_GEOM_*),
 * h_parent (the joint the object is fixed to, 0: the universe), h_placement (12 doubles each: R row-major, then p, object to
 * joint coordinates) and h_dims (3 doubles each, as hpp-fcl's constructors take them: box x y z full sides; cylinder radius,
 * full length along z; sphere radius; capsule radius, full length of its axis segment; unused entries 0).  h_pairs: n_pairs
 * <= FIGH_COLLISION_MAX_PAIRS pairs (first, second) of object ids.  The caps are what the kernel-argument block holds.
 * Convention: a shape is a convex core and a radius r (box, cylinder: their own core, r = 0; sphere: its centre; capsule: its
 * axis segment) and d = dist(core_A, core_B) - r_A - r_B -- the Euclidean distance of separated shapes (hpp-fcl's
 * min_distance), minus the penetration depth of rounded shapes in shallow overlap, and exactly -(r_A + r_B) with status
 * FIGH_COLLISION_CORES_INTERSECT when the cores intersect (hpp-fcl runs EPA there; not mirrored).  GJK in fp64 on the world
 * placements oM_parent . placement, one query per lane (csrc/figh_collision.hip, tools/robotcollisions.py): a query stops
 * with FIGH_COLLISION_OK when |v| - v.w / |v| <= tol (v the closest point of the simplex, w the new support point of
 * core_A - core_B: v.w / |v| <= dist <= |v|), and after max_iter support evaluations with FIGH_COLLISION_ITERATION_CAP,
 * when |v| is still an upper bound.
 * d_out[b ld_b + i n_pairs + p]: the distance of pair p at sample i of trajectory b -- two strides, so that the distances
 * can land behind the other three parts of a constraint row (d_out: the address of that tail, ld_b: the row stride);
 * nothing else of the buffer is written.  d_witness (6 doubles per query (b n_idx + i) n_pairs + p: the witness points on
 * core A and core B, world frame) and d_status (int32 per query: the status, the number of support evaluations in the
 * upper half) may each be NULL.  Plain stores, no atomics: two calls give the same bits.
 * FIGH_ERR_INVALID (nothing launched, figh_last_error says why): n_geom or n_pairs outside [1, cap], max_iter outside
 * [1, 1024], tol <= 0 or not finite, an unknown kind, a parent that is no joint, a pair naming an object that does not exist
 * (or one object twice), an index outside [0, n_per), ld_b < n_idx n_pairs, ldq < nq.  Without a HIP device:
 * FIGH_ERR_NO_DEVICE, before any argument is looked at. */
#define FIGH_COLLISION_MAX_GEOMETRIES 16
#define FIGH_COLLISION_MAX_PAIRS 64
enum { FIGH_GEOM_BOX = 0, FIGH_GEOM_CYLINDER = 1, FIGH_GEOM_SPHERE = 2, FIGH_GEOM_CAPSULE = 3 };
enum { FIGH_COLLISION_OK = 0, FIGH_COLLISION_CORES_INTERSECT = 1, FIGH_COLLISION_ITERATION_CAP = 2 };
int figh_collision_distances(figh_model_t model, int64_t B, int64_t n_per, int n_idx, const int32_t *h_idx,
                             const double *d_q, int64_t ldq, int n_geom, const int32_t *h_kind, const int32_t *h_parent,
                             const double *h_placement, const double *h_dims, int n_pairs, const int32_t *h_pairs, double tol,
                             int max_iter, double *d_out, int64_t ld_b, double *d_witness, int32_t *d_status);

/* figh_difference_quotients: the constraint Jacobian of the same problem by finite differences (the reference takes
 * nd.Jacobian around constraints, examples/tiago/optimal_trajectory.py:321-327) from the constraint rows that
 * figh_excitation_constraints and figh_collision_distances leave.  d_C: the rows of the stencil, ldc doubles apart: row 0 at
 * X, row 1 + j at X + h_j e_j and, with scheme = 3, row 1 + n_var + j at X - h_j e_j.  d_dx: the n_var steps as the host
 * re-read them ((x + h) - x, or (x + h) - (x - h) for scheme 3).  d_J[i ldj + j] = (C[1 + j][i] - C[0][i]) / dx[j] for
 * scheme = 2 and (C[1 + j][i] - C[1 + n_var + j][i]) / dx[j] for scheme = 3: one subtraction and one IEEE division,
 * bit-equal to the NumPy statement; the dense row-major (n_con, n_var) Jacobian that Ipopt takes, nothing outside
 * [n_con, n_var) of a padded d_J is touched.  FIGH_ERR_INVALID (nothing launched): scheme not 2 or 3, n_var < 1, n_con < 1,
 * ldc < n_con, ldj < n_var.  Without a HIP device: FIGH_ERR_NO_DEVICE, before any argument is looked at. */
int figh_difference_quotients(const double *d_C, int64_t ldc, int64_t n_con, int n_var, int scheme, const double *d_dx,
                              double *d_J, int64_t ldj);

/* figh_singular_values_batch: the singular values of B row-major r x r matrices, stride >= r r doubles apart, of which ONLY
 * THE UPPER TRIANGLE IS READ (figh_regressor_tsqr_batch[_fused] leave the strict lower part undefined) -- the r x r SVDs of
 * the batched condition-number objective (np.linalg.cond(W_b), examples/tiago/optimal_trajectory.py:100-133) without the
 * download of the triangles.  One-sided (Hestenes) Jacobi on the columns in fp64 (csrc/figh_singular.hip states the
 * rotation, its threshold 2^-52 sqrt(alpha beta) and the round-robin order; _host.jacobi_singular_values_mirror is the
 * same statements in NumPy), one workgroup per matrix with the matrix in LDS.  d_sigma[b ld_sigma + k], k < r: the singular
 * values of matrix b IN NO PARTICULAR ORDER; d_status[2 b]: the sweeps used, d_status[2 b + 1]: 1 when a sweep without a
 * rotation ended the matrix, 0 when max_sweeps sweeps did (sigma is then unspecified: the caller recomputes that matrix;
 * a matrix with a non-finite entry ends like this, it is no error of the call).  Every loop of the kernel is bounded by
 * its arguments.  No atomics, plain stores: two calls give the same bits.
 * FIGH_ERR_INVALID (nothing launched): r < 1, B < 1, stride < r r, ld_sigma < r, max_sweeps outside [1, 1000].
 * FIGH_ERR_UNSUPPORTED (nothing launched): r > 128 (the matrix no longer fits the LDS of a compute unit).  Without a HIP
 * device: FIGH_ERR_NO_DEVICE, before any argument is looked at. */
int figh_singular_values_batch(const double *d_R, int64_t B, int r, int64_t stride, int max_sweeps, double *d_sigma,
                               int64_t ld_sigma, int32_t *d_status);

/* ------------------------------------------------------------------ geometric calibration
 * The kinematic regressor and the updated forward kinematics of src/figaroh/calibration/calibration_tools.py, over
 * independent configurations, one per lane.  Conventions: 6-vectors are (linear, angular); a placement
 * (12 doubles: R row-major, then p) maps child to parent coordinates; Ad(M) = [[R, skew(p) R], [0, R]];
 * A_j = oM_parent(j) . jointPlacement_j, oM_j = A_j . M_j(q_j), and a frame on joint j with placement P is oMf = oM_j . P.
 * d_q: N x nq configurations, leading dimension ldq.  meas_mask: bit c set <=> component c of (x y z roll pitch yaw) is
 * measured (param["measurability"]); n_meas is the number of set bits.
 *
 * figh_kinematic_regressor: the loop body of calculate_identifiable_kinematics_model (:1432-1450) for all samples --
 * pin.computeFrameKinematicRegressor(..., LOCAL) and pin.computeFrameJacobian(..., LOCAL) of calculate_kinematics_model
 * (:1387-1391) when start_joint = -1 (universe), get_rel_kinreg (:693-704) and get_rel_jac (:729-739) otherwise.  The end
 * frame sits on end_joint with h_end_placement, the start frame on start_joint with h_start_placement.
 * d_R (n_meas N x 6 (njoints - 1), ldr): row k N + i is row c_k of sample i, c_k the k-th measured component (the
 * reference's rows N c + i of the unmeasured c are zero and deleted at :1452-1456); columns [6 (p - 1), 6 p) hold
 * Ad(oMf^-1 . A_p) for the n_support joints p of h_support (the whole root -> end path for calculate_kinematics_model,
 * get_sup_joints' list otherwise), each of which must lie between the root and the end frame or between the root and the
 * start frame.  d_J (n_meas N x nv, ldj): the columns of joint j on the root -> end path are Ad(oMf^-1 . oM_j) . S_j, minus,
 * with a start frame, the same for the start frame in ITS local frame (J_end - J_start, :737-739); S is (0, axis) for
 * revolute and continuous joints, (axis, 0) for prismatic ones, I6 for a free-flyer.  All other columns are +0.0, written
 * by one memset of the n_meas N x width part of each matrix ahead of the launches; nothing is written outside that part
 * of a padded buffer.  d_rowsq_R / d_rowsq_J (n_meas N doubles): the rows' sums of squares, for the norm < 1e-6 deletion of
 * :1452-1461.  Each of d_R, d_J, d_rowsq_R, d_rowsq_J may be NULL on its own (sums without their matrix: the same walk,
 * nothing stored; for J between two frames through a workspace).  Unlike the reference, nv need not equal njoints - 1.  No atomics: two calls give the
 * same bits.  FIGH_ERR_INVALID (nothing launched, figh_last_error says why): an end or start joint off the model, a
 * support joint off both paths or listed twice, meas_mask outside [1, 63], a leading dimension below the width.  Without a
 * HIP device: FIGH_ERR_NO_DEVICE, before any argument is looked at. */
int figh_kinematic_regressor(figh_model_t model, int64_t N, const double *d_q, int64_t ldq, int end_joint,
                             const double *h_end_placement, int start_joint, const double *h_start_placement,
                             const int32_t *h_support, int n_support, int meas_mask, double *d_R, int64_t ldr, double *d_J,
                             int64_t ldj, double *d_rowsq_R, double *d_rowsq_J);
/* figh_calib_fkm_batch: the loop over the poses of calc_updated_fkm (:1290-1311) for B parameter vectors in one launch (the
 * B = nvar + 1 vectors of a forward-difference Levenberg-Marquardt Jacobian).  h_chain: the n_chain joints whose placements
 * the parameters update (param["actJoint_idx"]); d_placements (B x n_chain x 12): their updated placements
 * (update_joint_placement, :1352-1361, formed by the host in float64); d_wMo / d_eeMf (B x 12): the base and marker
 * transforms (:1214-1251).  Per vector b and pose i: oMee = oM_start^-1 . oM_end with the updated placements
 * (get_rel_transform, :613-617; formed from the last joint both branches share, below which the factors cancel),
 * wMf = wMo[b] . oMee . eeMf[b] (:1300-1301), and the measured components of (translation, matrixToRpy(rotation)) --
 * pitch = atan2(-R20, sqrt(R00^2 + R10^2)), yaw = atan2(R10, R00), roll = atan2(R21, R22) -- go to
 * d_out[b ld_out + k N + i] (PEE.flatten("C"), :1311-1314).  ld_out >= n_meas N.  start_joint = -1: universe.  B is not
 * limited.  FIGH_ERR_INVALID as for figh_kinematic_regressor, and for a chain joint off the model or listed twice; without
 * a HIP device: FIGH_ERR_NO_DEVICE, before any argument is looked at. */
int figh_calib_fkm_batch(figh_model_t model, int64_t B, int64_t N, const double *d_q, int64_t ldq, int n_chain,
                         const int32_t *h_chain, const double *d_placements, const double *d_wMo, const double *d_eeMf,
                         int end_joint, const double *h_end_placement, int start_joint, const double *h_start_placement,
                         int meas_mask, double *d_out, int64_t ld_out);
/* figh_gather_rows: d_out[r, :] = d_W[d_row_idx[r], :] for r < n, cols columns -- np.delete(R, zero_rows, axis=0) (:1456,
 * :1461) with the kept rows listed in order by the caller, who reads the row sums of squares.  Pure copies; n = 0 does
 * nothing.  FIGH_ERR_INVALID: a leading dimension below cols; the indices are not checked. */
int figh_gather_rows(const double *d_W, int64_t ldw, int cols, const int32_t *d_row_idx, int64_t n, double *d_out,
                     int64_t ld_out);

/* ------------------------------------------------------------------ D-optimal posture selection
 * The two passes behind examples/tiago/optimal_config.py and examples/ur10/optimal_config.py over a resident pool of
 * candidate postures.  d_R: the base kinematic regressor as calculate_base_kinematics_regressor leaves it, row-major with
 * leading dimension ldr >= n: row k N + i is measured component k < c (c = param["calibration_index"], 1 .. 6) of candidate
 * i < N, n columns (1 .. FIGH_DESIGN_MAX_COLS).  rearrange_rb (:31-39) is not needed and no X_i = R_i^T R_i of
 * sub_info_matrix (:42-60) is stored.  Addresses are formed in 64 bits (c N ldr may exceed 2^31).
 *
 * figh_design_gram: h_M (n x n, row-major, HOST) = sum_i d_w[i] sum_k r_{k,i} r_{k,i}^T, the Mw of SOCP.add_constraints
 * (:137-140); d_w = NULL: all ones (M_whole of calculate_detroot_whole, :262).  fp64 on the matrix pipe, both triangles
 * written and exactly symmetric, per-workgroup partials through the library's workspace summed in a fixed order: no
 * atomics, two calls give the same bits whatever ldr.  A candidate with d_w[i] = 0 contributes exact zeros.  The call
 * returns when h_M is written.
 *
 * figh_design_scores: h_L (n x n row-major, HOST, lower triangle read) is the Cholesky factor of M.  With
 * G_i = R_i M^-1 R_i^T (c x c):  d_trace[i] = tr G_i (the variance function of the design: max_i <= n (1 + eps) certifies
 * D-efficiency >= 1 / (1 + eps));  d_det_add[i] = det(I + G_i) = det(M + X_i) / det M, the score of Detmax's add scan
 * (:98-104);  d_det_rm[i] = det(I - G_i) = det(M - X_i) / det M, the score of its remove scan (:112-119), +0.0 as soon as
 * a pivot is not positive (M - X_i is not positive definite).  Each output is N doubles and may be NULL on its own, not all
 * three; nothing is written outside the N entries.  The operation order is fixed in the header comment of
 * csrc/figh_design.hip and compiled without FMA contraction: the results are bit-equal to the NumPy mirror
 * (calibration/optimal_design.py).
 *
 * Both: FIGH_ERR_INVALID (nothing launched, figh_last_error says why) for c or n out of range, ldr < n, N < 1, a NULL
 * d_R / h_M / h_L, a diagonal entry of L that is not finite and positive, all outputs NULL.  Without a HIP device:
 * FIGH_ERR_NO_DEVICE, before any argument is looked at. */
#define FIGH_DESIGN_MAX_COLS 96 /* the packed factor (37 KB at 96) and the exchange buffers share 64 KB of LDS */
int figh_design_gram(const double *d_R, int64_t ldr, int64_t N, int c, int n, const double *d_w, double *h_M);
int figh_design_scores(const double *d_R, int64_t ldr, int64_t N, int c, int n, const double *h_L, double *d_trace,
                       double *d_det_add, double *d_det_rm);

/* ------------------------------------------------------------------ multi-GPU (RCCL over xGMI), SURVEY.md section 8e
 * One process per GPU.  Rank 0 calls figh_comm_unique_id and ships the 128 bytes to the other ranks by any
 * means (the Python side uses the torch.distributed store); every rank then calls figh_comm_init.
 * figh_comm_available is the local preflight (librccl loads, every symbol resolves, a HIP device is there): the ranks
 * agree on its outcome BEFORE anybody enters ncclCommInitRank, so that a rank without RCCL cannot leave the others
 * blocked in the rendezvous. */
int figh_comm_available(void);
int figh_comm_unique_id(void *h_id128);
int figh_comm_init(int nranks, int rank, const void *h_id128);
int figh_comm_destroy(void);
/* all-gather of each rank's nc x nc R factor into d_all (nranks*nc x nc), in rank order */
int figh_comm_allgather(const double *d_send, double *d_all, int64_t count_per_rank);
/* in-place sum all-reduce (column norms, Gram blocks, residual norms) */
int figh_comm_allreduce_sum(double *d_buf, int64_t count);

#ifdef __cplusplus
}
#endif
#endif /* FIGH_H */
