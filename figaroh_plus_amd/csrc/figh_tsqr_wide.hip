// K3, wide form, level 0: launcher of the blocked (compact-WY) Householder TSQR for 80 < nc <= 512 columns.  The kernel
// and its geometry table live in figh_tsqr_wide_kernel.h; the pair-merge levels are figh_tsqr_wide_pair.hip.
#include "figh_tsqr_wide_kernel.h"

namespace figh {

// persistent workgroups the wide kernel wants for nc columns (one private triangle each)
long tsqr_wide_workgroups(const int nc, const int cus) {
    int occ = 1;
    wy_dispatch(wy_config(nc), [&](auto NW, auto CPW, auto NRC, auto WPE, auto LDSC) {
        occ = wy_occupancy<decltype(NW)::value, decltype(CPW)::value, decltype(NRC)::value, decltype(WPE)::value,
                           decltype(LDSC)::value>();
    });
    return (long)cus * occ;
}

// rows of (W, ldw) -> nwg triangles (nc x nc, row-major) in Rws_out; tiles are dealt round-robin to the workgroups.
// chain_flags: bit 0 = the workgroups continue from the triangles Rws_out holds (same nwg and nc as the launch before)
int launch_tsqr_wide(const double *W, long rows, long ldw, const int *col_idx, int n, const double *tau,
                     const double *d_blkw, long rows_per_blk, int nc, long nwg, double *Rws_out, int chain_flags) {
    if (chain_flags & 1)  // the CHAIN instantiations live in figh_tsqr_wide_batch.hip
        return launch_tsqr_wide_chain(W, rows, ldw, col_idx, n, tau, d_blkw, rows_per_blk, nc, nwg, Rws_out);
    const int nch = (nc + 15) >> 4;
    const size_t blk_bytes = sizeof(double) * 256 * ((size_t)nch * (nch + 1) / 2) * (size_t)nwg;
    double *Rblk = static_cast<double *>(workspace(blk_bytes, kWsWideBlkOrFilter));
    if (!Rblk) return FIGH_ERR_ALLOC;
    const bool ok = wy_dispatch(wy_config(nc), [&](auto NW, auto CPW, auto NRC, auto WPE, auto LDSC) {
        FIGH_LAUNCH_TIMED((tsqr_wy_kernel<decltype(NW)::value, decltype(CPW)::value, decltype(NRC)::value,
                                          decltype(WPE)::value, decltype(LDSC)::value, 0>),
                          dim3((unsigned)nwg), dim3(64 * decltype(NW)::value), 0, W, rows, ldw, col_idx, n, tau, d_blkw,
                          rows_per_blk, Rblk, Rws_out, nc, 0L, 0, null_pivot_sq());
    });
    if (!ok) {
        set_error("figh_tsqr: no wide-kernel geometry for this column count");
        return FIGH_ERR_UNSUPPORTED;
    }
    FIGH_HIP(hipGetLastError());
    return FIGH_OK;
}

}  // namespace figh
