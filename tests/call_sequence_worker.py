"""One family of the call-sequence tests (tests/test_call_sequences.py) in a fresh process: every workspace slot of
libfigh starts empty and every host-side cache cold.  Performs the steps of call_sequence_common.steps(family) in order,
checks nothing but the status codes (a failing call raises) and writes every raw result to the .npz named on the command
line, keyed "<step tag>/<result name>".  The parent test judges them.

    python tests/call_sequence_worker.py <family> <out.npz>
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402

import call_sequence_common as cs  # noqa: E402
import qr_graded_common as qg  # noqa: E402
from figaroh_plus_amd import _lib as lib  # noqa: E402


def _dev(x, dtype=None):
    return lib.DeviceArray.from_host(np.ascontiguousarray(x, dtype=dtype).reshape(-1))


def _opt(x, dtype=None):
    return None if x is None else _dev(x, dtype)


def run_tsqr(a):
    h = a["h"]
    d_R = _dev(np.full(h.nc * h.nc, cs.SENT))
    lib.tsqr(_dev(h.A()), h.rows, h.ld, _opt(h.idx, np.int32), h.n, _opt(h.tau()), h.weights(), d_R,
             first_cols=h.first if a["hint"] else None)
    return {"R": d_R.to_host().reshape(h.nc, h.nc)}


def run_tsqr_selected(a):
    g = a["g"]
    nc = g.n + 1
    d_sel = lib.DeviceArray((2 + 2 * g.ncols,), np.int32)
    d_R = _dev(np.full(nc * nc, cs.SENT))
    lib.tsqr_selected(_dev(g.A()), g.rows, g.ncols, _dev(g.colsq()), g.ncols, g.tol_e(), 14, g.nblocks, g.n, _dev(g.tau()),
                      -1.0, d_sel, d_R)
    return {"R": d_R.to_host().reshape(nc, nc), "sel": d_sel.to_host()}


def run_merge(a):
    g = a["g"]
    d_R = _dev(np.full(g.nc * g.nc, cs.SENT))
    lib.tsqr_merge(_dev(g.A()), g.count, g.nc, d_R)
    return {"R": d_R.to_host().reshape(g.nc, g.nc)}


def run_merge_base(a):
    g = a["g"]
    d_out = _dev(np.full((g.nc + 1) * g.nc, cs.SENT))
    lib.tsqr_merge_base(_dev(g.A()), g.count, g.nc, g.n_free, cs.TOL_QR, d_out)
    return {"rows": d_out.to_host().reshape(g.nc + 1, g.nc)}


def run_filtfilt(a):
    x = a["x"]
    rows, cols = x.shape
    Lout = -(-(rows // a["nblocks"]) // a["q"])
    d_y = _dev(np.full((Lout * a["nblocks"] + 3) * cols, cs.SENT))
    got = lib.filtfilt_cols(_dev(x), rows, cols, cols, a["nblocks"], a["form"], a["b"], a["a"], a["zi"], a["padlen"], a["q"],
                            d_y, cols)
    return {"y": d_y.to_host().reshape(-1, cols), "rows_out": np.int64(got)}


def run_wrench(a):
    g, with_tau = a["g"], a["with_tau"]
    compact = a["layout"] == "force-link-compact"
    assert a["layout"] in ("force-compact", "force-link-compact")
    buf, ldw = g.force_compact(compact)
    nc = g.n + (1 if with_tau else 0)
    cs_ = g.colsq()
    d_sel = lib.DeviceArray((2 + 2 * g.ncols,), np.int32)
    d_R = _dev(np.full((nc + 1) * nc, cs.SENT))
    lib.tsqr_selected_wrench(_dev(buf), g.rows, ldw, _dev(cs_), g.ncols, 0.5 * cs_[cs_ > 0].min(), 16, g.n, g.nf,
                             _opt(g.tau() if with_tau else None), -1.0, d_sel, d_R,
                             d_link_pos=_dev(g.link_pos, np.int32) if compact else None, ld_force=g.force_ld(compact))
    return {"R": d_R.to_host()[:nc * nc].reshape(nc, nc), "sel": d_sel.to_host()}


def run_blocks(a):
    g, with_tau = a["g"], a["with_tau"]
    nc = g.n + (1 if with_tau else 0)
    cs_ = g.colsq()
    counts, cols, pos = g.block_columns(16)
    off = ld = None
    if a["compact"]:
        buf, off, ld, cols = g.compact()
        ldw = 1
    else:
        buf = g.dense(16)
        ldw = buf.shape[1]
    d_sel = lib.DeviceArray((2 + 2 * g.ncols,), np.int32)
    d_R = _dev(np.full((nc + 1) * nc, cs.SENT))
    nstack = int(g.stack_offsets(with_tau)[-1])
    d_tri = _dev(np.full((nstack + nc + 1) * nc, cs.SENT)) if a["want_tri"] else None
    lib.tsqr_selected_blocks(_dev(buf), g.rows, ldw, _dev(cs_), g.ncols, 0.5 * cs_[cs_ > 0].min(), 16, g.n, counts,
                             _dev(cols, np.int32), _dev(pos, np.int32), _opt(g.tau() if with_tau else None), -1.0, d_sel, d_R,
                             block_off=off, block_ld=ld, d_block_tri=d_tri)
    out = {"R": d_R.to_host()[:nc * nc].reshape(nc, nc), "sel": d_sel.to_host()}
    if d_tri is not None:
        out["stack"] = d_tri.to_host()[:nstack * nc].reshape(nstack, nc)
    return out


def _robot(model):
    from figaroh_plus_amd.tools.robot import Robot
    return Robot.from_flat(model)


def run_fused(a):
    from figaroh_plus_amd.tools.regressor import _samples_to_device
    robot = _robot("ur10")
    N, d_q, d_v, d_a = _samples_to_device(robot.model, a["q"], a["v"], a["a"])
    kept = cs.fused_kept()
    n, nc = len(kept), len(kept) + 1
    d_W = _dev(np.full(6 * N * 84, cs.SENT))
    d_cs = lib.DeviceArray((84,))
    d_R = _dev(np.full(nc * nc, cs.SENT))
    ok = lib.regressor_tsqr_fused(robot.device_model(), 0, N, d_q, d_v, d_a, d_W, 84, d_cs, _dev(kept, np.int32), n,
                                  _dev(a["tau"]), -1.0, d_R)
    return {"served": np.int64(ok), "W": d_W.to_host().reshape(6 * N, 84), "colsq_fused": d_cs.to_host(),
            "R": d_R.to_host().reshape(nc, nc)}


_STREAM = {}


def _stream(model):
    """(handle, mode, flags, ft, device q v a of all samples) of a streamed-family model, made once per process."""
    if model not in _STREAM:
        from figaroh_plus_amd.tools.regressor import _samples_to_device, regressor_flags
        param, (q, v, a), _ = cs.stream_inputs(model)
        robot = _robot(model)
        mode, flags, ft = regressor_flags(param, False)
        _STREAM[model] = (robot, robot.device_model(), mode, flags, ft) + tuple(_samples_to_device(robot.model, q, v, a)[1:])
    return _STREAM[model]


def run_rbuild(a):
    robot, h, mode, flags, ft, d_q, d_v, d_a = _stream(a["model"])
    N = cs.stream_total(a["model"])
    rps, ncols = h.shape(mode, flags)
    d_W = _dev(np.full(rps * N * ncols, cs.SENT))
    d_cs = lib.DeviceArray((ncols,))
    lib.regressor_build(h, mode, flags, ft, N, d_q, d_v, d_a, d_W, ncols, d_cs)
    return {"W": d_W.to_host().reshape(rps * N, ncols), "colsq": d_cs.to_host()}


def run_rcolsq(a):
    robot, h, mode, flags, ft, d_q, d_v, d_a = _stream(a["model"])
    ncols = h.shape(mode, flags)[1]
    d_cs = _dev(np.full(ncols, cs.SENT))
    lib.regressor_colsq(h, mode, flags, ft, cs.STREAM_N, d_q, d_v, d_a, d_cs, chunk_samples=a["chunk"])
    return {"colsq": d_cs.to_host()}


def run_rtsqr(a):
    robot, h, mode, flags, ft, d_q, d_v, d_a = _stream(a["model"])
    ncols = h.shape(mode, flags)[1]
    kept = cs.stream_kept(a["model"])
    n, nc = len(kept), len(kept) + 1
    d_R = _dev(np.full(nc * nc, cs.SENT))
    d_cs = _dev(np.full(ncols, cs.SENT)) if a["norms"] else None
    lib.regressor_tsqr(h, mode, flags, ft, cs.STREAM_N, d_q, d_v, d_a, _dev(kept, np.int32), n,
                       _dev(cs.stream_inputs(a["model"])[2]), None, d_R, chunk_samples=a["chunk"], d_colsq=d_cs)
    out = {"R": d_R.to_host().reshape(nc, nc)}
    if d_cs is not None:
        out["colsq"] = d_cs.to_host()
    return out


def run_rbatch(a):
    robot, h, mode, flags, ft, d_q, d_v, d_a = _stream(a["model"])
    kept = cs.stream_kept(a["model"])
    n = len(kept)
    d_R = _dev(np.full(cs.BATCH_B * n * n, cs.SENT))
    lib.regressor_tsqr_batch(h, mode, flags, ft, cs.BATCH_B, cs.STREAM_N, d_q, d_v, d_a, _dev(kept, np.int32), n, None, d_R)
    return {"R": d_R.to_host().reshape(cs.BATCH_B, n, n)}


def run_rgram(a):
    robot, h, mode, flags, ft, d_q, d_v, d_a = _stream(a["model"])
    kept = cs.stream_kept(a["model"])
    G, g, tt = lib.regressor_gram(h, mode, flags, ft, cs.STREAM_N, d_q, d_v, d_a, _dev(kept, np.int32), len(kept),
                                  _dev(cs.stream_inputs(a["model"])[2]), a["chunk"])
    return {"G": G, "g": g, "tt": np.float64(tt)}


def run_tsqr_deps(a):
    g = a["g"]
    d_R = _dev(np.full(g.n * g.n, cs.SENT))
    with lib.null_pivots(cs.TOL_QR if a["rule"] else 0.0):
        lib.tsqr(_dev(g.A()), g.rows, g.n, None, g.n, None, None, d_R)
    return {"R": d_R.to_host().reshape(g.n, g.n)}


def run_build_profile(a):
    from figaroh_plus_amd.tools.regressor import _samples_to_device, regressor_flags
    robot = _robot(a["model"])
    mode, flags, ft = regressor_flags(a["param"], False)
    h = robot.device_model()
    rps, ncols = h.shape(mode, flags)
    N, d_q, d_v, d_a = _samples_to_device(robot.model, a["q"], a["v"], a["a"])
    d_W = _dev(np.full(rps * N * ncols, cs.SENT))
    lib.profile_enable(a["level"] > 0, a["level"])
    try:
        lib.regressor_build(h, mode, flags, ft, N, d_q, d_v, d_a, d_W, ncols, None)
        W = d_W.to_host().reshape(rps * N, ncols)
    finally:
        lib.profile_enable(False)
    return {"W": W}


def run_active_rows_ab(a):
    """Two private handles of one model; A's active rows change between (and around) two builds on B."""
    from figaroh_plus_amd.tools.regressor import _samples_to_device, regressor_flags
    robot = _robot(a["model"])
    flat = robot.model.to_flat()
    hA, hB = lib.ModelHandle(flat), lib.ModelHandle(flat)
    mode, flags, ft = regressor_flags(a["param"], False)
    nl = hB.njoints - 1
    N, d_q, d_v, d_a = _samples_to_device(robot.model, a["q"], a["v"], a["a"])
    out = {}

    def build(h, tag):
        d_W = _dev(np.full(hB.nv * N * 16 * nl, cs.SENT))
        d_c = lib.DeviceArray((14 * nl,))
        lib.regressor_build_padded(h, mode, flags, ft, N, d_q, d_v, d_a, d_W, 16 * nl, d_c)
        out["W_" + tag], out["colsq_" + tag] = d_W.to_host().reshape(hB.nv * N, 16 * nl), d_c.to_host()

    build(hB, "B1")
    hA.set_active_rows(a["rows_a"])
    build(hA, "A")
    build(hB, "B2")
    hA.set_active_rows(None)
    build(hB, "B3")
    return out


RUN = {"tsqr": run_tsqr, "tsqr_selected": run_tsqr_selected, "merge": run_merge, "merge_base": run_merge_base,
       "filtfilt": run_filtfilt, "wrench": run_wrench, "blocks": run_blocks, "fused": run_fused, "rbuild": run_rbuild,
       "rcolsq": run_rcolsq, "rtsqr": run_rtsqr, "rbatch": run_rbatch, "rgram": run_rgram, "tsqr_deps": run_tsqr_deps,
       "build_profile": run_build_profile, "active_rows_ab": run_active_rows_ab}


def main(family, out_path):
    lib.load()
    if lib.device_count() <= 0:
        raise SystemExit("call_sequence_worker: no HIP device")
    qg.check_longdouble()
    results = {}
    for step in cs.steps(family):
        for name, val in RUN[step.op](step.args).items():
            results[cs.result_key(step.tag, name)] = np.asarray(val)
        lib.synchronize()
        print("step %s ok" % step.tag, flush=True)
    np.savez(out_path, **results)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
