"""GPU suite: the public entries of include/figh.h that no test called directly.

* figh_tsqr_structured with a HOST hint (the suite only ran the device-derived hint of figh_tsqr_selected; the host path's
  tile_hint_kernel only ever saw six blocks in ascending order): graded integer matrices whose zero structure is the hint
  (call_sequence_common.Hinted: every row carries the largest entry there is at its block's first column, so a hint on
  the wrong rows or the wrong tile destroys R), with the metrics and tolerances of test_qr_graded._check;
* figh_base_permutation against the index logic of figh.h;
* figh_coupling_tx40 as a stand-alone call, bit for bit;
* figh_model_set_active_rows at the ABI: link-padded layout, reset, a second handle, and the three paths figh.h says ignore
  the setting;
* figh_regressor_shape / _link_layout / _force_layout against a derivation from Model.to_flat() alone.

Refusal tests use only checks the library makes on the host before any launch (the FIGH_REQUIRE lines of tile_hint,
figh_coupling_tx40).
"""
import ctypes as C

import numpy as np
import pytest

import call_sequence_common as cs
import qr_graded_common as qg
import reductions_common as rc
import regressor_exact as rx
from test_qr_graded import _check

pytestmark = pytest.mark.gpu

SENT = cs.SENT
GUARD = -559038737  # guard word behind an int32 result


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    qg.check_longdouble()
    return _lib


def _dev(lib, x, dtype=None):
    return lib.DeviceArray.from_host(np.ascontiguousarray(x, dtype=dtype).reshape(-1))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and bool(np.array_equal(_bits(a), _bits(b)))


# ------------------------------------------------------------------------------------------- figh_tsqr_structured, host hint
def _structured(lib, h, first=None):
    d_R = _dev(lib, np.full(h.nc * h.nc, SENT))
    lib.tsqr(_dev(lib, h.A()), h.rows, h.ld, None if h.idx is None else _dev(lib, h.idx, np.int32), h.n,
             None if h.mt is None else _dev(lib, h.tau()), h.weights(), d_R, first_cols=h.first if first is None else first)
    return d_R.to_host().reshape(h.nc, h.nc)


@pytest.mark.parametrize("case", cs.STRUCTURED_CASES, ids=[c[0] for c in cs.STRUCTURED_CASES])
def test_tsqr_structured_host_hint(lib, case, record_property):
    """R of figh_tsqr_structured under a true hint (zeros, ascending, descending, random, a block that lives on its tau
    alone; unsorted gather out of a wider ld, tau, power-of-two row-block weights) against the exact Gram: backward for
    every shape, forward and diagonal when rows >= 2 nc.  At 81 columns the hint is ignored and R must still be right."""
    h = cs.structured_case(case)
    R = np.triu(_structured(lib, h))
    assert not (R == SENT).any(), "an element of the triangle was never written"
    _check(R, h.gram(), record_property, "structured_" + case[0], forward=h.forward())


def test_tsqr_structured_refusals_come_before_any_launch(lib):
    """tile_hint's host checks: rows % nfirst != 0, first[b] > n, first[b] < 0 -> FIGH_ERR_INVALID, the output untouched."""
    h = cs.structured_case(cs.STRUCTURED_CASES[2])  # 600 x 16, six blocks
    for bad in ([0] * 7, [0, 2, 5, 8, 10, h.n + 1], [0, 2, -1, 8, 10, 13]):
        d_R = _dev(lib, np.full(h.nc * h.nc, SENT))
        with pytest.raises(lib.FighError) as err:
            lib.tsqr(_dev(lib, h.A()), h.rows, h.ld, _dev(lib, h.idx, np.int32), h.n, None, None, d_R, first_cols=bad)
        assert err.value.code == lib.ERR_INVALID
        assert (d_R.to_host() == SENT).all(), "a refused call wrote to its output"


# ----------------------------------------------------------------------------------------------------- figh_base_permutation
def _perm_ref(diag, nc, n, tol):
    """figh.h: [i < n : |R_ii| > tol_qr, ascending], the remaining i < n, then n .. nc - 1."""
    big = np.abs(diag[:n]) > tol
    return np.r_[np.flatnonzero(big), np.flatnonzero(~big), np.arange(n, nc)].astype(np.int32)


def _diagonals(rng, nc, tol):
    i = np.arange(nc)
    up, big, small = np.nextafter(tol, np.inf), 4.0 * tol + 1.0, 0.25 * tol
    pats = {
        "all_base": np.full(nc, big), "none_base": np.full(nc, small),
        "alternating": np.where(i % 2 == 0, big, small), "alternating_64": np.where((i // 64) % 2 == 0, small, big),
        "every_third_across_lanes": np.where((i + i // 64) % 3 == 0, big, small),
        "at_tol_and_one_ulp_above": np.where(i % 2 == 0, tol, up), "negative": -np.where(i % 3 == 0, up, tol),
        "signed_zeros": np.where(i % 2 == 0, 0.0, -0.0), "random": np.where(rng.random(nc) < 0.5, -big, small),
    }
    pats["negative"] = np.where(i % 5 == 0, -big, pats["negative"])
    return pats


@pytest.mark.parametrize("nc", [1, 63, 64, 65, 129, 512])
def test_base_permutation_exact(lib, nc):
    """d_perm equals the NumPy reference exactly for n = nc, nc - 1, nc - 3; diagonals at tol_qr (not base), one ulp above
    it, negative, +-0.0, all / none base, alternating patterns across the 64-lane boundary, tol_qr = 0; the off-diagonal
    entries are NaN (never read), and the guard word behind entry nc stays."""
    rng = np.random.default_rng(nc)
    for tol in (1e-8, 0.0):
        pats = _diagonals(rng, nc, tol)
        if tol == 0.0:
            pats["subnormal_and_zero"] = np.where(np.arange(nc) % 2 == 0, 5e-324, -0.0)
        for name, diag in pats.items():
            R = np.full((nc, nc), np.nan)
            R[np.arange(nc), np.arange(nc)] = diag
            d_R = _dev(lib, R)
            for n in sorted({nc, nc - 1, nc - 3}):
                if n < 1:
                    continue
                d_perm = _dev(lib, np.full(nc + 1, GUARD), np.int32)
                lib.base_permutation(d_R, nc, n, tol, d_perm)
                got = d_perm.to_host()
                assert got[nc] == GUARD, "%s nc=%d n=%d: the word behind d_perm was written" % (name, nc, n)
                assert np.array_equal(got[:nc], _perm_ref(diag, nc, n, tol)), "%s nc=%d n=%d tol=%g" % (name, nc, n, tol)


# -------------------------------------------------------------------------------------------------------- figh_coupling_tx40
def _coupling_inputs(rng, N, nv):
    v, a = rng.standard_normal((N, nv)), rng.standard_normal((N, nv))
    tiny, huge = 5e-324, 1.0e308
    special = [(1.5, -1.5), (-0.0, -0.0), (0.0, -0.0), (tiny, -tiny), (tiny, tiny), (-tiny, 0.0), (huge, -huge), (huge, huge),
               (-huge, 1.0), (2.0 ** -1060, -2.0 ** -1061)]
    for k, (x, y) in enumerate(special):
        i = (k * 7) % N  # (N = 1: the last one stays)
        v[i, 4], v[i, 5] = x, y
        a[i, 4], a[i, 5] = y, -x
    return v, a


@pytest.mark.parametrize("nv", [6, 7, 9])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 4097])
def test_coupling_tx40_bit_for_bit(lib, N, nv):
    """Every one of the 6 N x 3 entries is written: the rows of joints 5 and 6 are [a6 v6 sign(v5 + v6)] and
    [a5 v5 sign(v5 + v6)] bit for bit, everything else +0.0.  v5 + v6 == 0 exactly, -0.0, subnormals, huge values."""
    v, a = _coupling_inputs(np.random.default_rng([N, nv]), N, nv)
    d_out = _dev(lib, np.full(6 * N * 3, SENT))
    lib.coupling_tx40(N, nv, _dev(lib, v), _dev(lib, a), d_out)
    out = d_out.to_host().reshape(6 * N, 3)
    with np.errstate(over="ignore"):
        s = np.sign(v[:, 4] + v[:, 5])
    ref = np.zeros((6 * N, 3))
    ref[4 * N:5 * N] = np.c_[a[:, 5], v[:, 5], s]
    ref[5 * N:6 * N] = np.c_[a[:, 4], v[:, 4], s]
    assert set(np.unique(s)) <= {-1.0, 0.0, 1.0} and (N < 64 or (s == 0).sum() >= 4)
    bad = np.argwhere(_bits(out) != _bits(ref))
    assert bad.size == 0, "N=%d nv=%d: %d entries differ, first (row %d, column %d): %r, expected %r" % (
        N, nv, len(bad), bad[0][0], bad[0][1], out[tuple(bad[0])], ref[tuple(bad[0])])


def test_coupling_tx40_refuses_five_dofs(lib):
    d_out = _dev(lib, np.full(6 * 8 * 3, SENT))
    z = _dev(lib, np.zeros(8 * 5))
    with pytest.raises(lib.FighError) as err:
        lib.coupling_tx40(8, 5, z, z, d_out)
    assert err.value.code == lib.ERR_INVALID
    assert (d_out.to_host() == SENT).all()


# ----------------------------------------------------------------------------------- figh_model_set_active_rows at the ABI
ALL_FLAGS = dict(friction=True, inertia=True, offset=True)


def _tree_model(name):
    """(robot, key of the flat model for regressor_exact.reference)."""
    if name == "tiago":
        from figaroh_plus_amd.tools.robot import Robot
        return Robot.from_flat("tiago"), "tiago"
    from test_regressor_entrywise import _tree
    return _tree(name, False)


def _padded_build(lib, h, mode, flags, ft, N, dq, dv, da, rows, nl):
    d_W = _dev(lib, np.full(rows * 16 * nl, SENT))
    d_cs = _dev(lib, np.full(14 * nl, SENT))
    lib.regressor_build_padded(h, mode, flags, ft, N, dq, dv, da, d_W, 16 * nl, d_cs)
    return d_W.to_host().reshape(rows, 16 * nl), d_cs.to_host()


@pytest.mark.parametrize("N", [65, 209])
@pytest.mark.parametrize("name", ["fork", "tiago"])
def test_active_rows_link_padded_layout(lib, name, N, record_property):
    """Link-padded W into a sentinel-filled buffer: the stored row blocks equal those of a build with all rows active bit for
    bit (and the long-double reference entry by entry), the rows of the other blocks keep the sentinel, d_colsq still covers
    every row block, the reset restores the first build bit for bit, and a second handle of the same model never notices."""
    from figaroh_plus_amd.tools.regressor import _samples_to_device, regressor_flags
    robot, key = _tree_model(name)
    param = rx.base_param(**ALL_FLAGS)
    (q, v, a), ref = rx.reference(key, "unit", N, param, seed=5)
    flat = robot.model.to_flat()
    hA, hB = lib.ModelHandle(flat), lib.ModelHandle(flat)
    nl, nv = hA.njoints - 1, hA.nv
    mode, flags, ft = regressor_flags(param)
    _, dq, dv, da = _samples_to_device(robot.model, q, v, a)
    args = (mode, flags, ft, N, dq, dv, da, nv * N, nl)
    c = np.arange(14 * nl)
    dev = 16 * (c // 14) + c % 14
    W_full, cs_full = _padded_build(lib, hA, *args)
    assert not (W_full == SENT).any() and not W_full[:, np.setdiff1d(np.arange(16 * nl), dev)].any()
    ratio = rx.assert_entrywise(W_full[:, dev], ref, rx.C_TOL, "%s N=%d all rows" % (name, N))
    record_property("entry_ratio", round(ratio, 2))
    active = sorted(set(range(0, nv, 3)) | {nv - 1})
    hA.set_active_rows(active)
    W_act, cs_act = _padded_build(lib, hA, *args)
    stored = np.repeat(np.isin(np.arange(nv), active), N)
    assert _same_bits(W_act[stored], W_full[stored]), "a stored row block differs from the build with all rows active"
    assert (W_act[~stored] == SENT).all(), "a row block that is not active was written"
    rx.assert_entrywise(W_act[stored][:, dev], rx.Ref(ref.W[stored], ref.S[stored], ref.copied), rx.C_TOL, "%s stored blocks" % name)
    r = rc.colsq_ratio(cs_act, rc.colsq_ld(W_full[:, dev]), nv * N)
    record_property("colsq_over_bound", "%.3e" % float(r.max()))
    assert (r <= 1.0).all(), "d_colsq no longer covers every row block: columns %s" % np.flatnonzero(~(r <= 1.0))[:8].tolist()
    W_B, cs_B = _padded_build(lib, hB, *args)  # (A still restricted)
    assert _same_bits(W_B, W_full) and _same_bits(cs_B, cs_full), "a second handle of the model saw the first one's setting"
    hA.set_active_rows(None)
    W_again, cs_again = _padded_build(lib, hA, *args)
    assert _same_bits(W_again, W_full) and _same_bits(cs_again, cs_full), "the reset does not restore the first build"


def test_active_rows_ignored_where_the_header_says_so(lib):
    """With rows set, figh_regressor_build (reference layout, tree), a chain model's build and an external-wrench
    build_padded on a free-flyer tree give the bits of the unset handle."""
    from figaroh_plus_amd.tools.regressor import _samples_to_device, regressor_flags
    from figaroh_plus_amd.tools.robot import Robot
    from test_regressor_entrywise import _tree
    N = 65

    def both(robot, key, param, build):
        (q, v, a), _ = rx.reference(key, "unit", N, param, seed=5)
        flat = robot.model.to_flat()
        _, dq, dv, da = _samples_to_device(robot.model, q, v, a)
        mode, flags, ft = regressor_flags(param)
        out = []
        for rows in (None, [0, 2]):
            h = lib.ModelHandle(flat)
            if rows is not None:
                h.set_active_rows(rows)
            out.append(build(h, mode, flags, ft, dq, dv, da))
        for x, y in zip(*out):
            assert not (x == SENT).any() and _same_bits(x, y)

    def dense(h, mode, flags, ft, dq, dv, da):
        rps, ncols = h.shape(mode, flags)
        d_W, d_cs = _dev(lib, np.full(rps * N * ncols, SENT)), _dev(lib, np.full(ncols, SENT))
        lib.regressor_build(h, mode, flags, ft, N, dq, dv, da, d_W, ncols, d_cs)
        return d_W.to_host(), d_cs.to_host()

    def padded_wrench(h, mode, flags, ft, dq, dv, da):
        nl = h.njoints - 1
        return _padded_build(lib, h, mode, flags, ft, N, dq, dv, da, 6 * N, nl)

    robot, key = _tree("fork", False)
    both(robot, key, rx.base_param(**ALL_FLAGS), dense)
    both(Robot.from_flat("ur10"), "ur10", rx.base_param(**ALL_FLAGS), dense)
    robot, key = _tree("fork", True)
    both(robot, key, rx.base_param(wrench=True), padded_wrench)


# ------------------------------------------------------------------------------------------------ shape and layout queries
FREEFLYER = 3  # jtype of a free-flyer joint in Model.to_flat()
FLAG_BITS = (1, 2, 4)  # friction, actuator inertia, offset


def derive_layout(flat, mode, flags, ft_mask):
    """What figh.h promises, from the flat model alone: (rows per sample or None when the mode does not fit the model,
    ncols, link_pos or None, nlive, ld_force or 0)."""
    nl, nv = int(flat["njoints"]) - 1, int(flat["nv"])
    joint_torque = mode == 0
    rps = (nv if nl == nv else None) if joint_torque else 6
    ncols = 14 * nl + (3 if flags & 8 else 0)
    ff = nl >= 1 and int(flat["jtype"][1]) == FREEFLYER
    if joint_torque or not ff or flags & 8:
        return rps, ncols, None, 0, 0
    extras = bool(flags & 7)
    body = np.asarray(flat["mass"], dtype=float)[1:] != 0.0
    live = (body & bool(ft_mask & 63)) | extras
    pos = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)
    nlive = int(live.sum())
    return rps, ncols, pos, nlive, (0 if extras or nlive == 0 else 16 * -(-nlive // 4))


def _query(lib, h, mode, flags, ft):
    """(rc, rows per sample, ncols), (rc, link_pos, nlive), (rc, ld_force) straight from the C entries."""
    L = lib.load()
    r, c = C.c_int(-1), C.c_int(-1)
    rc_s = L.figh_regressor_shape(h.handle, mode, flags, C.byref(r), C.byref(c))
    pos = np.full(h.njoints - 1, -7, dtype=np.int32)
    nlive = C.c_int(-7)
    rc_l = L.figh_regressor_link_layout(h.handle, mode, flags, ft, pos.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nlive))
    ldf = C.c_int64(-7)
    rc_f = L.figh_regressor_force_layout(h.handle, mode, flags, ft, C.byref(ldf))
    return (rc_s, r.value, c.value), (rc_l, pos, nlive.value), (rc_f, ldf.value)


def _layout_models():
    from figaroh_plus_amd.tools.robot import Robot
    from test_gpu_parity import _TREES
    from test_regressor_entrywise import _tree
    for name in ("tx40", "ur10", "tiago", "talos", "human"):
        yield name, Robot.from_flat(name).model.to_flat()
    for shape in sorted(_TREES):
        yield shape + "-ff", _tree(shape, True)[0].model.to_flat()


def test_shape_and_layout_queries_against_the_flat_model(lib):
    """figh_regressor_shape, _link_layout and _force_layout for the five shipped models and the synthetic free-flyer trees,
    both modes, all eight flag sets (and the TX40 coupling flag on the 6-dof chains), ft_mask in {63, 7, 56, 1}: equal to the
    derivation; FIGH_ERR_UNSUPPORTED where a layout does not apply."""
    seen = {"link": 0, "force": 0, "unsupported": 0, "massless": 0}
    for name, flat in _layout_models():
        h = lib.ModelHandle(flat)
        chain6 = name in ("tx40", "ur10")
        for mode in (lib.MODE_JOINT_TORQUE, lib.MODE_EXT_WRENCH):
            for f in range(8):
                for tx in ((0, lib.FLAG_TX40) if chain6 and mode == lib.MODE_JOINT_TORQUE else (0,)):
                    flags = sum(b for b in FLAG_BITS if f & b) | tx
                    for ft in (63, 7, 56, 1):
                        what = "%s mode %d flags %d ft %d" % (name, mode, flags, ft)
                        rps, ncols, pos, nlive, ldf = derive_layout(flat, mode, flags, ft)
                        (rc_s, r, c), (rc_l, got_pos, got_live), (rc_f, got_ldf) = _query(lib, h, mode, flags, ft)
                        if rps is None:
                            assert rc_s == lib.ERR_INVALID, what
                        else:
                            assert (rc_s, r, c) == (lib.FIGH_OK, rps, ncols), what
                        if pos is None:
                            assert rc_l == lib.ERR_UNSUPPORTED and rc_f == lib.ERR_UNSUPPORTED, what
                            seen["unsupported"] += 1
                            continue
                        assert rc_l == lib.FIGH_OK and got_live == nlive and np.array_equal(got_pos, pos), what
                        seen["link"] += 1
                        seen["massless"] += int(nlive < len(pos))
                        if ldf:
                            assert (rc_f, got_ldf) == (lib.FIGH_OK, ldf), what
                            seen["force"] += 1
                        else:
                            assert rc_f == lib.ERR_UNSUPPORTED, what
    assert min(seen.values()) > 0, seen
