"""CPU tests of tests/regressor_exact.py: the long-double reference is right (against a 50-digit evaluation), the entry scale
bounds the entries and vanishes on the structural zero pattern only, the two float64 oracles stay within C_ORACLE of it,
the scale hides nothing (tightness per row block, link and slot group), and the entry-wise metric rejects planted errors
that the norm-wise check ``max |W - ref| <= 1e-12 max |ref|`` accepts.

Measured here (N = 200, seed 0; entry_ratio in units of u S; both oracles have exact zeros wherever S == 0 and equal copied
columns in every case):
  C oracle      five models: 2.1 .. 11.2 (largest: TALOS, one); random trees, fixed and floating base: up to 23.5 (13-link
                chain under a free-flyer, mixed; 16.4 in static)
  NumPy oracle  five models: 2.0 .. 12.5 (largest: human, static); random trees: up to 17.8 (the same tree, mixed)
  => C_ORACLE = 23.5, C_TOL = 8 C_ORACLE rounded up to a power of two = 256.  The ratio does not grow with N (N = 16: up to
  8.2 on the five models); it grows slowly with the depth of the tree, and it is largest in static / one / mixed.
Tightness (rms S / rms |W_ld| per row block, link and slot group, N = 64, all seven regimes): medians 2.6 .. 35.4 (cap 64);
groups above 2^8: TX40 2 .. 10 of 53, UR10 2 .. 10 of 56, TIAGo 12 .. 36 of 190 (most in static: 19 %, cap 25 %), TALOS 2 .. 3
of 492, human none of 279 (largest 250).  Regimes reach and the pi / 2 block of bigq behave like unit (UR10: 2 of 56, median
14.5 / 13.6).  The groups above 2^8 are the mass and first-moment groups in the rows of joints whose axis is parallel to
gravity (TX40 joint_1, UR10 shoulder_pan_joint; TIAGo's casters and their wheels, torso_lift_joint, arm_1_joint, head_1_joint;
TALOS two mass slots in the Mz rows), where the gravity term vanishes geometrically -- W_ld is then 1e-20 S, or exactly zero in
1 (TX40, UR10), 10 (TIAGo), 2 (TALOS) groups -- and u S is what a float64 evaluation can deliver.
Planted errors (old check in units of its tolerance / new ratio in u S; UR10, TIAGo, TALOS): (i) 0.25 / 2.9e3 .. 1.4e11 (dropped
everywhere the term reaches 2.2 .. 4.4 of the old tolerance in regime static, so it is dropped where it is below a quarter
of it), (ii) 0.38 .. 0.49 / 9.0e9, (iii) 0.23 .. 0.40 / 1.2e3 .. 2.1e3, (iv) 1e-6 / 6e15 .. 9e15.
"""
import numpy as np
import pytest

import oracle_np
import regressor_exact as rx

MODELS = ["tx40", "ur10", "tiago", "talos", "human"]
N_ORACLE = 200


def _param_of(name, **kw):
    return rx.base_param(wrench=name in ("talos", "human"), **kw)


def _tree_flat(shape, freeflyer):
    from test_gpu_parity import _TREES, _synthetic_tree
    parents = _TREES[shape]
    if freeflyer:
        parents = [0] + [p + 1 for p in parents]
        massless = (6, 9) if shape in ("fork", "caterpillar") else ()
        robot = _synthetic_tree(parents, seed=3 + len(parents), massless=massless, freeflyer=True)
    else:
        robot = _synthetic_tree(parents, seed=len(parents), massless=(4,) if shape == "fork" else ())
    return robot.model.to_flat()


# ------------------------------------------------------------------------------------------------ 50-digit evaluation
def _mp_joint_regressor(flat, q, v, a):
    """The same recursion for one sample in mpmath (50 digits), written on 3-vectors: Y as nv x 10 (njoints - 1) mpf."""
    import mpmath as mp
    f, M = mp.mpf, mp.matrix
    n, nv = int(flat["njoints"]), int(flat["nv"])

    def vec(x):
        return M([f(float(t)) for t in x])

    def skew(x):
        return M([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])

    def L(x):
        return M([[x[0], x[1], 0, x[2], 0, 0], [0, x[0], x[1], 0, x[2], 0], [0, 0, 0, x[0], x[1], x[2]]])

    z3 = M([0, 0, 0])
    R, P, S = [None] * n, [None] * n, [None] * n
    Vl, Va, Al, Aa = ([z3.copy() for _ in range(n)] for _ in range(4))
    Al[0] = -vec(flat["gravity"])
    for i in range(1, n):
        jt, iq, iv = int(flat["jtype"][i]), int(flat["idx_q"][i]), int(flat["idx_v"][i])
        ax = vec(flat["axis"][i])
        if jt in (0, 2):
            c, s = (mp.cos(f(float(q[iq]))), mp.sin(f(float(q[iq])))) if jt == 0 else (f(float(q[iq])), f(float(q[iq + 1])))
            K = skew(ax)
            Rj, pj, cols = mp.eye(3) + s * K + (1 - c) * (K * K), z3, [(z3, ax)]
        elif jt == 1:
            Rj, pj, cols = mp.eye(3), ax * f(float(q[iq])), [(ax, z3)]
        else:
            x, y, z, w = (f(float(t)) for t in q[iq + 3:iq + 7])
            Rj = M([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
            pj = vec(q[iq:iq + 3])
            e = [M([1 if r == k else 0 for r in range(3)]) for k in range(3)]
            cols = [(e[k], z3) for k in range(3)] + [(z3, e[k]) for k in range(3)]
        pl = [f(float(t)) for t in flat["placement"][i]]
        Rp, pp = M(3, 3), M(pl[9:])
        for r in range(3):
            for c_ in range(3):
                Rp[r, c_] = pl[3 * r + c_]
        R[i], P[i], S[i] = Rp * Rj, Rp * pj + pp, cols
        par, Rt = int(flat["parents"][i]), (Rp * Rj).T
        vjl, vja, ajl, aja = z3.copy(), z3.copy(), z3.copy(), z3.copy()
        for k, (sl, sa) in enumerate(cols):
            vk, ak = f(float(v[iv + k])), f(float(a[iv + k]))
            vjl, vja, ajl, aja = vjl + sl * vk, vja + sa * vk, ajl + sl * ak, aja + sa * ak
        Vl[i] = vjl + Rt * (Vl[par] - skew(P[i]) * Va[par])
        Va[i] = vja + Rt * Va[par]
        Al[i] = skew(Va[i]) * vjl + skew(Vl[i]) * vja + ajl + Rt * (Al[par] - skew(P[i]) * Aa[par])
        Aa[i] = skew(Va[i]) * vja + aja + Rt * Aa[par]
    Y = [[f(0)] * (10 * (n - 1)) for _ in range(nv)]
    for i in range(n - 1, 0, -1):
        w, dw = Va[i], Aa[i]
        acc = Al[i] + skew(w) * Vl[i]
        Bl, Ba = M(3, 10), M(3, 10)
        Bl[:, 0] = acc
        Bl[:, 1:4] = skew(dw) + skew(w) * skew(w)
        Ba[:, 1:4] = -skew(acc)
        Ba[:, 4:10] = L(dw) + skew(w) * L(w)
        j = i
        while j > 0:
            iv = int(flat["idx_v"][j])
            for k, (sl, sa) in enumerate(S[j]):
                row = sl.T * Bl + sa.T * Ba
                for c_ in range(10):
                    Y[iv + k][10 * (i - 1) + c_] = row[0, c_]
            l2 = R[j] * Bl
            Bl, Ba = l2, R[j] * Ba + skew(P[j]) * l2
            j = int(flat["parents"][j])
    return Y


def _small_tree_flat(freeflyer):
    from test_gpu_parity import _synthetic_tree
    parents = [0, 1, 1, 3, 3, 2] if not freeflyer else [0, 1, 2, 2, 1, 5]
    return _synthetic_tree(parents, seed=21, massless=(3,), freeflyer=freeflyer).model.to_flat()


@pytest.mark.parametrize("regime", ["static", "fast", "bigq"])
@pytest.mark.parametrize("model", ["tree", "freeflyer", "ur10"])
def test_long_double_reference_against_50_digits(model, regime):
    import mpmath as mp
    flat = rx.shipped_flat("ur10") if model == "ur10" else _small_tree_flat(model == "freeflyer")
    N = 8  # samples 5 .. 7 of 8: in bigq the last quarter are the multiples of pi / 2
    q, v, a = rx.inputs(flat, N, regime, seed=3)
    Y, SC = rx.joint_regressor_ld(flat, q, v, a)
    worst = 0.0
    with mp.workdps(50):
        for s in (0, 6, 7):
            Ymp = _mp_joint_regressor(flat, q[s], v[s], a[s])
            for r in range(Y.shape[1]):
                for c in range(Y.shape[2]):
                    hi = float(Y[s, r, c])
                    lo = float(Y[s, r, c] - np.longdouble(hi))
                    d = abs(mp.mpf(hi) + mp.mpf(lo) - Ymp[r][c])
                    if SC[s, r, c] == 0:
                        assert Ymp[r][c] == 0 and Y[s, r, c] == 0, (s, r, c)
                    else:
                        worst = max(worst, float(d / mp.mpf(SC[s, r, c])))
    print("regressor_ld vs 50 digits, %s %s: %.3g (2^-60 = %.3g)" % (model, regime, worst, 2.0 ** -60))
    assert worst <= 2.0 ** -60


# ------------------------------------------------------------------------------------------------- scale: bound, zeros
def _ancestors(flat):
    n = int(flat["njoints"])
    anc = [set() for _ in range(n)]  # anc[k]: k and its ancestors (joint 0 excluded)
    for k in range(1, n):
        anc[k] = {k} | anc[int(flat["parents"][k])]
    return anc


def _known_zero_pattern(flat, param, N, v=None):
    """(must_zero, must_live) masks over the reference layout from the structure the suite knows: a link outside the
    subtree of the row's joint, rotational-inertia slots in force rows and in the rows of prismatic joints, massless links
    and unselected components in wrench mode are zero; inside, the first-moment slots of rotational rows are live (gravity),
    their inertia slots and the first-moment slots of translational rows are live where some joint on the root path of the
    link turns and zero where none does: nowhere below a fixed base with prismatic joints only, and with ``v`` given
    (regime ``one``, v = a = 0 except for one degree of freedom per sample) in the samples where none of them moves."""
    nl = int(flat["njoints"]) - 1
    anc = _ancestors(flat)
    jt = np.asarray(flat["jtype"])
    torque = bool(param["is_joint_torques"])
    nblocks = nl if torque else 6
    zero = np.zeros((nblocks * N, 14 * nl), dtype=bool)
    live = np.zeros_like(zero)
    sel = set(range(nblocks)) if torque else set(rx.ft_rows(param["force_torque"]))
    # turning[i, k]: some joint on the root path of link k + 1 turns in sample i (every sample unless ``v`` is given)
    turning = np.zeros((N, nl), dtype=bool)
    for k in range(1, nl + 1):
        for j in anc[k]:
            if jt[j] == 1:
                continue
            iv = int(flat["idx_v"][j]) + (3 if jt[j] == 3 else 0)
            turning[:, k - 1] |= True if v is None else np.any(v[:, iv:iv + (3 if jt[j] == 3 else 1)] != 0, axis=1)
    for b in range(nblocks):
        r = slice(b * N, (b + 1) * N)
        rotational = (jt[b + 1] != 1) if torque else b >= 3
        for k in range(1, nl + 1):
            c = 14 * (k - 1)
            inside = ((b + 1) in anc[k]) if torque else (b in sel and float(flat["mass"][k]) != 0.0)
            if not inside:
                zero[r, c:c + 10] = True
                continue
            turns = turning[:, k - 1][:, None]
            if rotational:  # first moment: gravity x axis; inertia: dw, w w
                live[r, c + 6:c + 9] = True
                zero[r, c:c + 6], live[r, c:c + 6] = ~turns, turns
            else:  # a translation axis: no inertia entries, first moment from dw, w w alone
                zero[r, c:c + 6] = True
                zero[r, c + 6:c + 9], live[r, c + 6:c + 9] = ~turns, turns
    return zero, live


@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("model", MODELS + ["fork", "fork-ff", "human-FxMz"])
def test_scale_bounds_the_reference_and_vanishes_on_the_structural_zeros(model, regime):
    if model in MODELS:
        flat, param = rx.shipped_flat(model), _param_of(model)
    elif model == "human-FxMz":
        flat, param = rx.shipped_flat("human"), rx.base_param(wrench=True, force_torque=("Fx", "Mz"))
    else:
        flat = _tree_flat("fork", model.endswith("-ff"))
        param = rx.base_param(wrench=model.endswith("-ff"))
    N = 24
    q, v, a = rx.inputs(flat, N, regime, seed=1)
    ref = rx.regressor_ld(flat, q, v, a, param)
    live_cols = ~ref.copied
    # (rotations count 1 in the scale; the float64 placements and quaternions are orthonormal to a few u only)
    assert np.all(ref.S[:, live_cols] * (1 + 2.0 ** -40) >= np.abs(ref.W[:, live_cols]).astype(np.float64))
    assert not ref.S[:, ref.copied].any() and not ref.W[:, ref.copied].any()  # (no flag set: the copied columns are zero)
    zero, live = _known_zero_pattern(flat, param, N, v if regime == "one" else None)
    assert not ref.S[zero].any(), "scale on a structural zero"
    assert np.all(ref.S[live] > 0), "no scale on a live entry"
    assert not ref.W[ref.S == 0].any()


# ---------------------------------------------------------------------------------------------------- oracles measured
def _oracle_cases():
    from test_gpu_parity import _TREES
    cases = [(m, m) for m in MODELS]
    for shape in sorted(_TREES):
        cases += [(shape, shape), (shape + "-ff", shape)]
    return cases


@pytest.mark.parametrize("label,what", _oracle_cases())
def test_oracles_within_scale(label, what, oracle_lib):
    """entry_ratio of both float64 oracles against the long-double reference, every regime, N = 200: at most C_ORACLE, the
    recorded maximum of this very measurement (a larger value means the constant, and with it C_TOL, is to be derived
    again), and 8 times it within C_TOL; exact zeros where the scale is zero, copied columns equal."""
    if label in MODELS:
        flat = rx.shipped_flat(label)
        param = _param_of(label, friction=True, inertia=True, offset=True)
    else:
        flat = _tree_flat(what, label.endswith("-ff"))
        param = rx.base_param(wrench=label.endswith("-ff"), friction=True, inertia=True, offset=True)
    coupling = label == "tx40"
    om = oracle_lib.OracleModel(flat)
    mode, fl, ft = oracle_lib.param_flags(param, coupling)
    worst = 0.0
    for regime in rx.REGIMES:
        q, v, a = rx.inputs(flat, N_ORACLE, regime)
        ref = rx.regressor_ld(flat, q, v, a, param, coupling)
        W_c = om.build_regressor_basic(q, v, a, mode, fl, ft)
        W_np = oracle_np.build_regressor_basic(flat, q, v, a, param)
        if coupling:
            W_np = oracle_np.add_coupling_TX40(W_np, N_ORACLE, v, a)
        for name, W in (("C", W_c), ("NumPy", W_np)):
            r = rx.entry_ratio(W, ref.W, ref.S, ref.copied)
            print("oracle %-5s %-14s %-7s ratio %.2f" % (name, label, regime, r.ratio))
            assert r.zeros_ok and r.copied_ok, (name, label, regime)
            worst = max(worst, r.ratio)
    assert worst <= rx.C_ORACLE and 8 * worst <= rx.C_TOL, (label, worst)


def test_tolerance_constants():
    assert 8 * rx.C_ORACLE <= rx.C_TOL < 16 * rx.C_ORACLE and np.log2(rx.C_TOL) == int(np.log2(rx.C_TOL))


# ----------------------------------------------------------------------------------------------------------- tightness
@pytest.mark.parametrize("regime", rx.REGIMES)
@pytest.mark.parametrize("model", MODELS)
def test_scale_hides_nothing(model, regime):
    """Per (row block, link, slot group) with S != 0: rms S / rms |W_ld|.  Median <= 64 and at most a quarter of the groups
    above 2^8 (exact-zero groups included) in every model and regime: the scale is the size of the entries except where a
    term vanishes geometrically."""
    flat = rx.shipped_flat(model)
    N = 64
    q, v, a = rx.inputs(flat, N, regime, seed=2)
    ref = rx.regressor_ld(flat, q, v, a, _param_of(model))
    t, labels = rx.group_tightness(ref.W, ref.S, N, int(flat["njoints"]) - 1)
    above = t > 2.0 ** 8
    print("tightness %-6s %-7s median %.1f, %d of %d groups above 2^8 (%d exactly zero), largest finite %.3g" % (
        model, regime, np.median(t), above.sum(), len(t), np.isinf(t).sum(), t[np.isfinite(t)].max()))
    assert np.median(t) <= 64
    assert above.sum() <= 0.25 * len(t)


# ------------------------------------------------------------------------------------------------------ planted errors
def _inertia_cols(k):
    return 14 * k + np.arange(6)


@pytest.mark.parametrize("model", ["ur10", "tiago", "talos"])
def test_planted_errors(model):
    """Four errors planted into the float64 rounding of W_ld: each passes the norm-wise check with a factor >= 2 to spare
    and fails the entry-wise one by a factor >= 4."""
    flat = rx.shipped_flat(model)
    param = _param_of(model)
    nl = int(flat["njoints"]) - 1
    N = 32
    seen = []

    def verdict(name, W_bad, ref):
        W64 = np.asarray(ref.W, dtype=np.float64)
        assert rx.entry_ratio(W64, ref.W, ref.S, ref.copied).ratio <= 1.0  # (the rounding itself: half an ulp of |W| <= u S)
        old = rx.old_normwise(W_bad, W64)
        new = rx.entry_ratio(W_bad, ref.W, ref.S, ref.copied).ratio
        print("planted %-22s %-6s old check %.3g of its tolerance, new ratio %.3g (C_TOL %g)" % (name, model, old, new, rx.C_TOL))
        assert old <= 0.5, (name, old)
        assert new >= 4 * rx.C_TOL, (name, new)
        seen.append(name)

    # (i) w x (w x J_l) dropped from the first-moment slots, slow trajectory.  Dropped everywhere the term is just within
    # reach of the norm-wise check (2.2 .. 4.4 of its tolerance on these models: a dozen joints at 2e-6 rad/s and a lever of
    # 1 m), so it is dropped where it is below a quarter of that tolerance -- most entries -- and kept elsewhere.
    q, v, a = rx.inputs(flat, N, "static", seed=5)
    ref = rx.regressor_ld(flat, q, v, a, param)
    Y_bad, _ = rx.joint_regressor_ld(flat, q, v, a, drop_centripetal=True)
    W_all = np.asarray(rx.stack(flat, Y_bad, param, N), dtype=np.float64)
    W64 = np.asarray(ref.W, dtype=np.float64)
    term = np.abs(W_all - W64)
    small = term <= 0.25e-12 * np.abs(W64).max()
    print("planted (i) everywhere: old check %.3g of its tolerance; dropped in %d of %d entries that have the term" % (
        rx.old_normwise(W_all, W64), (small & (term > 0)).sum(), (term > 0).sum()))
    assert (small & (term > 0)).sum() >= 0.5 * (term > 0).sum()
    verdict("(i) centripetal term", np.where(small, W_all, W64), ref)
    # (ii) inertia columns of one link in one row block times 1 + 1e-6, slow trajectory
    W_bad = np.asarray(ref.W, dtype=np.float64)
    # (the slowest link: the first one, with one joint above it -- further out dw grows with every joint and 1e-6 of it
    # comes within reach of the norm-wise check: 1.3 .. 1.8 of its tolerance at the last link of these models)
    b = k = 0
    if not param["is_joint_torques"]:
        b = 3
    assert ref.S[b * N:(b + 1) * N][:, _inertia_cols(k)].all()
    W_bad[b * N:(b + 1) * N, _inertia_cols(k)] *= 1 + 1e-6
    verdict("(ii) inertia 1 + 1e-6", W_bad, ref)
    # (iii) a sincos that loses a few bits: the angle of one revolute joint off by 2 * 2^-44 relative
    q, v, a = rx.inputs(flat, N, "unit", seed=5)
    ref = rx.regressor_ld(flat, q, v, a, param)
    rev = [i for i in range(1, nl + 1) if int(flat["jtype"][i]) == 0]
    iq = int(flat["idx_q"][rev[len(rev) // 2]])
    q_bad = q.copy()
    q_bad[:, iq] *= 1 + 2.0 * 2.0 ** -44
    W_bad = np.asarray(rx.regressor_ld(flat, q_bad, v, a, param).W, dtype=np.float64)
    verdict("(iii) angle 2 * 2^-44", W_bad, ref)
    # (iv) the nearly-at-rest quarter of a mixed wave gets zeros in the inertia slots
    q, v, a = rx.inputs(flat, N, "mixed", seed=5)
    ref = rx.regressor_ld(flat, q, v, a, param)
    W_bad = np.asarray(ref.W, dtype=np.float64)
    rest = np.flatnonzero(np.arange(N) % 4 == 1)
    rows = (np.arange(len(W_bad) // N)[:, None] * N + rest[None, :]).reshape(-1)
    W_bad[np.ix_(rows, np.flatnonzero(np.arange(W_bad.shape[1]) % 14 < 6))] = 0.0
    verdict("(iv) rest quarter zeroed", W_bad, ref)
    assert len(seen) == 4


def test_exact_conditions_reject():
    flat = rx.shipped_flat("ur10")
    param = rx.base_param(friction=True, inertia=True, offset=True)
    N = 12
    q, v, a = rx.inputs(flat, N, "one", seed=4)
    ref = rx.regressor_ld(flat, q, v, a, param)
    W = np.asarray(ref.W, dtype=np.float64)
    ok = rx.entry_ratio(W, ref.W, ref.S, ref.copied)
    assert ok.zeros_ok and ok.copied_ok and ok.ratio <= 1.0
    Wm = W.copy()
    Wm[W == 0] = -0.0  # a negative zero is a zero
    ok = rx.entry_ratio(Wm, ref.W, ref.S, ref.copied)
    assert ok.zeros_ok and ok.copied_ok
    # fs = +1 where v == 0: row block 1, sample 0 (only joint 0 moves there)
    assert v[0, 1] == 0.0 and W[1 * N + 0, 14 * 1 + 12] == 0.0
    bad = W.copy()
    bad[1 * N + 0, 14 * 1 + 12] = 1.0
    assert not rx.entry_ratio(bad, ref.W, ref.S, ref.copied).copied_ok
    # 1e-300 in a structural zero (row block 5, link 0: outside the subtree)
    assert ref.S[5 * N, 0] == 0.0
    bad = W.copy()
    bad[5 * N, 0] = 1e-300
    r = rx.entry_ratio(bad, ref.W, ref.S, ref.copied)
    assert not r.zeros_ok and r.copied_ok
    # one ulp in an Ia entry
    bad = W.copy()
    bad[2 * N + 2, 14 * 2 + 10] = np.nextafter(bad[2 * N + 2, 14 * 2 + 10], np.inf)
    assert a[2, 2] != 0.0
    r = rx.entry_ratio(bad, ref.W, ref.S, ref.copied)
    assert r.zeros_ok and not r.copied_ok
    with pytest.raises(AssertionError, match="copied columns"):
        rx.assert_entrywise(bad, ref)
    # a NaN is no pass
    bad = W.copy()
    bad[0, 0] = np.nan
    assert not rx.entry_ratio(bad, ref.W, ref.S, ref.copied).ratio <= rx.C_TOL
