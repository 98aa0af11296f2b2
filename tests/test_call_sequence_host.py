"""CPU suite for the call-sequence and ABI-entry tests (tests/test_call_sequences.py, tests/test_abi_entries_exact.py): what
they assert on the GPU is only as good as their inputs and metrics, and both can be examined without a device.

* every step's input stays inside what its reference can certify (the cond^2 2^-64 <= 0.1 cond u guard of
  test_qr_graded._check, rows >= 2 nc for the full-rank steps, true pivots >= 3 tol_qr under exact dependencies);
* the three ways carried state can go wrong -- a stale hint, a stale entry of a stream buffer, a level-0 triangle lost to
  a shared slot -- are emulated on the CPU and REJECTED by the metric at the tolerance the GPU test uses, while the same
  computation without the plant passes;
* the flat-model derivation of the shape and layout queries reproduces what tests/golden/cfg*.json records;
* worker and parent read one step table.
"""
import numpy as np
import pytest

import call_sequence_common as cs
import qr_graded_common as qg
from test_qr_graded import _check


def _rp(*_):
    pass


def _qr_r(A):
    """Upper-triangular factor of A by LAPACK's Householder QR, square (zero rows appended when A is short)."""
    R = np.linalg.qr(A, mode="r")
    nc = A.shape[1]
    return np.triu(np.vstack([R, np.zeros((nc - R.shape[0], nc))]) if R.shape[0] < nc else R)


def _step(family, tag):
    return {s.tag: s for s in cs.steps(family)}[tag]


# ------------------------------------------------------------------------------------------------------- one step table
def test_worker_and_parent_share_one_table():
    import call_sequence_worker as worker
    import test_call_sequences as parent
    assert sorted(worker.RUN) == sorted(parent.CHECK), "the worker runs ops the parent does not judge, or the reverse"
    assert sorted(cs.STATE) == sorted(cs.FAMILIES)
    for family in cs.FAMILIES:
        table = cs.steps(family)
        assert cs.steps(family) is table, "worker and parent would build different inputs"
        tags = [s.tag for s in table]
        assert len(set(tags)) == len(tags)
        by = {s.tag: s for s in table}
        for s in table:
            assert s.op in worker.RUN and s.op in parent.CHECK, "%s: op %s" % (s.tag, s.op)
            if s.repeat_of is not None:
                first = by[s.repeat_of]
                assert first.op == s.op and first.repeat_of is None
                # a repeat is the SAME call: the same input objects (what differs, if anything, is a setting under test)
                same = [k for k in s.args if s.args[k] is first.args[k] or np.array_equal(s.args[k], first.args[k])]
                assert len(same) >= len(s.args) - 1, "%s does not repeat %s" % (s.tag, s.repeat_of)
    # every family has at least one repeat: that is what the family is for
    assert all(any(s.repeat_of for s in cs.steps(f)) or f == "settings" for f in cs.FAMILIES)


def test_sequences_cover_the_states_they_name():
    """The shapes that make a slot grow or a cache change hands are in the tables (derived from the launch rules)."""
    h = {s.tag: s.args for s in cs.steps("hints")}
    s1, s2, s3 = h["02_S1"]["h"], h["03_S2_descending"]["h"], h["07_S3_slot_grows"]["h"]
    assert (s1.rows, s1.nfirst) == (s2.rows, s2.nfirst) and not np.array_equal(s1.first, s2.first)  # same key but the list
    assert np.all(np.diff(s1.first) > 0) and np.all(np.diff(s2.first) < 0)
    assert h["04_S1_again"]["h"] is s1 and h["05_S1_cache_hit"]["h"] is s1
    assert (s3.rows + 63) // 64 + 1 > 1.25 * ((s1.rows + 63) // 64 + 1)  # kWsTileHint grows (workspace() adds 25 %)
    d1, d9 = h["01_dense_640"]["h"], h["09_dense_192000_zero_hint_grows"]["h"]
    assert (d9.rows + 63) // 64 > 1.25 * ((max(d1.rows, s3.rows) + 63) // 64 + 1)  # kWsZeroHint grows
    d6 = h["06_dense_600_no_zeros"]["h"]
    assert d6.rows == s1.rows and np.all(d6.M() != 0)  # an inherited hint would drop entries
    s13 = h["13_S_79_tau_other_instantiation"]["h"]
    assert 64 < s13.nc <= 80 and s1.nc <= 64 and s13.first.max() == s13.n
    m = [s.args["g"] for s in cs.steps("merges")]
    assert {(g.nc <= 64) for g in m if g.nc <= 80} == {True, False}  # both instantiations of the stream kernel
    assert any(g.nc > 80 for g in m) and any(g.count >= 4500 for g in m)
    w = {s.tag: s.args for s in cs.steps("wide_filter")}
    f1, t1 = w["02_filtfilt_large"], w["01_tsqr_4000x96"]["h"]
    work = (f1["x"].shape[0] // f1["nblocks"] + 2 * f1["padlen"]) * f1["nblocks"] * f1["x"].shape[1]
    nch = (t1.nc + 15) // 16
    assert work > 1.25 * 256 * (nch * (nch + 1) // 2) * (t1.rows // (8 * t1.nc))  # the filter grows the blocked kernel's slot


# ---------------------------------------------------------------------------------------- inputs the references certify
@pytest.mark.parametrize("family", cs.FAMILIES)
def test_family_inputs_are_certifiable(family):
    qg.check_longdouble()
    for step in cs.steps(family):
        c = cs.certify(step)
        assert c.get("guard", True), "%s: cond %.3g is too large for the long-double reference" % (step.tag, c.get("cond"))
        assert c.get("tall", True) in (True, None), "%s: a full-rank step with rows < 2 nc" % step.tag
        if "pivot" in c:
            assert c["pivot"] >= 3 * cs.TOL_QR, "%s: true pivot %.3g within 3x of tol_qr" % (step.tag, c["pivot"])


@pytest.mark.parametrize("case", cs.STRUCTURED_CASES, ids=[c[0] for c in cs.STRUCTURED_CASES])
def test_structured_cases_are_true_hints_and_certifiable(case):
    """In block b the gathered columns < first[b] are exactly zero, every row carries +-2^10 at column first[b], and LAPACK's
    QR of the same input passes the metric the GPU test applies (so a failure there is the kernel's)."""
    h = cs.structured_case(case)
    Mg = h.Mw[:, h.cols]
    f = np.repeat(h.first.astype(np.int64), h.rb)
    assert not Mg[np.arange(h.n)[None, :] < f[:, None]].any()
    r = np.flatnonzero(f < h.n)
    assert np.all(np.abs(Mg[r, f[r]]) == qg.INT_MAX)
    assert h.mt is None or np.all(h.mt != 0)
    _check(_qr_r(h.gathered()), h.gram(), _rp, case[0], forward=h.forward())


def test_structured_cases_reach_every_path():
    cases = [cs.structured_case(c) for c in cs.STRUCTURED_CASES]
    assert {h.nc for h in cases} >= {1, 16, 17, 64, 65, 80, 81}
    assert {h.rb for h in cases} >= {1, 37, 64, 100, 640} and {h.nfirst for h in cases} >= {1, 6, 7, 640}
    assert any(h.rows < 64 for h in cases) and any(h.rows % 64 for h in cases)
    assert any(np.all(np.diff(h.first) < 0) for h in cases) and any(h.first.max() == h.n and h.mt is not None for h in cases)
    assert any(h.wexp is not None and len(h.wexp) != h.nfirst for h in cases)
    for nc_lo, nc_hi in ((1, 64), (65, 80)):  # both instantiations with and without tau
        assert {h.mt is None for h in cases if nc_lo <= h.nc <= nc_hi} == {True, False}


# ------------------------------------------------------------------------------------------------------ planted failures
def test_stale_hint_is_rejected():
    """S2 factored under S1's hint (the entries in front of the WRONG first[] never read): the metric rejects it."""
    s1, s2 = _step("hints", "02_S1").args["h"], _step("hints", "03_S2_descending").args["h"]
    A, G = s2.gathered(), s2.gram()
    _check(_qr_r(A), G, _rp, "unplanted", forward=s2.forward())
    stale = np.repeat(s1.first.astype(np.int64), s1.rb)
    A_bad = np.where(np.arange(s2.nc)[None, :] < stale[:, None], 0.0, A)
    assert np.count_nonzero(A_bad != A) > 0
    with pytest.raises(AssertionError, match="backward"):
        _check(_qr_r(A_bad), G, _rp, "stale_hint", forward=s2.forward())


def test_stale_stream_entry_is_rejected():
    """One row of one child triangle replaced by the row the previous launch left there: the merge metric rejects it."""
    prev, cur = _step("merges", "02_50x300").args["g"], _step("merges", "03_50x17").args["g"]
    assert prev.nc == cur.nc
    A, G = cur.A(), cur.gram()
    _check(_qr_r(A), G, _rp, "unplanted")
    nc, t, row = cur.nc, 5, 3
    A_bad = A.copy()
    A_bad[t * nc + row] = prev.A()[t * nc + row]
    with pytest.raises(AssertionError, match="backward"):
        _check(_qr_r(A_bad), G, _rp, "stale_stream_entry")


def test_lost_level0_triangle_is_rejected():
    """A two-level TSQR whose level-0 triangle number 3 was overwritten with zeros (another user of its slot)."""
    h = _step("structured", "04_tsqr_workspace_triangles").args["h"]
    A, G = h.gathered(), h.gram()
    tris = [_qr_r(part) for part in np.array_split(A, 8)]
    _check(_qr_r(np.vstack(tris)), G, _rp, "unplanted", forward=h.forward())
    tris[3] = np.zeros_like(tris[3])
    with pytest.raises(AssertionError, match="backward"):
        _check(_qr_r(np.vstack(tris)), G, _rp, "lost_triangle", forward=h.forward())


# ----------------------------------------------------------------------------------- the derivation of the layout queries
@pytest.mark.parametrize("cfg", ["cfg1_tx40", "cfg2_ur10", "cfg3_tiago", "cfg4_talos", "cfg5_human"])
def test_layout_derivation_reproduces_the_golden_shapes(cfg):
    from conftest import Golden
    from figaroh_plus_amd import _lib
    from figaroh_plus_amd.tools.regressor import regressor_flags
    from test_abi_entries_exact import derive_layout
    g = Golden(cfg)
    flat, dims = g.flat(), g.meta["dims"]
    mode, flags, ft = regressor_flags(g.param, g.coupling)
    rps, ncols, pos, nlive, ldf = derive_layout(flat, mode, flags, ft)
    assert ncols == dims["cols"] == len(g.meta["names_std"])
    assert rps == (dims["nv"] if g.param["is_joint_torques"] else 6)
    assert g["tau"].shape[0] == rps * g["q_big"].shape[0]
    bodies = [j for j in g.meta["id_inertias"] if j >= 1]
    assert bodies == (np.flatnonzero(np.asarray(flat["mass"], dtype=float)[1:] != 0) + 1).tolist()
    if mode == _lib.MODE_EXT_WRENCH:
        extras = bool(flags & 7)
        assert pos is not None and nlive == (dims["njoints"] - 1 if extras else len(bodies))
        assert np.flatnonzero(pos >= 0).tolist() == (list(range(dims["njoints"] - 1)) if extras else [j - 1 for j in bodies])
        assert ldf == (0 if extras else 16 * -(-len(bodies) // 4))
    else:
        assert pos is None and ldf == 0
