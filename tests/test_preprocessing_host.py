"""Host suite (no GPU): the reference of the bit-exact preprocessing tests is itself right, and its case table reaches
what it claims.

test_preprocessing_exact.py compares figh_filtfilt_cols bit for bit with tests/preprocessing_common.filtfilt_ref, a
float64 NumPy emulation of the kernel's recurrences.  Here that emulation is compared bit for bit with scipy.signal over
the same case table, the float64 / long-double gap of every design is bounded (an unstable design would make a bit
comparison meaningless), compact_rows_ref is checked against hand-written expectations, and the table is shown to reach
every kernel instantiation and every branch of the kernel's tiling.

Measured here (SciPy 1.15.3): every design of the table is bit-equal to SciPy; the float64 / long-double gap is at most
1.7e-8 of the sequence maximum (Butterworth order 8, Wn = 0.05).
"""
import functools

import numpy as np
import pytest

import preprocessing_common as pc

GUARD = 1.0e-6  # float64 against long-double emulation, relative to max |sequence|: a guard on the INPUTS, no kernel tolerance


@functools.lru_cache(maxsize=None)
def _cases(di):
    """[(case, x, float64 emulation)] of design number di, computed once for the tests of this module."""
    form, b, a, zi, padlen = pc.design(*pc.DESIGNS[di])
    out = []
    for case in pc.cross_cases(di):
        L, cols, nblocks, q = case[:4]
        x = pc.make_signal(L, cols, nblocks, 1000 * di + L)
        out.append((case, x, pc.filtfilt_ref(form, b, a, zi, padlen, q, x, nblocks)))
    return out


@pytest.mark.parametrize("di", range(len(pc.DESIGNS)), ids=[pc.design_id(d) for d in pc.DESIGNS])
def test_emulation_is_bit_equal_to_scipy(di):
    """filtfilt_ref(float64) == signal.sosfiltfilt / signal.filtfilt(padtype="odd", padlen=...) under array_equal, at
    every length of the table (L = padlen + 1 and the padlen = 0 designs included)."""
    kind, n, _ = pc.DESIGNS[di]
    padlen = pc.design(*pc.DESIGNS[di])[4]
    assert pc.lengths(padlen)[0] == padlen + 1
    for (L, cols, nblocks, q, _, _), x, ref in _cases(di):
        sp = pc.scipy_ref(kind, n, padlen, q, x, nblocks)
        assert ref.shape == sp.shape == (-(-L // q) * nblocks, cols)
        same = np.array_equal(ref, sp)
        if pc.design_id(pc.DESIGNS[di]) in pc.SCIPY_DISAGREES:
            continue
        assert same, "%s L=%d cols=%d nblocks=%d q=%d: first difference at %s" % (
            pc.design_id(pc.DESIGNS[di]), L, cols, nblocks, q, np.argwhere(ref != sp)[0])


@pytest.mark.parametrize("di", range(len(pc.DESIGNS)), ids=[pc.design_id(d) for d in pc.DESIGNS])
def test_designs_are_stable_enough_for_bit_comparison(di, record_property):
    """Per sequence, the float64 and the long-double emulation agree within 1e-6 of the sequence maximum."""
    assert np.finfo(np.longdouble).nmant >= 63, "the guard needs an 80-bit (or wider) long double"
    form, b, a, zi, padlen = pc.design(*pc.DESIGNS[di])
    worst = 0.0
    for (L, cols, nblocks, q, _, _), x, ref in _cases(di):
        ld = pc.filtfilt_ref(form, b, a, zi, padlen, q, x, nblocks, dtype=np.longdouble)
        Lout = ref.shape[0] // nblocks
        for k in range(nblocks):
            r, l = ref[k * Lout:(k + 1) * Lout], ld[k * Lout:(k + 1) * Lout]
            gap = np.abs(r - l).max(axis=0) / np.abs(l).max(axis=0)
            worst = max(worst, float(gap.max()))
            assert (gap <= GUARD).all(), (pc.design_id(pc.DESIGNS[di]), L, k, int(gap.argmax()), float(gap.max()))
    record_property("float64_vs_longdouble", "%.2e" % worst)


def test_case_table_reaches_every_instantiation():
    """Every case label of the two switch statements of figh_filtfilt_cols, and both default arms (the generic run-time
    loops: 7-8 sections, orders 7 and 9-16).  The labels are data here, not parsed from the source."""
    sos_labels, tf_labels = (1, 2, 3, 4, 5, 6), (1, 2, 3, 4, 5, 6, 8)
    assert pc.SOS_CASE_LABELS == sos_labels and pc.TF_CASE_LABELS == tf_labels
    want = {(0, c) for c in sos_labels} | {(0, "default")} | {(1, c) for c in tf_labels} | {(1, "default")}
    assert len(want) == 15 and set(pc.ALL_INSTANTIATIONS) == want
    got = {pc.instantiation(kind, n) for kind, n, _ in pc.DESIGNS}
    assert got == want
    # the default arms see both ends of what the API accepts
    assert {n for kind, n, _ in pc.DESIGNS if pc.instantiation(kind, n) == (0, "default")} == {7, 8}
    assert {n for kind, n, _ in pc.DESIGNS if pc.instantiation(kind, n) == (1, "default")} == {7} | set(range(9, 17))
    assert [pc.design(*d)[4] for d in pc.DESIGNS[:8]] == [9, 15, 21, 27, 33, 39, 45, 51]
    assert [pc.design(*d)[4] for d in pc.DESIGNS[8:24]] == [3 * o for o in range(1, 17)]


def _tile_events(L, edge):
    """What the kernel's two loops do for a length: branch taken per forward tile and the size of the ragged tile."""
    Lext, ev = L + 2 * edge, set()
    for n0 in range(0, Lext, pc.TB):
        ev.add("interior" if n0 >= edge and n0 + pc.TB <= edge + L else "extension")
    ev.add("last_tile_%d" % ((Lext - 1) % pc.TB + 1))
    if not any(n0 >= edge and n0 + pc.TB <= edge + L for n0 in range(0, Lext, pc.TB)):
        ev.add("no_interior")
    if Lext < pc.TB:
        ev.add("single_partial_tile")
    return ev


def test_lengths_reach_every_tiling_branch():
    """For every design: a full, a 1-sample and a 31-sample ragged tile, interior tiles and a length without any; for the
    short edges a sequence shorter than one tile; the tile-aligned edges put an interior tile right at the edge."""
    for d in pc.DESIGNS:
        edge = pc.design(*d)[4]
        Ls = pc.lengths(edge)
        assert all(L > edge for L in Ls) and len(set(Ls)) == len(Ls) and max(Ls) <= 300
        ev = set().union(*[_tile_events(L, edge) for L in Ls])
        assert {"interior", "extension", "last_tile_32", "last_tile_1", "last_tile_31"} <= ev, (d, ev)
        # (from these edges on even the minimum length edge + 1 holds a whole tile of plain samples)
        assert ("no_interior" in ev) == (edge not in (32, 48, 51, 64)), (d, ev)
        if 3 * edge < pc.TB - 2:
            assert "single_partial_tile" in ev, d
    for di, d in enumerate(pc.DESIGNS):  # the spread columns: every design sees padded and tight leading dimensions
        cases = pc.cross_cases(di)
        assert {c[4] - c[1] for c in cases} == {0, 3} and {c[5] - c[1] for c in cases} == {0, 2}
    seen = {(c[1], c[2]) for di in range(len(pc.DESIGNS)) for c in pc.cross_cases(di)}
    assert seen == set(pc.SEQ_COUNTS)
    assert {c[3] for di in range(len(pc.DESIGNS)) for c in pc.cross_cases(di)} == set(pc.Q_CYCLE)


def test_odd_ext_by_hand():
    x = np.array([[1.0], [2.0], [4.0], [8.0]])
    assert np.array_equal(pc.odd_ext(x, 0), x)
    assert np.array_equal(pc.odd_ext(x, 2)[:, 0], [-2.0, 0.0, 1.0, 2.0, 4.0, 8.0, 12.0, 14.0])
    assert np.array_equal(pc.odd_ext(x, 3)[:, 0], [-6.0, -2.0, 0.0, 1.0, 2.0, 4.0, 8.0, 12.0, 14.0, 15.0])


def test_compact_rows_ref_by_hand():
    """Three tiny inputs with the expectations written out: a key equal to the threshold is kept (either sign), the next
    double towards zero is dropped, -0.0 and 0.0 pass a zero threshold, a NaN key never does."""
    W = np.array([[1.0, -2.0, 9.0], [0.5, 3.0, 9.0], [-1.0, 4.0, 9.0]])
    Wk, tk, n = pc.compact_rows_ref(W, 2, 0, 1.0, np.array([10.0, 20.0, 30.0]))
    assert n == 2 and np.array_equal(Wk, [[1.0, -2.0], [-1.0, 4.0]]) and np.array_equal(tk, [10.0, 30.0])
    thr = 0.6
    W = np.array([[0.0, np.nextafter(thr, 0.0)], [1.0, -thr], [2.0, np.nan], [3.0, thr], [4.0, -np.nextafter(thr, 0.0)]])
    Wk, tk, n = pc.compact_rows_ref(W, 2, 1, thr)
    assert n == 2 and tk is None and np.array_equal(Wk, [[1.0, -thr], [3.0, thr]])
    W = np.array([[-0.0], [0.0], [np.nan], [-np.inf]])
    Wk, tk, n = pc.compact_rows_ref(W, 1, 0, 0.0, np.arange(4.0))
    assert n == 3 and np.array_equal(tk, [0.0, 1.0, 3.0]) and np.signbit(Wk[0, 0]) and not np.signbit(Wk[1, 0])
    Wk, tk, n = pc.compact_rows_ref(np.ones((3, 2)), 2, 1, 2.0, np.ones(3))  # none kept
    assert n == 0 and Wk.shape == (0, 2) and tk.shape == (0,)


def test_compaction_sizes_reach_the_multi_count_scan():
    """compact_scan_kernel takes per = ceil(groups / 1024) counts per thread: the sizes of the GPU module reach per = 1
    at its upper edge, per = 2 and per = 3 with threads whose range starts past the last group."""
    assert [pc.scan_per(r) for r in pc.COMPACT_ROWS] == [1, 1, 1, 1, 2, 3]
    for rows in pc.COMPACT_ROWS[-2:]:
        ngroups, per = (rows + 63) // 64, pc.scan_per(rows)
        assert 1023 * per > ngroups  # threads whose range starts past the last group (lo > ngroups, hi = ngroups)
    assert ((pc.COMPACT_ROWS[-2] + 63) // 64) % 2 == 1  # per = 2 with a last range of one group
