"""GPU suite: the real-data preprocessing kernels bit for bit.

figh_filtfilt_cols (zero-phase IIR filtering + decimation), figh_compact_rows (row rejection), figh_place_block and
figh_gather_cols (strided copies) and their caller _decimate_device run on either side of every real-data
identification.  None of them has a rounding of its own to hide behind: the filter uses __dmul_rn / __dadd_rn /
__dsub_rn in SciPy's operation order, the others move doubles (place_block: one multiplication).  So every assertion
here is np.array_equal, sequence by sequence, against tests/preprocessing_common.py: a float64 NumPy emulation of the
recurrences with one statement per rounding (the primary oracle; test_preprocessing_host.py ties it to SciPy bit for
bit on the CPU and explains why a long-double reference would be the wrong oracle), and scipy.signal itself as the
secondary one.

The case table (preprocessing_common.DESIGNS x lengths) launches all 15 instantiations of filtfilt_cols_kernel -- 1-6
sections and orders 1-6, 8 as compile-time forms, both generic run-time-loop kernels (7-8 sections, orders 7, 9-16) --
at lengths placed on the branch boundaries of its 32-sample tiling; every test records the instantiation it reached.
The compaction cases reach two and three counts per thread in compact_scan_kernel.

Wall time of the whole module on an MI355X machine: 2.5 s for its 89 tests (the NumPy emulation is the slow part; the
slowest test, the first one, takes 0.8 s with the library's start-up).
"""
import numpy as np
import pytest

import preprocessing_common as pc

pytestmark = pytest.mark.gpu

SENT = -7.25e77  # pre-fill of every output buffer: finite, and nothing here computes it


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _untouched(a):
    """Every element still holds the sentinel, bit for bit."""
    return bool((_bits(a) == _bits(np.float64(SENT))).all())


def _padded(x, ld, fill=np.nan):
    """x in a buffer of leading dimension ld, the padding columns filled (NaN: reading them would poison the result)."""
    out = np.full((x.shape[0], ld), fill)
    out[:, :x.shape[1]] = x
    return out


def _device_filtfilt(lib, form, b, a, zi, padlen, q, x, nblocks, ldx=None, ldy=None, spare=3, finite=True):
    """figh_filtfilt_cols on x (nblocks * L, cols) with the given leading dimensions; checks the returned row count, the
    sentinel in the output padding and in the spare rows, and that no NaN came out.  Returns (rows_out, cols)."""
    rows, cols = x.shape
    ldx, ldy = ldx or cols, ldy or cols
    Lout = -(-(rows // nblocks) // q)
    d_x = lib.DeviceArray.from_host(_padded(x, ldx).reshape(-1))
    d_y = lib.DeviceArray.from_host(np.full((Lout * nblocks + spare) * ldy, SENT))
    got = lib.filtfilt_cols(d_x, rows, cols, ldx, nblocks, form, b, a, zi, padlen, q, d_y, ldy)
    Y = d_y.to_host().reshape(-1, ldy)
    assert got == Lout * nblocks, "returned row count %d, expected %d" % (got, Lout * nblocks)
    assert _untouched(Y[got:]), "spare rows behind the result were written"
    assert _untouched(Y[:got, cols:]), "padding columns of the result (ldy > cols) were written"
    y = Y[:got, :cols].copy()
    if finite:
        assert not np.isnan(y).any(), "NaN in the result (input padding read, or an element never written)"
        assert not (_bits(y) == _bits(np.float64(SENT))).any(), "an element of the result was never written"
    return y


def _assert_sequences_equal(dev, ref, nblocks, what, equal_nan=False, skip=()):
    """array_equal per (block, column) sequence; the message names the block, the column and the first differing sample."""
    assert dev.shape == ref.shape, "%s: shape %s, reference %s" % (what, dev.shape, ref.shape)
    Lout = dev.shape[0] // nblocks
    for blk in range(nblocks):
        for col in range(dev.shape[1]):
            if (blk, col) in skip:
                continue
            d, r = dev[blk * Lout:(blk + 1) * Lout, col], ref[blk * Lout:(blk + 1) * Lout, col]
            if not np.array_equal(d, r, equal_nan=equal_nan):
                bad = d != r
                if equal_nan:
                    bad &= ~(np.isnan(d) & np.isnan(r))
                m = int(np.argmax(bad))
                raise AssertionError("%s: block %d column %d differs first at kept sample %d of %d: device %r (%s), "
                                     "reference %r (%s); %d samples differ" % (
                                         what, blk, col, m, Lout, d[m], float(d[m]).hex(), r[m], float(r[m]).hex(),
                                         int(bad.sum())))


def _check_case(lib, d, L, cols, nblocks, q, ldx, ldy, seed):
    kind, n, _ = d
    form, b, a, zi, padlen = pc.design(*d)
    x = pc.make_signal(L, cols, nblocks, seed)
    what = "%s L=%d cols=%d nblocks=%d q=%d ldx=%d ldy=%d" % (pc.design_id(d), L, cols, nblocks, q, ldx, ldy)
    dev = _device_filtfilt(lib, form, b, a, zi, padlen, q, x, nblocks, ldx, ldy)
    assert dev.shape[0] == -(-L // q) * nblocks
    _assert_sequences_equal(dev, pc.filtfilt_ref(form, b, a, zi, padlen, q, x, nblocks), nblocks, what + " (emulation)")
    if pc.design_id(d) not in pc.SCIPY_DISAGREES:
        _assert_sequences_equal(dev, pc.scipy_ref(kind, n, padlen, q, x, nblocks), nblocks, what + " (SciPy)")


def _record_instantiation(record_property, d):
    form, label = pc.instantiation(d[0], d[1])
    record_property("instantiation", "form=%d %s=%d: %s" % (form, "nsec" if form == 0 else "order", d[1],
                                                              "case %s" % label if label != "default" else "default (NS = 0)"))


# ------------------------------------------------------------------------------------------------- figh_filtfilt_cols
@pytest.mark.parametrize("di", range(len(pc.DESIGNS)), ids=[pc.design_id(d) for d in pc.DESIGNS])
def test_filtfilt_every_design_at_every_tile_boundary(lib, di, record_property):
    """Every design x every length of preprocessing_common.lengths (edge + 1; the extended length on a multiple of the
    tile and one to either side; shorter than a tile; several interior tiles), the sequence counts, decimation factors
    and padded leading dimensions spread over them (preprocessing_common.cross_cases)."""
    d = pc.DESIGNS[di]
    _record_instantiation(record_property, d)
    for L, cols, nblocks, q, ldx, ldy in pc.cross_cases(di):
        _check_case(lib, d, L, cols, nblocks, q, ldx, ldy, 1000 * di + L)


@pytest.mark.parametrize("d", [("sos", 4, None), ("tf", 7, None)], ids=pc.design_id)
def test_filtfilt_decimation_factors(lib, d, record_property):
    """q in {1, 2, 3, 10, L, L + 5} at lengths with L % q in {0, 1, q - 1}: the kept-sample test m % q == 0 and the
    returned row count ceil(L / q) per block (asserted in _device_filtfilt and here)."""
    _record_instantiation(record_property, d)
    cases = [(60, 1), (60, 2), (61, 2), (60, 3), (61, 3), (62, 3), (60, 10), (61, 10), (69, 10), (60, 60), (61, 61),
             (60, 65), (31, 36)]
    for L, q in cases:
        assert L % q in (0, 1, q - 1) or q > L
        _check_case(lib, d, L, 3, 2, q, 3, 3, 7 * L + q)


@pytest.mark.parametrize("cols,nblocks", pc.SEQ_COUNTS)
def test_filtfilt_sequence_counts_and_leading_dimensions(lib, cols, nblocks, record_property):
    """A partial wave, an exact wave, two and three workgroups, the seq / cols split crossing block boundaries -- with
    ldx = cols + 3 (NaN in the input padding), ldy = cols + 2 and spare rows (sentinel intact), the column scales 2^k
    spread over k = -40..40 in one launch and one column on a 1e6 offset (make_signal)."""
    for d, L, q in ((("sos", 8, None), 75, 3), (("tf", 8, None), 70, 1)):
        _record_instantiation(record_property, d)
        _check_case(lib, d, L, cols, nblocks, q, cols + 3, cols + 2, 31 * cols + nblocks)


@pytest.mark.parametrize("d", [("sos", 4, None), ("tf", 5, None)], ids=pc.design_id)
def test_filtfilt_is_exactly_linear_in_powers_of_two(lib, d, record_property):
    """y(2^k x) == 2^k y(x) bitwise: the zi scaling and the odd extension are exactly linear in powers of two."""
    _record_instantiation(record_property, d)
    form, b, a, zi, padlen = pc.design(*d)
    L, cols, nblocks = 77, 7, 2
    x = pc.make_signal(L, cols, nblocks, 5, scales=False)
    y = _device_filtfilt(lib, form, b, a, zi, padlen, 2, x, nblocks)
    _assert_sequences_equal(y, pc.filtfilt_ref(form, b, a, zi, padlen, 2, x, nblocks), nblocks, pc.design_id(d))
    for k in (-40, -7, 13, 40):
        s = np.ldexp(1.0, k)
        ys = _device_filtfilt(lib, form, b, a, zi, padlen, 2, x * s, nblocks)
        _assert_sequences_equal(ys, y * s, nblocks, "%s scaled by 2^%d" % (pc.design_id(d), k))


@pytest.mark.parametrize("d", [("sos", 4, None), ("sos", 7, None), ("tf", 4, None), ("tf", 9, None)], ids=pc.design_id)
def test_filtfilt_sequences_are_independent(lib, d, record_property):
    """A NaN in one sequence and an Inf in another: every other sequence stays bit-equal, the poisoned ones equal the
    emulation under equal_nan."""
    _record_instantiation(record_property, d)
    form, b, a, zi, padlen = pc.design(*d)
    L, cols, nblocks = 90, 6, 2
    x = pc.make_signal(L, cols, nblocks, 9)
    clean = _device_filtfilt(lib, form, b, a, zi, padlen, 3, x, nblocks, cols + 3, cols + 2)
    xp = x.copy()
    xp[L // 2, 1] = np.nan      # block 0, column 1
    xp[L + 5, 4] = np.inf       # block 1, column 4
    dev = _device_filtfilt(lib, form, b, a, zi, padlen, 3, xp, nblocks, cols + 3, cols + 2, finite=False)
    poisoned = ((0, 1), (1, 4))
    _assert_sequences_equal(dev, clean, nblocks, pc.design_id(d) + " next to NaN / Inf", skip=poisoned)
    ref = pc.filtfilt_ref(form, b, a, zi, padlen, 3, xp, nblocks)
    assert np.isnan(ref[:30, 1]).all() and not np.isfinite(ref[30:, 4]).any()
    _assert_sequences_equal(dev, ref, nblocks, pc.design_id(d) + " poisoned (emulation)", equal_nan=True)


def test_filtfilt_workspace_reuse(lib):
    """The forward-pass work array shares its workspace slot with the wide TSQR launchers: a small call after a large
    call and a wide figh_tsqr gives the bits it gives when made first."""
    form, b, a, zi, padlen = pc.design("sos", 4)
    xs = pc.make_signal(45, 3, 2, 21)
    first = _device_filtfilt(lib, form, b, a, zi, padlen, 2, xs, 2)
    xl = pc.make_signal(300, 64, 8, 22)
    big = _device_filtfilt(lib, form, b, a, zi, padlen, 10, xl, 8)
    rng = np.random.default_rng(23)
    n, rows = 96, 960  # > 80 columns: the wide kernels
    A = rng.standard_normal((rows, n))
    d_R = lib.DeviceArray((n * n,), np.float64)
    d_A = lib.DeviceArray.from_host(A.reshape(-1))
    lib.tsqr(d_A, rows, n, None, n, None, None, d_R)
    R = np.triu(d_R.to_host().reshape(n, n))
    G = A.T @ A
    assert np.abs(R.T @ R - G).max() <= 1e-11 * np.abs(G).max()
    again = _device_filtfilt(lib, form, b, a, zi, padlen, 2, xs, 2)
    _assert_sequences_equal(again, first, 2, "small call after a large call and a wide TSQR")
    _assert_sequences_equal(again, pc.filtfilt_ref(form, b, a, zi, padlen, 2, xs, 2), 2, "small call (emulation)")
    _assert_sequences_equal(big[:30], pc.filtfilt_ref(form, b, a, zi, padlen, 10, xl[:300], 1), 1, "large call, block 0")


def test_filtfilt_argument_errors_leave_the_output_alone(lib):
    """Each bad argument raises FighError before any launch: the output still holds the sentinel."""
    sos = pc.design("sos", 4)
    tf = pc.design("tf", 4)
    base = dict(rows=60, cols=3, ldx=3, nblocks=2, form=0, b=sos[1], a=sos[2], zi=sos[3], padlen=27, q=2, ldy=3)
    bad = {
        "L == padlen": dict(rows=54),
        "nsec = 9": dict(b=np.ones((9, 3)), a=np.ones((9, 3)), zi=np.ones((9, 2))),
        "order = 17": dict(form=1, b=np.ones(18), a=np.ones(18), zi=np.ones(17), padlen=12),
        "rows % nblocks != 0": dict(rows=61),
        "form = 2": dict(form=2, b=tf[1], a=tf[2], zi=tf[3], padlen=12),
        "q = 0": dict(q=0),
        "ldx < cols": dict(ldx=2),
        "ldy < cols": dict(ldy=2),
    }
    d_x = lib.DeviceArray.from_host(np.ones(64 * 3))
    for what, change in bad.items():
        k = dict(base, **change)
        d_y = lib.DeviceArray.from_host(np.full(64 * 3, SENT))
        with pytest.raises(lib.FighError):
            lib.filtfilt_cols(d_x, k["rows"], k["cols"], k["ldx"], k["nblocks"], k["form"], k["b"], k["a"], k["zi"],
                              k["padlen"], k["q"], d_y, k["ldy"])
        assert _untouched(d_y.to_host()), what
    # the same buffers with the arguments in order
    d_y = lib.DeviceArray.from_host(np.full(64 * 3, SENT))
    assert lib.filtfilt_cols(d_x, 60, 3, 3, 2, 0, sos[1], sos[2], sos[3], 27, 2, d_y, 3) == 30
    assert not _untouched(d_y.to_host()[:90]) and _untouched(d_y.to_host()[90:])


# -------------------------------------------------------------------------------------------------- figh_compact_rows
def _device_compact(lib, W, cols, key_col, thr, tau, ld_out, spare=2):
    """figh_compact_rows on W (rows x ldw, the padding columns already filled by the caller) -> (count, out buffer
    (rows + spare) x ld_out, tau buffer rows + spare or None), both pre-filled with the sentinel."""
    rows, ldw = W.shape
    d_W = lib.DeviceArray.from_host(W.reshape(-1))
    d_out = lib.DeviceArray.from_host(np.full((rows + spare) * ld_out, SENT))
    d_tau = d_to = None
    if tau is not None:
        d_tau = lib.DeviceArray.from_host(tau)
        d_to = lib.DeviceArray.from_host(np.full(rows + spare, SENT))
    kept = lib.compact_rows(d_W.ptr, rows, cols, ldw, d_tau.ptr if d_tau else None, key_col, thr, d_out.ptr, ld_out,
                            d_to.ptr if d_to else None)
    return kept, d_out.to_host().reshape(rows + spare, ld_out), (d_to.to_host() if d_to else None)


def _check_compact(lib, W, cols, key_col, thr, tau, ld_out, what):
    Wk, tk, count = pc.compact_rows_ref(W, cols, key_col, thr, tau)
    kept, out, tout = _device_compact(lib, W, cols, key_col, thr, tau, ld_out)
    assert kept == count, "%s: %d rows kept, reference %d" % (what, kept, count)
    assert np.array_equal(out[:kept, :cols], Wk, equal_nan=True), "%s: first differing row %d" % (
        what, int(np.argmax((out[:kept, :cols] != Wk).any(axis=1))))
    assert _untouched(out[:kept, cols:]), what + ": output padding (ld_out > cols) written"
    assert _untouched(out[kept:]), what + ": rows past the returned count written"
    if tau is not None:
        assert np.array_equal(tout[:kept], tk), what + ": tau"
        assert _untouched(tout[kept:]), what + ": tau past the returned count written"
    return kept


@pytest.mark.parametrize("pattern", ["half", "all", "none", "first", "last"])
@pytest.mark.parametrize("rows", pc.COMPACT_ROWS)
def test_compact_rows_sizes_and_keep_patterns(lib, rows, pattern, record_property):
    """1, 64, 65 rows and 65536, 65537, 131077: one, two and three group counts per thread of the scan (the last two
    with threads whose range lies past the last group) -- 3 columns in ldw = 5 (NaN padding), ld_out = 4."""
    record_property("scan_counts_per_thread", pc.scan_per(rows))
    rng = np.random.default_rng(rows)
    W = _padded(rng.standard_normal((rows, 3)), 5)
    tau = rng.standard_normal(rows)
    thr = {"half": 0.6745, "all": 0.0, "none": 1.0e300, "first": 50.0, "last": 50.0}[pattern]
    if pattern == "first":
        W[0, 1] = -50.0
    if pattern == "last":
        W[-1, 1] = 50.0
    kept = _check_compact(lib, W, 3, 1, thr, tau, 4, "rows=%d %s" % (rows, pattern))
    assert kept == {"all": rows, "none": 0, "first": 1, "last": 1}.get(pattern, kept)
    if pattern == "half" and rows > 1000:
        assert 0.45 * rows < kept < 0.55 * rows


@pytest.mark.parametrize("cols", [1, 64, 65, 130])
def test_compact_rows_column_counts_and_padding(lib, cols):
    """One lane, one full pass, one pass + one lane and three passes of the copy loop over the columns; 193 rows (three
    groups and one row), ldw = cols + 3 with NaN padding, ld_out = cols + 2, the key in the last column."""
    rng = np.random.default_rng(cols)
    W = _padded(rng.standard_normal((193, cols)), cols + 3)
    _check_compact(lib, W, cols, cols - 1, 0.6, rng.standard_normal(193), cols + 2, "cols=%d" % cols)


def test_compact_rows_key_edges(lib):
    """Keys exactly +-thr are kept, the next double towards zero is dropped, a NaN key is dropped (as NumPy's >= does);
    -0.0 and 0.0 pass thr = 0.0."""
    thr = 0.6
    below = np.nextafter(thr, 0.0)
    keys = np.array([thr, -thr, below, -below, np.nan, np.nextafter(thr, 1.0), 0.0, -0.0, np.inf, -np.inf] * 13)
    W = np.c_[np.arange(keys.size, dtype=float), keys]
    assert _check_compact(lib, W, 2, 1, thr, np.arange(keys.size) + 0.5, 2, "keys at the threshold") == 5 * 13
    assert _check_compact(lib, W, 2, 1, 0.0, None, 3, "zero threshold") == 9 * 13
    assert _check_compact(lib, W, 2, 1, -0.0, None, 3, "negative-zero threshold") == 9 * 13


def test_compact_rows_without_tau_and_mismatched_pair(lib):
    """tau in and out both absent: W alone is compacted; one without the other is refused before any launch."""
    rng = np.random.default_rng(4)
    W = _padded(rng.standard_normal((131, 4)), 6)
    _check_compact(lib, W, 4, 2, 0.5, None, 5, "no tau")
    d_W = lib.DeviceArray.from_host(W.reshape(-1))
    d_tau = lib.DeviceArray.from_host(np.ones(131))
    for tau_in, tau_out in ((True, False), (False, True)):
        d_out = lib.DeviceArray.from_host(np.full(131 * 4, SENT))
        d_to = lib.DeviceArray.from_host(np.full(131, SENT))
        with pytest.raises(lib.FighError):
            lib.compact_rows(d_W.ptr, 131, 4, 6, d_tau.ptr if tau_in else None, 2, 0.5, d_out.ptr, 4,
                             d_to.ptr if tau_out else None)
        assert _untouched(d_out.to_host()) and _untouched(d_to.to_host())


# -------------------------------------------------------------------------------- figh_place_block, figh_gather_cols
def _grid_stride_elements(lib):
    """More elements than the capped grid has threads (cu_count * 16 blocks of 256): the grid-stride loop runs twice."""
    return lib.device_info()["cu_count"] * 16 * 256


@pytest.mark.parametrize("scale", [1.0, -1.0, 2.0 ** -3, 0.1])
def test_place_block_submatrix_views(lib, scale):
    """dst block = scale * src block with one rounding, between sub-matrix views with both leading dimensions larger
    than the width; everything around the destination block keeps the sentinel."""
    rng = np.random.default_rng(11)
    for rows, cols, lds, ldd in ((37, 19, 31, 26), (1, 1, 4, 3), (300, 257, 260, 259)):
        src = rng.standard_normal((rows + 4, lds)) * np.ldexp(1.0, rng.integers(-30, 30, (rows + 4, lds)))
        d_src = lib.DeviceArray.from_host(src.reshape(-1))
        d_dst = lib.DeviceArray.from_host(np.full((rows + 3) * ldd, SENT))
        r0, c0, r1, c1 = 2, 3, 1, 2
        assert c0 + cols <= lds and c1 + cols <= ldd
        lib.place_block(d_src.ptr + 8 * (r0 * lds + c0), lds, rows, cols, scale, d_dst.ptr + 8 * (r1 * ldd + c1), ldd)
        dst = d_dst.to_host().reshape(rows + 3, ldd)
        assert np.array_equal(dst[r1:r1 + rows, c1:c1 + cols], scale * src[r0:r0 + rows, c0:c0 + cols])
        mask = np.ones(dst.shape, bool)
        mask[r1:r1 + rows, c1:c1 + cols] = False
        assert _untouched(dst[mask]), "place_block wrote outside its %d x %d block" % (rows, cols)


def test_place_block_grid_stride_and_empty(lib, record_property):
    """A block with more elements than the capped grid has threads; rows = 0 and cols = 0 leave the destination alone."""
    cap = _grid_stride_elements(lib)
    cols = 1031
    rows = cap // cols + 2
    record_property("elements_over_grid_threads", "%.3f" % (rows * cols / cap))
    assert rows * cols > cap
    rng = np.random.default_rng(12)
    src = rng.standard_normal((rows, cols + 1))
    d_src = lib.DeviceArray.from_host(src.reshape(-1))
    d_dst = lib.DeviceArray.from_host(np.full((rows + 1) * (cols + 2), SENT))
    lib.place_block(d_src.ptr, cols + 1, rows, cols, 0.1, d_dst.ptr, cols + 2)
    dst = d_dst.to_host().reshape(rows + 1, cols + 2)
    assert np.array_equal(dst[:rows, :cols], 0.1 * src[:, :cols])
    assert _untouched(dst[:rows, cols:]) and _untouched(dst[rows:])
    d_dst = lib.DeviceArray.from_host(np.full(64, SENT))
    lib.place_block(d_src.ptr, cols + 1, 0, 5, 2.0, d_dst.ptr, 8)
    lib.place_block(d_src.ptr, cols + 1, 5, 0, 2.0, d_dst.ptr, 8)
    assert _untouched(d_dst.to_host())


def test_gather_cols_permutations_repeats_and_padding(lib, record_property):
    """out[:, j] = W[:, idx[j]] for a permutation and for a list with repeats, ldo > n with the padding intact, a block
    larger than the capped grid, n = 0."""
    rng = np.random.default_rng(13)
    cap = _grid_stride_elements(lib)
    for rows, ncols, ldw, idx in ((53, 17, 20, rng.permutation(17)), (53, 17, 20, np.array([3, 3, 0, 16, 3, 16, 5])),
                                  (1, 1, 1, np.array([0])), (cap // 700 + 2, 9, 12, rng.integers(0, 9, 700))):
        n = len(idx)
        W = _padded(rng.standard_normal((rows, ncols)), ldw)
        ldo = n + 3
        d_out = lib.DeviceArray.from_host(np.full((rows + 1) * ldo, SENT))
        d_W, d_idx = lib.DeviceArray.from_host(W.reshape(-1)), lib.DeviceArray.from_host(idx.astype(np.int32))
        lib.gather_cols(d_W, rows, ldw, d_idx, n, d_out, ldo)
        out = d_out.to_host().reshape(rows + 1, ldo)
        assert np.array_equal(out[:rows, :n], W[:, idx])
        assert _untouched(out[:rows, n:]) and _untouched(out[rows:])
    assert rows * n > cap
    record_property("elements_over_grid_threads", "%.3f" % (rows * n / cap))
    d_out = lib.DeviceArray.from_host(np.full(32, SENT))
    d_none = lib.DeviceArray((0,), np.int32)
    lib.gather_cols(d_W, rows, ldw, d_none, 0, d_out, 4)
    assert _untouched(d_out.to_host())


# -------------------------------------------------------------------------------------------------- _decimate_device
def test_decimate_device_two_stages_of_listed_blocks(lib):
    """_decimate_device on a GpuMatrix with ld > cols, blocks = [2, 0], two stages of q = 10 at the smallest block length
    that survives them (271 -> 28 > padlen 27 -> 3): bit-equal to two applications of filtfilt_ref on the host copy of
    the listed blocks, W and tau alike."""
    from figaroh_plus_amd.device import GpuMatrix
    from figaroh_plus_amd.identification.identification_tools import _decimate_design, _decimate_device
    nj, cols, ld, blocks, q = 271, 5, 8, [2, 0], 10
    W = pc.make_signal(nj, cols, 4, 17)
    tau = pc.make_signal(nj, 1, len(blocks), 18)[:, 0]
    dW = GpuMatrix(lib.DeviceArray.from_host(_padded(W, ld).reshape(-1)), 4 * nj, cols, ld)
    W_list, tau_list = _decimate_device(dW, tau, len(blocks), q, 2, blocks=blocks)
    sos, zi, padlen = _decimate_design(q)
    assert padlen == 27 and len(W_list) == len(tau_list) == 2

    def twice(x):
        once = pc.filtfilt_ref(0, sos[:, :3], sos[:, 3:], zi, padlen, q, x, 1)
        return pc.filtfilt_ref(0, sos[:, :3], sos[:, 3:], zi, padlen, q, once, 1)

    for i, blk in enumerate(blocks):
        got = W_list[i].numpy()
        assert got.shape == (3, cols) and tau_list[i].size == 3
        _assert_sequences_equal(got, twice(W[blk * nj:(blk + 1) * nj]), 1, "W block %d (row block %d of W)" % (i, blk))
        t = np.empty(3)
        lib.check(lib.load().figh_memcpy_d2h(t.ctypes.data, tau_list[i].ptr, t.nbytes))
        _assert_sequences_equal(t[:, None], twice(tau[i * nj:(i + 1) * nj, None]), 1, "tau block %d" % i)
