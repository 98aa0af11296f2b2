"""Reference side of the bit-exact preprocessing tests (test_preprocessing_host.py, test_preprocessing_exact.py).

figh_filtfilt_cols runs SciPy's recurrences with __dmul_rn / __dadd_rn / __dsub_rn only, in SciPy's operation order, so
its result is determined bit for bit by IEEE-754 double arithmetic.  The oracle is therefore a NumPy emulation of the
same recurrences: float64, ONE NumPy statement per rounding (NumPy never contracts separate ufunc calls into an FMA),
vectorised across the sequences, a Python loop over the samples.  A long-double reference is the wrong oracle here: the
recurrence amplifies its own roundings, and the float64 and long-double runs of one design differ by up to 1e-8 of the
sequence maximum (test_preprocessing_host.py measures it) -- any tolerance against it would be wide enough to hide a
wrong operation order.  The long-double mode of these functions exists only for that guard: it keeps a design whose
recurrence is unstable -- where bit comparison means nothing -- out of the table.

The case table of the GPU module lives here too, so that the host suite can check what it covers without a device.
"""
import numpy as np

TB = 32  # samples per tile of filtfilt_cols_kernel

# ---------------------------------------------------------------------------------------------------- the recurrences


def odd_ext(x, edge):
    """scipy.signal._arraytools.odd_ext along axis 0 (one subtraction per sample; 2 * x is exact)."""
    x = np.asarray(x)
    if edge == 0:
        return x.copy()
    left = 2 * x[0] - x[edge:0:-1]
    right = 2 * x[-1] - x[-2:-edge - 2:-1]
    return np.concatenate([left, x, right], axis=0)


def sos_pass(b, a, zi, x):
    """scipy/signal/_sosfilt.pyx over axis 0 of x; b, a: (nsec, 3), zi: (nsec, 2); the state starts at zi * x[0]."""
    dt = x.dtype
    b, a, zi = (np.asarray(v, dtype=dt) for v in (b, a, zi))
    nsec = b.shape[0]
    z0 = [zi[s, 0] * x[0] for s in range(nsec)]
    z1 = [zi[s, 1] * x[0] for s in range(nsec)]
    y = np.empty_like(x)
    for n in range(x.shape[0]):
        xc = x[n]
        for s in range(nsec):
            t = b[s, 0] * xc
            yc = t + z0[s]
            t1 = b[s, 1] * xc
            t2 = a[s, 1] * yc
            t3 = t1 - t2
            z0[s] = t3 + z1[s]
            t4 = b[s, 2] * xc
            t5 = a[s, 2] * yc
            z1[s] = t4 - t5
            xc = yc
        y[n] = xc
    return y


def tf_pass(b, a, zi, x):
    """scipy/signal/_lfilter.c.in (direct form II transposed, a[0] = 1) over axis 0 of x; zi: (order,)."""
    dt = x.dtype
    b, a, zi = (np.asarray(v, dtype=dt).reshape(-1) for v in (b, a, zi))
    order = b.size - 1
    z = [zi[i] * x[0] for i in range(order)]
    y = np.empty_like(x)
    for n in range(x.shape[0]):
        xc = x[n]
        t = b[0] * xc
        yc = z[0] + t
        for i in range(order - 1):
            t1 = xc * b[i + 1]
            t2 = z[i + 1] + t1
            t3 = yc * a[i + 1]
            z[i] = t2 - t3
        t4 = xc * b[order]
        t5 = yc * a[order]
        z[order - 1] = t4 - t5
        y[n] = yc
    return y


def filtfilt_ref(form, b, a, zi, padlen, q, x2d, nblocks, dtype=np.float64):
    """figh_filtfilt_cols on the host: x2d is (nblocks * L, cols); per row block extend, forward pass, backward pass over
    the reversed output with the state re-initialised from the last forward output, un-reverse, drop the extension, keep
    every q-th sample.  Returns (nblocks * ceil(L / q), cols) in ``dtype``."""
    x2d = np.asarray(x2d, dtype=np.float64)
    rows, cols = x2d.shape
    assert rows % nblocks == 0
    L = rows // nblocks
    assert L > padlen >= 0 and q >= 1
    # the blocks are independent sequences: (L, nblocks * cols), all through the Python loop at once
    x = x2d.reshape(nblocks, L, cols).transpose(1, 0, 2).reshape(L, nblocks * cols).astype(dtype)
    run = sos_pass if form == 0 else tf_pass
    with np.errstate(invalid="ignore", over="ignore"):
        ext = odd_ext(x, padlen)
        fwd = run(b, a, zi, ext)
        bwd = run(b, a, zi, fwd[::-1])
        y = bwd[::-1]
    y = y[padlen:padlen + L][::q]
    return np.ascontiguousarray(y.reshape(-1, nblocks, cols).transpose(1, 0, 2).reshape(-1, cols))


def compact_rows_ref(W, cols, key_col, thr, tau=None):
    """figh_compact_rows on the host: rows with |W[:, key_col]| >= thr, in order (a NaN key drops its row, as NumPy's
    >= does).  Returns (kept rows of W[:, :cols], kept tau or None, count)."""
    W = np.asarray(W)
    with np.errstate(invalid="ignore"):
        keep = np.abs(W[:, key_col]) >= thr
    return W[keep][:, :cols].copy(), (None if tau is None else np.asarray(tau)[keep].copy()), int(keep.sum())


COMPACT_ROWS = [1, 64, 65, 65536, 65537, 131077]  # 1024 groups: the last size with one count per scan thread


def scan_per(rows):
    """Group counts per thread of compact_scan_kernel (1024 threads over the 64-row groups)."""
    ngroups = (rows + 63) // 64
    return (ngroups + 1023) // 1024


# ------------------------------------------------------------------------------------------------------- the designs
Q_DESIGN = 10  # the decimation factor of the real-data scripts: Chebyshev-I cut-off 0.8 / 10


def butter_wn(order):
    """Cut-off per order: as low as the float64 recurrence stays within the guard of test_preprocessing_host.py."""
    return 0.02 if order <= 6 else 0.05 if order <= 8 else 0.1 if order <= 10 else 0.2 if order <= 13 else 0.3


def design(kind, n, padlen=None):
    """(form, b, a, zi, padlen) of a table entry: ("sos", nsec) = Chebyshev-I of order 2 nsec as scipy.signal.decimate
    designs it, with sosfiltfilt's padlen rule; ("tf", order) = Butterworth with filtfilt's default padlen."""
    from scipy import signal
    if kind == "sos":
        sos = signal.cheby1(2 * n, 0.05, 0.8 / Q_DESIGN, output="sos")
        ntaps = 2 * sos.shape[0] + 1
        ntaps -= min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())
        return 0, sos[:, :3].copy(), sos[:, 3:].copy(), signal.sosfilt_zi(sos), int(3 * ntaps if padlen is None else padlen)
    b, a = signal.butter(n, butter_wn(n))
    assert a[0] == 1.0
    return 1, b, a, signal.lfilter_zi(b, a), int(3 * n if padlen is None else padlen)


def scipy_ref(kind, n, padlen, q, x2d, nblocks):
    """The same call through scipy.signal (sosfiltfilt / filtfilt, odd padding), block by block."""
    from scipy import signal
    L = x2d.shape[0] // nblocks
    out = []
    for k in range(nblocks):
        xb = x2d[k * L:(k + 1) * L]
        if kind == "sos":
            sos = signal.cheby1(2 * n, 0.05, 0.8 / Q_DESIGN, output="sos")
            y = signal.sosfiltfilt(sos, xb, axis=0, padtype="odd", padlen=padlen)
        else:
            b, a = signal.butter(n, butter_wn(n))
            y = signal.filtfilt(b, a, xb, axis=0, padtype="odd", padlen=padlen)
        out.append(y[::q])
    return np.vstack(out)


# (kind, n, explicit padlen or None).  The explicit padlens put the edge exactly on a tile boundary (0, TB, 2 TB).
DESIGNS = ([("sos", ns, None) for ns in range(1, 9)] + [("tf", order, None) for order in range(1, 17)]
           + [("sos", 4, p) for p in (0, 32, 64)] + [("tf", 4, p) for p in (0, 32, 64)])

# Designs for which scipy.signal does NOT reproduce the emulation bit for bit on the SciPy of this project's machines
# (test_preprocessing_host.py asserts the complement): they rely on the emulation alone in the GPU module.
SCIPY_DISAGREES = frozenset()

# the case labels of the two switch statements of figh_filtfilt_cols (figh_signal.hip), kept as data
SOS_CASE_LABELS = (1, 2, 3, 4, 5, 6)
TF_CASE_LABELS = (1, 2, 3, 4, 5, 6, 8)


def instantiation(kind, n):
    """The kernel instantiation a design launches: (form, label) with label a case label or "default"."""
    if kind == "sos":
        return (0, n if n in SOS_CASE_LABELS else "default")
    return (1, n if n in TF_CASE_LABELS else "default")


ALL_INSTANTIATIONS = ([(0, c) for c in SOS_CASE_LABELS] + [(0, "default")] + [(1, c) for c in TF_CASE_LABELS]
                      + [(1, "default")])


def design_id(d):
    return "%s%d" % (d[0], d[1]) + ("" if d[2] is None else "_pad%d" % d[2])


def lengths(edge):
    """The smallest lengths that reach every branch of the kernel's tiling for an edge (= padlen):
      - edge + 1: the minimum, every extension index at its extreme;
      - Lext = L + 2 edge on a multiple of TB and one to either side of it: a full, a 1-sample and a 31-sample last
        tile of the forward pass (= first tile of the backward pass, whose partial tile is at the low end).  The
        multiple is the smallest above 3 edge; where one of the three lengths would not exceed the edge (3 edge + 1 a
        multiple of TB: edge 21) the next multiple supplies it;
      - TB - 1 - 2 edge where that is a valid length: Lext = 31, no interior tile and no second tile at all;
      - 203 (7 * 29: odd, no multiple of TB, of 2, 3 or 10): several interior tiles."""
    m = (3 * edge // TB + 1) * TB
    out = [edge + 1]
    for d in (-1, 0, 1):
        L = m - 2 * edge + d
        out.append(L if L > edge else L + TB)
    if TB - 1 - 2 * edge > edge:
        out.append(TB - 1 - 2 * edge)
    out.append(203)
    seen, uniq = set(), []
    for L in out:
        if L not in seen:
            seen.add(L)
            uniq.append(L)
    return uniq


SEQ_COUNTS = [(1, 1), (63, 1), (64, 1), (65, 1), (5, 13), (43, 3)]  # (cols, nblocks)
Q_CYCLE = [1, 2, 3, 10]


def cross_cases(di):
    """(L, cols, nblocks, q, ldx, ldy) for design number ``di``: every length of ``lengths``; the sequence counts, the
    decimation factors and the padded leading dimensions are spread over designs and lengths (every design sees each
    of them at least once over its lengths, rotated by the design number)."""
    edge = design(*DESIGNS[di])[4]
    out = []
    for li, L in enumerate(lengths(edge)):
        cols, nblocks = SEQ_COUNTS[(di + li) % len(SEQ_COUNTS)]
        q = Q_CYCLE[(di + 2 * li) % len(Q_CYCLE)]
        pad = (di + li) % 2 == 0
        out.append((L, cols, nblocks, q, cols + (3 if pad else 0), cols + (2 if pad else 0)))
    return out


def make_signal(L, cols, nblocks, seed, scales=True):
    """Sine + noise + offset (the shape of the suite's other filter tests); column c scaled by 2^k with k spread over
    -40..40 across the columns of one launch, the last column of a launch with >= 3 columns on a 1e6 offset."""
    rng = np.random.default_rng(seed)
    t = np.arange(L * nblocks)[:, None]
    x = np.sin(0.01 * t * (1 + np.arange(cols))) + 0.1 * rng.standard_normal((L * nblocks, cols)) + 3.0
    if scales and cols > 1:
        k = np.round(np.linspace(-40, 40, cols)).astype(int)
        x = x * np.ldexp(1.0, k)[None, :]
    if cols >= 3:
        x[:, -1] = np.sin(0.013 * t[:, 0]) + 0.1 * rng.standard_normal(L * nblocks) + 1.0e6
    return x
