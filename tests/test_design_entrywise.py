"""GPU suite of the posture-selection entries (csrc/figh_design.hip): figh_design_scores bit for bit against the NumPy
mirror, figh_design_gram entry by entry against the derived bound of tests/design_common.py, the refusals, and the solvers
on a resident pool.  Every input has a padded leading dimension whose border holds a sentinel, every output is pre-filled
with the sentinel and has spare entries, which are asserted untouched."""
import numpy as np
import pytest

import design_common as dc
from figaroh_plus_amd.calibration import optimal_design as od
from figaroh_plus_amd.device import GpuMatrix

pytestmark = pytest.mark.gpu

# every tile count of the Gram kernel (1 .. 6 x 16 columns) and, for the scores, n below / at / above a multiple of 8, a padded
# n whose workgroup takes more than 64 KB of LDS (70, 80), and both widths that read their rows without the staging tile (88, 96)
NS = (1, 7, 8, 9, 20, 34, 50, 70, 80, 88, od.MAX_COLS)
CS = (1, 3, 6)
POOLS = (1, 63, 64, 65, 500)


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


def _upload(lib, R, pad):
    """R with `pad` sentinel columns behind every row; returns (device buffer, ldr)."""
    rows, n = R.shape
    host = np.full((rows, n + pad), dc.SENTINEL)
    host[:, :n] = R
    return lib.DeviceArray.from_host(host.reshape(-1)), n + pad


def _factor(R, n):
    """A Cholesky factor for the scores of any pool, full rank or not: of R^T R + I."""
    return np.linalg.cholesky(R.T @ R + np.eye(n))


def _device_scores(lib, d_R, ldr, N, c, n, L, which=(True, True, True)):
    outs = [lib.DeviceArray.from_host(np.full(N + 2, dc.SENTINEL)) for _ in range(3)]
    lib.design_scores(d_R.ptr, ldr, N, c, n, L, *[o if on else None for o, on in zip(outs, which)])
    host = [o.to_host() for o in outs]
    for h, on in zip(host, which):
        assert np.all(h[N:] == dc.SENTINEL)
        assert on or np.all(h == dc.SENTINEL)
    return [h[:N] for h in host]


def _problem(N, c, n, seed=0):
    return dc.random_problem("graded" if n >= 7 else "plain", N, c, n, seed)


@pytest.mark.parametrize("n", NS)
def test_scores_bit_equal_to_mirror(lib, n):
    """np.array_equal on trace, det_add and det_rm for every c and N, ldr = n + 3 with a sentinel border, sentinels behind
    the N outputs; at one shape per n, each output NULL on its own."""
    for c in CS:
        for N in POOLS:
            R = _problem(N, c, n)
            L = _factor(R, n)
            d_R, ldr = _upload(lib, R, 3)
            want = od.scores_mirror(R, N, c, L)
            got = _device_scores(lib, d_R, ldr, N, c, n, L)
            for name, g, w in zip(("trace", "det_add", "det_rm"), got, want):
                assert np.array_equal(g, w), (name, c, N, float(np.max(np.abs(g - w))))
            assert not np.any(np.signbit(got[2]))
            if c == 3 and N == 65:
                for off in range(3):
                    which = tuple(k != off for k in range(3))
                    part = _device_scores(lib, d_R, ldr, N, c, n, L, which)
                    assert all(np.array_equal(p, w) for p, w, on in zip(part, want, which) if on)


def test_scores_persistent_grid_with_ragged_tail(lib):
    """More 64-candidate tiles than the grid holds workgroups (four per compute unit), so every workgroup loops, and a last
    tile of 37 candidates; a design of four candidates, so det_rm is +0.0 for many of the others."""
    cus = lib.device_info()["cu_count"]
    N, c, n = 64 * (4 * cus) + 64 * 5 + 37, 3, 9
    R = _problem(N, c, n)
    design = np.arange(0, N, N // 4)[:4]  # twelve rows for nine columns: most other candidates cannot be taken out
    rows = np.concatenate([k * N + design for k in range(c)])
    L = np.linalg.cholesky(R[rows].T @ R[rows])
    d_R, ldr = _upload(lib, R, 1)
    want = od.scores_mirror(R, N, c, L)
    got = _device_scores(lib, d_R, ldr, N, c, n, L)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.any(got[2] == 0.0) and np.all(got[2][design] > 0.0)


@pytest.mark.parametrize("n", NS)
def test_gram_entrywise(lib, n):
    """|M_ab - exact| <= (c N + 2) u S_ab through an extended-precision reference whose own error is taken off the bound;
    w = None, random w and w with exact zeros in turn; symmetric bit for bit; two leading dimensions give the same bits;
    candidates of weight 0.0 contribute exact zeros (the same bits as the pool without them)."""
    kinds = (None, "random", "zeros")
    turn, worst = 0, 0.0
    for c in CS:
        for N in POOLS:
            R = _problem(N, c, n, seed=1)
            kind = kinds[turn % 3] if N >= 3 else kinds[turn % 2]
            turn += 1
            w = dc.weights(N, kind)
            d_w = lib.DeviceArray.from_host(w) if w is not None else None
            d_R, ldr = _upload(lib, R, 3)
            M = lib.design_gram(d_R.ptr, ldr, N, c, n, d_w)
            ratio = dc.gram_ratio_extended(M, R, N, c, w)
            assert ratio <= 1.0, (c, N, kind, ratio)
            worst = max(worst, ratio)
            assert np.array_equal(M, M.T)
            d_R2, ldr2 = _upload(lib, R, 0)
            assert np.array_equal(lib.design_gram(d_R2.ptr, ldr2, N, c, n, d_w), M)
            assert np.array_equal(lib.design_gram(d_R.ptr, ldr, N, c, n, d_w), M)
            if kind == "zeros":
                keep = np.flatnonzero(w != 0.0)
                sub = R[np.concatenate([k * N + keep for k in range(c)])]
                d_sub, ld_sub = _upload(lib, sub, 0)
                d_wk = lib.DeviceArray.from_host(w[keep])
                # (the same candidates in the same order and wave partition only when nothing moves: compare by the bound)
                assert dc.gram_ratio_extended(lib.design_gram(d_sub.ptr, ld_sub, len(keep), c, n, d_wk), R, N, c, w) <= 1.0
                only = np.zeros(N)
                assert not np.any(lib.design_gram(d_R.ptr, ldr, N, c, n, lib.DeviceArray.from_host(only)))
    print("gram device ratio n = %d: %.4f" % (n, worst))


def test_gram_many_workgroups(lib):
    """A pool beyond eight workgroups per compute unit (the most that are resident) x 256 candidates: every wave owns more
    than 64 candidates, the last ones a ragged run."""
    cus = lib.device_info()["cu_count"]
    N, c, n = 256 * (8 * cus) + 64 * 3 + 37, 2, 7
    R = _problem(N, c, n, seed=2)
    w = dc.weights(N, "zeros")
    d_R, ldr = _upload(lib, R, 1)
    M = lib.design_gram(d_R.ptr, ldr, N, c, n, lib.DeviceArray.from_host(w))
    assert dc.gram_ratio_extended(M, R, N, c, w) <= 1.0 and np.array_equal(M, M.T)


def test_refusals_launch_nothing(lib):
    """Every FIGH_ERR_INVALID cause of the two entries: nothing is launched (figh_profile_get), no output is touched."""
    N, c, n = 70, 3, 9
    R = _problem(N, c, n)
    L = _factor(R, n)
    d_R, ldr = _upload(lib, R, 2)
    outs = [lib.DeviceArray.from_host(np.full(N + 2, dc.SENTINEL)) for _ in range(3)]
    h_M = np.full((n, n), dc.SENTINEL)
    raw = lib.load()
    import ctypes as C

    def gram(c=c, n=n, ldr=ldr, N=N, R=d_R.ptr, M=h_M):
        lib.check(raw.figh_design_gram(R, ldr, N, c, n, None, M.ctypes.data_as(C.POINTER(C.c_double)) if M is not None else None))

    def scores(c=c, n=n, ldr=ldr, N=N, L=L, outs=outs):
        Lh = np.ascontiguousarray(L, dtype=np.float64)
        lib.check(raw.figh_design_scores(d_R.ptr, ldr, N, c, n, Lh.ctypes.data_as(C.POINTER(C.c_double)),
                                         *[o.ptr if o is not None else None for o in outs]))

    def bad_diag(value, at=4):
        Lb = L.copy()
        Lb[at, at] = value
        return Lb

    cases = [(gram, dict(c=0)), (gram, dict(c=7)), (gram, dict(n=0)), (gram, dict(n=od.MAX_COLS + 1)),
             (gram, dict(ldr=n - 1)), (gram, dict(N=0)), (gram, dict(R=None)), (gram, dict(M=None)),
             (scores, dict(c=0)), (scores, dict(c=7)), (scores, dict(n=0)), (scores, dict(n=od.MAX_COLS + 1)),
             (scores, dict(ldr=n - 1)), (scores, dict(N=0)), (scores, dict(N=-5)), (scores, dict(outs=[None, None, None])),
             (scores, dict(L=bad_diag(0.0))), (scores, dict(L=bad_diag(-1.0))), (scores, dict(L=bad_diag(np.nan))),
             (scores, dict(L=bad_diag(np.inf))), (scores, dict(L=bad_diag(-0.0, at=n - 1)))]
    lib.profile_enable(level=2)
    try:
        lib.profile_reset()
        for call, kw in cases:
            with pytest.raises(lib.FighError) as e:
                call(**kw)
            assert e.value.code == lib.ERR_INVALID, kw
            assert str(e.value).split(": ", 1)[1], kw  # figh_last_error says why
        assert lib.profile_get("design_gram")[0] == 0 and lib.profile_get("design_scores")[0] == 0
        assert np.all(h_M == dc.SENTINEL) and all(np.all(o.to_host() == dc.SENTINEL) for o in outs)
        gram()
        scores()
        assert lib.profile_get("design_gram")[0] == 1 and lib.profile_get("design_scores")[0] == 1
        assert not np.any(h_M == dc.SENTINEL) and all(not np.any(o.to_host()[:N] == dc.SENTINEL) for o in outs)
    finally:
        lib.profile_enable(False)


def test_resident_pool_is_never_downloaded(lib, monkeypatch, capsys):
    """A GpuMatrix pool with a padded leading dimension goes through SOCP.solve and Detmax.main_algo while GpuMatrix.numpy
    raises: only the n x n matrix and the N scores cross the bus."""
    R = dc.fixture_pool(6)
    N, c, n = R.shape[0] // 6, 6, R.shape[1]
    buf, ldr = _upload(lib, R, 2)
    resident = GpuMatrix(buf, c * N, n, ldr)

    def refuse(self):
        raise AssertionError("the pool was downloaded")

    monkeypatch.setattr(GpuMatrix, "numpy", refuse)
    pool = od.CandidatePool(resident, N, c)
    assert pool.on_device and pool.R_dev is resident
    solver = od.SOCP(pool, {"NbSample": N})
    w = np.array(solver.solve(tol=1e-3)[0])
    assert solver.max_variance <= n * (1 + 1e-3) and abs(w.sum() - 1.0) < 1e-9
    chosen = od.select_configurations(solver.solve(tol=1e-3)[1], min_chosen=n // c + 1)
    assert len(chosen) >= n // c + 1
    algo = od.Detmax(pool, n // c + 2)
    crit = algo.main_algo(rng=5)
    assert len(algo.opt_set) == n // c + 2 and all(b >= a * (1 - 1e-12) for a, b in zip(crit, crit[1:]))
    assert od.detroot_whole(pool) > 0.0
    capsys.readouterr()


@pytest.mark.parametrize("c", [3, 6])
def test_device_solve_equals_mirror_solve(lib, c, monkeypatch, capsys):
    """The fixture pool through both routes: the weights agree to 1e-12 (the Gram matrices are not bit-equal between the
    routes, so neither are the weights) after the same number of updates; Detmax on the 40-candidate pool selects the
    identical sequence of sets."""
    R = dc.fixture_pool(c)
    N = R.shape[0] // c
    Rd = dc.detmax_pool()
    initial = [17, 3, 29, 8]
    runs = {}
    for route in ("device", "mirror"):
        with monkeypatch.context() as mp:
            if route == "mirror":
                mp.setattr(od._lib, "device_count", lambda: 0)
            pool = od.CandidatePool(R, N, c)
            assert pool.on_device == (route == "device")
            solver = od.SOCP(pool, {"NbSample": N})
            w = np.array(solver.solve(tol=1e-3)[0])
            algo = od.Detmax(od.CandidatePool(Rd, 40, 3), 4)
            crit = algo.main_algo(initial_set=initial)
            runs[route] = (w, solver.iterations, crit, algo.opt_set)
    dev, host = runs["device"], runs["mirror"]
    assert dev[1] == host[1] and np.allclose(dev[0], host[0], rtol=0, atol=1e-12)
    assert dev[3] == host[3] and len(dev[2]) == len(host[2]) and np.allclose(dev[2], host[2], rtol=1e-12, atol=0)
    capsys.readouterr()
