"""CPU suite: the one-sided Jacobi mirror of figh_singular_values_batch (_host.jacobi_singular_values_mirror) against its
own long-double run on the graded matrices of tests/singular_common.py, its sweep counts, the special matrices, and the
planted errors; the refusals of the entry that need no device."""
import numpy as np
import pytest

import singular_common as sc
from figaroh_plus_amd import _host


@pytest.fixture(scope="module")
def mirror_runs():
    """{(r, kind): (ratio to the long-double reference, sweeps, converged)} of the float64 mirror, computed once."""
    out = {}
    for r, kind in sc.cases():
        s, sweeps, conv = _host.jacobi_singular_values_mirror(sc.with_nan_below(sc.matrix_of(r, kind)))
        out[(r, kind)] = (sc.ratio_to_reference(s[0], sc.reference(r, kind)), int(sweeps[0]), int(conv[0]))
    return out


def test_mirror_within_c_sv_of_its_long_double_run(mirror_runs):
    for key, (ratio, sweeps, conv) in mirror_runs.items():
        assert conv == 1 and ratio <= sc.C_SV, (key, ratio, sweeps)


def test_c_oracle_matches_the_recorded_figures(mirror_runs):
    """C_SV is the power of two in [8, 16] x the recorded C_ORACLE (singular_common.py), and the largest ratio of
    the float64 mirror over the matrices is that figure."""
    worst = max(v[0] for v in mirror_runs.values())
    print("C_ORACLE measured %.6g (recorded %.6g); per case: %s"
          % (worst, sc.C_ORACLE, {k: round(v[0], 3) for k, v in mirror_runs.items()}))
    assert 8 * sc.C_ORACLE <= sc.C_SV <= 16 * sc.C_ORACLE and np.log2(sc.C_SV) == int(np.log2(sc.C_SV))
    assert 0.5 * sc.C_ORACLE <= worst <= 1.001 * sc.C_ORACLE  # (no larger; of its size on another host's LAPACK-made matrices)


def test_every_matrix_converges_within_thirty_sweeps(mirror_runs):
    """The cap of 40 in the device tests hides nothing: no test matrix can take the host fallback."""
    worst = max(v[1] for v in mirror_runs.values())
    print("sweeps: %s" % {k: v[1] for k, v in mirror_runs.items()})
    assert all(v[2] == 1 for v in mirror_runs.values())
    assert worst <= 30 and abs(worst - sc.SWEEPS_SEEN) <= 2  # (the recorded figure, give or take another host's matrices)


def test_batched_run_equals_the_single_runs():
    """The mirror is vectorised over B: a stack gives, matrix by matrix, the bits and the sweeps of the single runs (a matrix
    that has converged no longer moves while the others sweep on)."""
    r = 17
    stack = sc.with_nan_below(np.stack([sc.matrix_of(r, k) for k in sc.RATIOS + (sc.CLOSE,)]))
    s, sweeps, conv = _host.jacobi_singular_values_mirror(stack)
    for b in range(len(stack)):
        s1, w1, c1 = _host.jacobi_singular_values_mirror(stack[b])
        assert np.array_equal(s[b], s1[0]) and sweeps[b] == w1[0] and conv[b] == c1[0] == 1
    assert len(set(sweeps.tolist())) > 1


def test_round_robin_visits_every_pair_once():
    for r in sc.SIZES:
        steps = _host.jacobi_round_robin(r)
        assert len(steps) == (r - 1 if r % 2 == 0 else r)
        seen = set()
        for p, q in steps:
            assert len(p) <= (r + 1) // 2 and np.all(p < q) and np.all(q < r)
            assert len(set(p.tolist()) | set(q.tolist())) == 2 * len(p)  # disjoint
            seen.update(zip(p.tolist(), q.tolist()))
        assert len(seen) == r * (r - 1) // 2 == sum(len(p) for p, _ in steps)


def test_special_matrices():
    sp = sc.special_cases()
    s, sweeps, conv = _host.jacobi_singular_values_mirror(sc.with_nan_below(sp["zero"]))
    assert np.all(s == 0.0) and not np.any(np.signbit(s)) and conv[0] == 1 and sweeps[0] == 1
    s, sweeps, conv = _host.jacobi_singular_values_mirror(sc.with_nan_below(sp["zero_column"]))
    assert conv[0] == 1 and s[0, 1] == 0.0 and not np.signbit(s[0, 1]) and np.count_nonzero(s[0]) == 2
    want = np.linalg.svd(sp["zero_column"], compute_uv=False)
    assert np.allclose(np.sort(s[0])[::-1], want, rtol=1e-14, atol=0)
    s, sweeps, conv = _host.jacobi_singular_values_mirror(sc.with_nan_below(sp["identity"]))
    assert np.all(s == 1.0) and conv[0] == 1 and sweeps[0] == 1
    s, sweeps, conv = _host.jacobi_singular_values_mirror(sc.with_nan_below(sp["nan"]), max_sweeps=5)
    assert conv[0] == 0 and sweeps[0] == 5


def test_long_double_and_size_128_run():
    s, _, conv = _host.jacobi_singular_values_mirror(sc.with_nan_below(sc.matrix(128, 1e3)))
    assert conv[0] == 1 and s.dtype == np.float64 and s.shape == (1, 128)
    s, _, conv = _host.jacobi_singular_values_mirror(sc.with_nan_below(sc.matrix(16, 1e3)), dtype=np.longdouble)
    assert conv[0] == 1 and s.dtype == np.longdouble


@pytest.mark.parametrize("r", [3, 17])
@pytest.mark.parametrize("plant", ["last_step", "sign", "lower", "threshold"])
def test_planted_errors_are_caught(plant, r):
    """The scalar restatement passes the bound as it is and fails it (or does not converge) with each planted error: a
    dropped step, a flipped sign and the lower triangle on the graded matrices, the threshold of 2^-26 on the pair of equal
    columns whose cosine is 2^-30 (on graded matrices a skipped pair is a second-order effect and stays below the bound)."""
    kinds = (sc.CLOSE,) if plant == "threshold" else (1e3, 1e6)
    for kind in kinds:
        R, ref = sc.with_nan_below(sc.matrix_of(r, kind)), sc.reference(r, kind)
        s, sweeps, conv = sc.jacobi_scalar(R)
        assert conv == 1 and sc.ratio_to_reference(s, ref) <= sc.C_SV, (kind, sweeps)
        s, sweeps, conv = sc.jacobi_scalar(R, plant=plant)
        caught = conv == 0 or not np.isfinite(s).all() or sc.ratio_to_reference(s, ref) > sc.C_SV
        assert caught, (plant, r, kind, sweeps)


def test_device_route_without_a_device_fails_loudly():
    from figaroh_plus_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.FighError) as e:  # before any argument is looked at
        _lib.singular_values_batch(None, 0, 0, 0, 0, None, 0, None)
    assert e.value.code == _lib.ERR_NO_DEVICE
    with pytest.raises(_lib.FighError) as e:
        _lib.difference_quotients(None, 0, 0, 0, 7, None, None, 0)
    assert e.value.code == _lib.ERR_NO_DEVICE
