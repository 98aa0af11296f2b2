"""GPU suite: the one-call fused pass (figh_chain_pass_fused: launches, one copy, selection check and native host tail) against
the same pipeline with ``native_tail=False`` (one call per launch, NumPy / LAPACK tail) on the same inputs.

Index sets, names, expressions and ``beta`` are compared exactly; ``col_norm`` and ``sel`` bit for bit (the same kernels sum
in the same fixed order).  ``absdiagR`` (1e-11, up to the first dependent column: behind it no two Householder orders
agree), ``residual_norm`` (1e-11) and ``phi_ls`` (1e-10) carry the tolerances tests/test_gpu_parity.py uses between fused
runs: which consumer wave takes which tile is decided at run time, so R is reproduced up to rounding."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


def _pipes(g, q, v, a, with_tau, seed=3):
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    both = []
    for native in (False, True):
        pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling, native_tail=native)
        pipe.set_samples(q, v, a)
        if with_tau:
            pipe.set_tau_from_parameters(g.phi_ref(), noise_std=0.05, seed=seed)
        both.append(pipe)
    return both


def _sel(pipe):
    ncols = pipe.W.ref_cols
    return pipe._host_pack.array[ncols:ncols + pipe._sel_words].view(np.int32)[:2 + 2 * ncols].copy()


def _same(py, nat, with_tau):
    assert nat["idx_e"] == py["idx_e"] and nat["params_r"] == py["params_r"]
    assert nat["idx_base"] == py["idx_base"] and nat["params_base"] == py["params_base"]
    assert nat["rows"] == py["rows"]
    assert nat.get("null_rule_certified") == py.get("null_rule_certified")
    assert np.array_equal(nat["col_norm"], py["col_norm"]), "col_norm is not bit-identical"
    assert np.array_equal(nat["beta"], py["beta"])
    dep = [i for i in range(len(py["params_r"])) if i not in set(py["idx_base"])]
    first_dep = min(dep) if dep else len(py["params_r"])
    d_a, d_b = py["absdiagR"][:first_dep], nat["absdiagR"][:first_dep]
    assert np.abs(d_a - d_b).max() <= 1e-11 * d_a.max()
    if with_tau:
        assert np.abs(nat["phi_ls"] - py["phi_ls"]).max() <= 1e-10 * np.abs(py["phi_ls"]).max()
        assert np.array_equal(nat["phi_b"], np.round(nat["phi_ls"], 6))
        assert abs(nat["residual_norm"] - py["residual_norm"]) <= 1e-11 * py["residual_norm"]
    else:
        assert "phi_ls" not in nat and "phi_ls" not in py


@pytest.mark.parametrize("with_tau", [True, False])
@pytest.mark.parametrize("N", [4096, 4096 + 37])
def test_native_pass_equals_python_pass(lib, golden_ur10, N, with_tau):
    g = golden_ur10
    rng = np.random.default_rng(500 + N)
    q, v, a = (rng.uniform(-6, 6, (N, 6)) for _ in range(3))
    py, nat = _pipes(g, q, v, a, with_tau)
    for rep in range(2):  # (the first pass learns the kept set from the prefix and is fused as well)
        o_py, o_nat = py.run(), nat.run()
        assert py.fused_passes == nat.fused_passes == rep + 1
        _same(o_py, o_nat, with_tau)
        assert np.array_equal(_sel(py), _sel(nat)), "sel is not bit-identical"
        assert o_nat["idx_e"] == list(g["idx_e"]) and o_nat["idx_base"] == list(g["idx_base"])
        assert o_nat["params_base"] == g.meta["params_base"]
    assert nat.strings_memo_hits >= 1  # (same kept set, index sets and rounded coefficients in the second pass)


def test_native_pass_falls_back_when_the_kept_set_changes(lib, golden_ur10):
    """Samples with another elimination pattern under the same pipeline: the one-call pass reports the changed selection, the
    two-launch path solves the pass and learns the new set, the pass after that is one call again."""
    g = golden_ur10
    N = 4096
    rng = np.random.default_rng(77)
    q, v, a = (rng.uniform(-6, 6, (N, 6)) for _ in range(3))
    py, nat = _pipes(g, q, v, a, True)
    _same(py.run(), nat.run(), True)
    q2, v2, a2 = q.copy(), v.copy(), a.copy()
    q2[:, :3] = 0.0
    v2[:, :3] = 0.0
    a2[:, :3] = 0.0
    for pipe in (py, nat):
        for d_arr, h in ((pipe.d_q, q2), (pipe.d_v, v2), (pipe.d_a, a2)):
            h = np.ascontiguousarray(h)
            lib.check(lib.load().figh_memcpy_h2d(d_arr.ptr, h.ctypes.data, h.nbytes))
    fused_before = nat.fused_passes
    o_py, o_nat = py.run(), nat.run()
    assert nat.fused_passes == fused_before and py.fused_passes == fused_before  # (both fell back to the two launches)
    assert len(o_nat["idx_e"]) != len(g["idx_e"])
    _same(o_py, o_nat, True)
    o_py, o_nat = py.run(), nat.run()
    assert nat.fused_passes == fused_before + 1 and py.fused_passes == fused_before + 1
    _same(o_py, o_nat, True)


def test_native_pass_after_forget(lib, golden_ur10):
    g = golden_ur10
    N = 4096 + 37
    rng = np.random.default_rng(78)
    q, v, a = (rng.uniform(-6, 6, (N, 6)) for _ in range(3))
    py, nat = _pipes(g, q, v, a, True)
    first = nat.run()
    _same(py.run(), first, True)
    for pipe in (py, nat):
        pipe.forget()
    o_py, o_nat = py.run(), nat.run()
    assert nat.prefix_passes == 2 and nat.fused_passes == 2
    _same(o_py, o_nat, True)
    assert o_nat["idx_base"] == first["idx_base"] and np.array_equal(o_nat["beta"], first["beta"])
