"""The state of ``IdentificationPipeline`` is declared once, by lifetime (the table in the class docstring): no attribute is
born in the middle of a pass, and ``forget()`` puts every attribute learnt from earlier passes back to its declared initial
value.  CPU part: the device-free construction of tests/test_host_tail_native.py through ``_finish``.  GPU part: one sequence
of calls per path family, each at the smallest shape that still takes its path.  No numerical value is asserted here: the rest
of the suite holds those."""
import os

import numpy as np
import pytest

from figaroh_plus_amd import _lib
from figaroh_plus_amd.pipeline import IdentificationPipeline

# the "learnt from earlier passes" group and its initial values, as the class docstring states them
LEARNT = {"_fused_kept": None, "_kept_cache": None, "_n_expected": -1, "_nf_expected": -1, "_mask_expected": None,
          "_block_cache": None, "_chunk_kept": None, "_cert_cache": None}


def _learnt(pipe):
    return {k: getattr(pipe, k) for k in LEARNT}


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("null_pivots", [True, False])
@pytest.mark.parametrize("native_tail", [True, False])
def test_finish_adds_no_attribute(built, native_tail, null_pivots):
    from test_host_tail_native import ROWS, make_rows
    names = {"p%d" % i: 0.0 for i in range(80)}
    p = IdentificationPipeline(None, None, params_std=names, native_tail=native_tail, null_pivots=null_pivots)
    declared = set(vars(p))
    assert _learnt(p) == LEARNT
    p.N = 10 ** 9  # (one separately launched piece whatever total_rows, as in test_host_tail_native.pipes)
    n = 6
    for dep, seed in (([], 31), ([2, 4], 32)):  # full rank, rank deficient
        rows_k = make_rows(n, dep, True, seed)[0]
        out = p._finish(rows_k, n, n + 1, ["p%d" % i for i in range(n)], [], np.zeros(n), True, ROWS, True)
        assert len(out["idx_base"]) == n - len(dep)
        assert set(vars(p)) == declared
    p.forget()
    assert set(vars(p)) == declared and _learnt(p) == LEARNT


# ------------------------------------------------------------------------------------------------ GPU
def _problem(family):
    """(golden fixture, constructor arguments, N, run() arguments) of a path family."""
    from conftest import Golden
    if family == "ur10_fused_native":  # the fused launch refuses fewer than 4096 local samples
        return Golden("cfg2_ur10"), {}, 4096, {}
    if family == "ur10_two_launch":  # ragged last tile
        return Golden("cfg2_ur10"), {"fuse": False}, 200, {}
    if family == "tx40_coupling":
        return Golden("cfg1_tx40"), {}, 200, {}
    if family.startswith("tiago_"):  # per-row-block TSQR and its triangles
        g = Golden("cfg3_tiago")
        kw = {"tiago_dense": {"w_layout": "dense"}, "tiago_block_compact": {"w_layout": "block-compact"}}.get(family)
        if kw is None:
            m = g.robot().model
            kw = {"row_blocks": [m.joints[m.getJointId("arm_%d_joint" % k)].idx_v for k in (1, 2)]}
        return g, kw, 128, {"wls": True}
    if family.startswith("human_"):  # external wrench on the free-flyer: link-compact and force-compact W
        from figaroh_plus_amd.tools.regressor import regressor_flags
        g = Golden("cfg5_human")
        mode, flags, _ = regressor_flags(g.param, g.coupling)
        ncols = g.robot().device_model().shape(mode, flags)[1]
        N = 64 * -(-16 * (ncols + 1) // (3 * 64))  # the smallest multiple of 64 with 3 N >= 16 (ncols + 1)
        assert 3 * N >= 16 * (ncols + 1) > 3 * (N - 64)
        return g, {}, N, ({"wls": True} if family == "human_wls" else {})
    assert family == "ur10_chunked"  # streamed pass: two passes over the samples first, one from then on
    return Golden("cfg2_ur10"), {"chunk_samples": 128}, 300, {}


def _samples(g, N, seed):
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    rng = np.random.default_rng(seed)
    if g.model_name == "ur10":
        return tuple(rng.uniform(-6, 6, (N, 6)) for _ in range(3))
    return sample_inputs(g.robot().model, N, rng, 1.5, 2, 5)


FAMILIES = ["ur10_fused_native", "ur10_two_launch", "tx40_coupling", "tiago_dense", "tiago_block_compact", "tiago_row_blocks",
            "human_run", "human_wls", "ur10_chunked"]


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_no_attribute_is_born_in_a_pass(family):
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    g, kw, N, run_kw = _problem(family)

    def make():
        return IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling, **kw)

    def load(pipe, seed):
        pipe.set_samples(*_samples(g, N, seed))
        pipe.set_tau_from_parameters(g.phi_ref(), noise_std=0.05, seed=seed)
        assert set(vars(pipe)) == declared, "set_samples: %s" % sorted(set(vars(pipe)) ^ declared)

    def run(pipe, what):
        # (human_wls: a plain first pass, so that the weighted one has a force-compact W to drop and re-create)
        out = pipe.run(**({} if family == "human_wls" and what == "first pass" else run_kw))
        assert set(vars(pipe)) == declared, "%s: %s" % (what, sorted(set(vars(pipe)) ^ declared))
        return out

    pipe = make()
    declared = set(vars(pipe))
    assert _learnt(pipe) == LEARNT
    load(pipe, 5)
    outs = [run(pipe, "first pass")]
    if family.startswith("human_"):
        assert pipe._link_pos is not None and pipe._force_ld > 0 and pipe.W.force_ld == pipe._force_ld
    outs += [run(pipe, what) for what in ("speculative repeat", "steady state")]
    # the path the family is named after was taken
    if family == "ur10_fused_native":
        assert pipe.fused_passes == 3 and pipe.prefix_passes == 1
    else:
        assert pipe.fused_passes == 0 and pipe.prefix_passes == 0
    if family.startswith("tiago_"):
        assert pipe._tree_blocks and outs[-1]["wls_source"] == "per-row-block triangles"
        assert (pipe._compact is not None) == (family == "tiago_block_compact")
    if family == "human_wls":
        assert pipe._link_pos is not None and pipe._force_ld == 0 and outs[-1]["wls_source"] == "second pass over W"
    if family == "ur10_chunked":
        assert pipe.W is None and pipe._chunk_kept is not None
    pipe.forget()
    assert set(vars(pipe)) == declared
    assert _learnt(pipe) == LEARNT == _learnt(make())
    outs.append(run(pipe, "first pass after forget()"))
    if family == "ur10_fused_native":
        assert pipe.fused_passes == 4 and pipe.prefix_passes == 2
    for out in outs[1:]:
        for key in ("idx_e", "idx_base", "params_base"):
            assert out[key] == outs[0][key], key
    load(pipe, 6)
    run(pipe, "first pass on fresh samples")
