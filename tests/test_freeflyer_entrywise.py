"""GPU suite of the free-flyer real-data entries (figh_quat_log, figh_rotvec_to_quat, figh_wrench_transport) and the public
functions on top of them: every entry against the exact restatement of freeflyer_common at C_TOL_*, for N around the wave
size and in every regime; padded buffers with their borders intact; the exact alias of the exponential; bit equality with the
mirror where no library call is involved; resident in, resident out; refusals that launch nothing; and the human pipeline fed
with a wrench that went to the world frame and back on the device."""
import numpy as np
import pytest

import freeflyer_common as fc
from figaroh_plus_amd.device import GpuMatrix
from figaroh_plus_amd.identification import identification_tools as it

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


_handles = {}


def _handle(lib, name):
    if name not in _handles:
        _handles[name] = lib.ModelHandle(fc.transport_case(name)[0].to_flat())
    return _handles[name]


def _padded_input(lib, x, ld):
    """x (N, w) as rows of a NaN-filled (N, ld) buffer: whatever is read outside the columns poisons the result."""
    full = np.full((len(x), ld), np.nan)
    full[:, :x.shape[1]] = x
    return lib.DeviceArray.from_host(full.reshape(-1))


def _sentinel(lib, rows, ld):
    return lib.DeviceArray.from_host(np.full(rows * ld, fc.SENTINEL))


def _read_padded(buf, N, width, ld, spare):
    """The (N, width) window of a sentinel-filled (N + spare, ld) buffer, after checking that nothing else was written."""
    full = buf.to_host().reshape(N + spare, ld)
    assert np.all(full[:N, width:] == fc.SENTINEL) and np.all(full[N:] == fc.SENTINEL)
    assert not np.any(full[:N, :width] == fc.SENTINEL)
    return full[:N, :width]


# ------------------------------------------------------------------------------------------------------------------- log
@pytest.mark.parametrize("regime", fc.LOG_REGIMES)
def test_quat_log_entrywise(lib, regime, record_property):
    quat, ex = fc.log_inputs(regime), fc.log_reference(regime)
    worst = 0.0
    for N in fc.GPU_N:
        d_q, d_r = _padded_input(lib, quat[:N], 9), _sentinel(lib, N + 2, 5)
        lib.quat_log(d_q.ptr, N, 9, d_r.ptr, 5)
        got = _read_padded(d_r, N, 3, 5, 2)
        r, zeros_ok = fc.ratio(got, ex.rows(N))
        worst = max(worst, r)
        assert zeros_ok and r <= fc.C_TOL_LOG, (N, r)
        if regime == "n_0":
            assert not np.any(np.signbit(got))
        d_q2, d_r2 = lib.DeviceArray.from_host(quat[:N].reshape(-1)), _sentinel(lib, N, 3)
        lib.quat_log(d_q2.ptr, N, 4, d_r2.ptr, 3)  # dense leading dimensions, and a second call: the same bits
        assert np.array_equal(d_r2.to_host().reshape(N, 3), got)
    record_property("ratio", worst)
    print("device log %-12s ratio %.4f" % (regime, worst))


# ------------------------------------------------------------------------------------------------------------------- exp
@pytest.mark.parametrize("regime", fc.EXP_REGIMES)
def test_rotvec_to_quat_entrywise(lib, regime, record_property):
    (rotvec, ref), ex = fc.exp_inputs(regime), fc.exp_reference(regime)
    worst = 0.0
    for N in fc.GPU_N:
        d_r, d_f, d_o = _padded_input(lib, rotvec[:N], 4), _padded_input(lib, ref[:N], 9), _sentinel(lib, N + 2, 6)
        lib.rotvec_to_quat(d_r.ptr, N, 4, d_f.ptr, 9, d_o.ptr, 6)
        got = _read_padded(d_o, N, 4, 6, 2)
        r, zeros_ok = fc.ratio(got, ex.rows(N))
        worst = max(worst, r)
        assert zeros_ok and r <= fc.C_TOL_EXP, (N, r)
        # the exact alias: the output is the reference itself (same pointer, same leading dimension), a window of a q-like
        # buffer whose other columns must survive
        full = np.full((N + 1, 9), fc.SENTINEL)
        full[:N, 3:7] = ref[:N]
        d_q = lib.DeviceArray.from_host(full.reshape(-1))
        lib.rotvec_to_quat(d_r.ptr, N, 4, d_q.ptr + 8 * 3, 9, d_q.ptr + 8 * 3, 9)
        after = d_q.to_host().reshape(N + 1, 9)
        assert np.array_equal(after[:N, 3:7], got)
        assert np.all(after[:N, :3] == fc.SENTINEL) and np.all(after[:N, 7:] == fc.SENTINEL) and np.all(after[N] == fc.SENTINEL)
    record_property("ratio", worst)
    print("device exp %-20s ratio %.4f" % (regime, worst))


# ------------------------------------------------------------------------------------------------------------- transport
@pytest.mark.parametrize("name", fc.TRANSPORT_CASES)
def test_wrench_transport_entrywise(lib, name, record_property):
    model, joint = fc.transport_case(name)
    q, F = fc.transport_inputs(name)
    h = _handle(lib, name)
    ldq = model.nq + 2
    worst = 0.0
    for N in fc.GPU_N:
        d_q = _padded_input(lib, q[:N], ldq)
        for inverse in (False, True):
            ex = fc.transport_reference(name, inverse).rows(N)
            mirror = it.transport_wrench_mirror(model, q[:N], F[:N], joint, inverse, "sample", "sample")
            for lin in ("sample", "stacked"):
                d_F = lib.DeviceArray.from_host(fc.to_layout(F[:N], lin).reshape(-1))
                for lout in ("sample", "stacked"):
                    d_o = _sentinel(lib, 6 * N + 7, 1)
                    lib.wrench_transport(h, joint, N, d_q.ptr, ldq, d_F.ptr, lin, inverse, d_o.ptr, lout)
                    full = d_o.to_host()
                    assert np.all(full[6 * N:] == fc.SENTINEL) and not np.any(full[:6 * N] == fc.SENTINEL)
                    got = fc.from_layout(full[:6 * N], N, lout)
                    r, zeros_ok = fc.ratio(got, ex)
                    worst = max(worst, r)
                    assert zeros_ok and r <= fc.C_TOL_TRN, (N, inverse, lin, lout, r)
                    if name == "human_root":
                        # a free-flyer behind a constant placement: no library call on the path, contraction is off
                        assert np.array_equal(got, mirror), (N, inverse, lin, lout)
    record_property("ratio", worst)
    print("device transport %-22s ratio %.4f" % (name, worst))


def test_wrench_transport_many_tiles_and_universe(lib):
    """More tiles than one pass of the grid's waves is not needed for correctness, but more than one workgroup is: 1000
    samples are 16 tiles in 4 workgroups, the last tile partial.  Joint 0 is the identity."""
    name = "placed_tree_freeflyer"
    model, joint = fc.transport_case(name)
    N = 1000
    q = fc.configurations(model, N, 77)
    F = np.random.default_rng(78).uniform(-50, 50, (N, 6))
    d_q, d_F = lib.DeviceArray.from_host(q.reshape(-1)), lib.DeviceArray.from_host(F.reshape(-1))
    for inverse in (False, True):
        mirror = it.transport_wrench_mirror(model, q, F, joint, inverse, "sample", "sample")
        for lout in ("sample", "stacked"):
            d_o = _sentinel(lib, 6 * N + 3, 1)
            lib.wrench_transport(_handle(lib, name), joint, N, d_q.ptr, model.nq, d_F.ptr, "sample", inverse, d_o.ptr, lout)
            full = d_o.to_host()
            assert np.all(full[6 * N:] == fc.SENTINEL)
            got = fc.from_layout(full[:6 * N], N, lout)
            assert np.abs(got - mirror).max() <= 1e-12 * np.abs(mirror).max()
    d_o = _sentinel(lib, 6 * N, 1)
    lib.wrench_transport(_handle(lib, name), 0, N, d_q.ptr, model.nq, d_F.ptr, "sample", False, d_o.ptr, "stacked")
    assert np.array_equal(fc.from_layout(d_o.to_host(), N, "stacked"), F)


# ----------------------------------------------------------------------------------------------------- public functions
def _param():
    return {"ts": 0.01, "cut_off_frequency_butterworth": 15.0}


def _trajectory(model, n, seed=5):
    return fc.mocap_like(model, n, seed)


def test_public_functions_host_in_host_out(lib):
    quat = fc.log_inputs("generic")[:130]
    rv = it.quaternion_log(quat)
    assert isinstance(rv, np.ndarray) and fc.ratio(rv, fc.log_reference("generic").rows(130))[0] <= fc.C_TOL_LOG
    rotvec, ref = (x[:130] for x in fc.exp_inputs("generic_vector_case"))
    out = it.rotation_vector_to_quaternion(rotvec, ref)
    assert isinstance(out, np.ndarray) and fc.ratio(out, fc.exp_reference("generic_vector_case").rows(130))[0] <= fc.C_TOL_EXP
    model, joint = fc.transport_case("human_root")
    q, F = (x[:130] for x in fc.transport_inputs("human_root"))
    tau = it.transport_wrench(model, q, F, "root_joint", inverse=True)  # the script's call: sample in, stacked out
    assert isinstance(tau, np.ndarray) and tau.shape == (6 * 130,)
    assert np.array_equal(tau, it.transport_wrench_mirror(model, q, F, "root_joint", inverse=True))
    q_m = _trajectory(model, 171)
    got, want = it.filter_free_flyer(model, q_m, _param()), it.filter_free_flyer_mirror(model, q_m, _param())
    assert isinstance(got, np.ndarray) and got.shape == want.shape == (121, model.nq)
    # (the filter is SciPy's bit for bit; the quaternion columns go through atan2, sincos and sqrt of two libraries)
    assert np.abs(got - want).max() <= 1e-12
    plain = [c for c in range(model.nq) if not 3 <= c < 7]
    assert np.array_equal(got[:, plain], want[:, plain])


def test_resident_in_resident_out_without_download(lib, monkeypatch):
    """GpuMatrix / device vector in: the result stays in HBM and not one byte comes back to the host on the way."""
    model, joint = fc.transport_case("human_root")
    n = 171
    q_m = _trajectory(model, n)
    want_q = it.filter_free_flyer(model, q_m, _param())
    F = np.random.default_rng(3).uniform(-100, 100, (n - 50, 6))
    want_tau = it.transport_wrench(model, want_q, F, "root_joint", inverse=True)
    want_rv = it.quaternion_log(q_m[:, 3:7])
    want_quat = it.rotation_vector_to_quaternion(want_rv, q_m[:, 3:7])
    d_q, d_F = GpuMatrix.from_host(q_m), GpuMatrix.from_host(F)
    raw, down = lib.load(), []
    d2h = raw.figh_memcpy_d2h

    def recording_d2h(dst, src, nbytes):
        down.append(int(nbytes))
        return d2h(dst, src, nbytes)

    with monkeypatch.context() as mp:
        mp.setattr(raw, "figh_memcpy_d2h", recording_d2h)
        q_f = it.filter_free_flyer(model, d_q, _param())
        tau = it.transport_wrench(model, q_f, d_F, "root_joint", inverse=True)
        world = it.transport_wrench(model, q_f, tau, "root_joint", inverse=False, layout_in="stacked", layout_out="sample")
        window = GpuMatrix(it._DevView(d_q.buf, 8 * 3), n, 4, model.nq)
        rv = it.quaternion_log(window)
        quat = it.rotation_vector_to_quaternion(rv, window)
    assert down == []
    assert isinstance(q_f, GpuMatrix) and isinstance(tau, lib.DeviceArray) and isinstance(world, GpuMatrix)
    assert isinstance(rv, GpuMatrix) and isinstance(quat, GpuMatrix)
    assert np.array_equal(q_f.numpy(), want_q) and np.array_equal(tau.to_host(), want_tau)
    assert np.array_equal(rv.numpy(), want_rv) and np.array_equal(quat.numpy(), want_quat)
    assert np.abs(world.numpy() - F).max() <= 1e-12 * np.abs(F).max()
    assert np.array_equal(d_q.numpy(), q_m)  # the raw configurations are read, never written


# ------------------------------------------------------------------------------------------------------------- refusals
def test_freeflyer_refusals_launch_nothing(lib):
    name = "human_root"
    model, joint = fc.transport_case(name)
    N = 9
    q, F = (x[:N] for x in fc.transport_inputs(name))
    h = _handle(lib, name)
    d_q, d_F = lib.DeviceArray.from_host(q.reshape(-1)), lib.DeviceArray.from_host(F.reshape(-1))
    d_quat = lib.DeviceArray.from_host(fc.log_inputs("generic")[:N].reshape(-1))
    d_rv = lib.DeviceArray.from_host(fc.exp_inputs("generic_scalar_case")[0][:N].reshape(-1))
    d_o = _sentinel(lib, 6 * N, 1)

    def log(n=N, ldq=4, ldr=3, out=None):
        lib.quat_log(d_quat.ptr, n, ldq, d_o.ptr if out is None else out, ldr)

    def exp(n=N, ldr=3, ldf=4, ldo=4, out=None):
        lib.rotvec_to_quat(d_rv.ptr, n, ldr, d_quat.ptr, ldf, d_o.ptr if out is None else out, ldo)

    def trn(n=N, j=joint, ldq=model.nq, lin="sample", lout="stacked", out=None, raw_layout=None):
        if raw_layout is not None:
            lib.check(lib.load().figh_wrench_transport(h.handle, j, n, d_q.ptr, ldq, d_F.ptr, raw_layout[0], 0, d_o.ptr,
                                                       raw_layout[1]))
        else:
            lib.wrench_transport(h, j, n, d_q.ptr, ldq, d_F.ptr, lin, False, d_o.ptr if out is None else out, lout)

    cases = [(log, dict(n=0)), (log, dict(ldq=3)), (log, dict(ldr=2)), (log, dict(out=d_quat.ptr + 8)),
             (exp, dict(n=0)), (exp, dict(ldr=2)), (exp, dict(ldf=3)), (exp, dict(ldo=3)), (exp, dict(out=d_quat.ptr + 8)),
             (exp, dict(out=d_quat.ptr, ldo=5, ldf=4)), (exp, dict(out=d_rv.ptr)),
             (trn, dict(n=0)), (trn, dict(ldq=model.nq - 1)), (trn, dict(j=model.njoints)), (trn, dict(j=-1)),
             (trn, dict(raw_layout=(2, 1))), (trn, dict(raw_layout=(0, -1))), (trn, dict(out=d_F.ptr + 8 * 6))]
    lib.profile_enable(level=2)
    try:
        lib.profile_reset()
        for call, kw in cases:
            with pytest.raises(lib.FighError) as e:
                call(**kw)
            assert e.value.code == lib.ERR_INVALID and len(str(e.value)) > 30, kw
        for fam in ("quat_log", "rotvec_to_quat", "wrench_transport"):
            assert lib.profile_get(fam)[0] == 0, fam
        assert np.all(d_o.to_host() == fc.SENTINEL)
        assert np.array_equal(d_quat.to_host().reshape(N, 4), fc.log_inputs("generic")[:N])
        log()
        exp()
        trn()
        for fam in ("quat_log", "rotvec_to_quat", "wrench_transport"):
            assert lib.profile_get(fam)[0] == 1, fam
        assert not np.any(d_o.to_host() == fc.SENTINEL)
    finally:
        lib.profile_enable(False)


# ----------------------------------------------------------------------------------------------------------- end to end
def test_human_pipeline_takes_the_transported_wrench(lib):
    """The human fixture at its own sample count: tau = W phi is computed resident, carried to the world frame and back to the
    pelvis on the device, and handed to the pipeline as a device vector.  run() returns the base parameters it returns for
    the untouched tau: the same columns, phi within the suite's 1e-6 (relative on the least-squares solution, and the
    both-rounded form of test_pipeline_matches_reference_outputs on the 6-decimal phi_b)."""
    from conftest import Golden
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.regressor import regressor_times_parameters

    g = Golden("cfg5_human")
    robot = g.robot()
    q, v, a = g["q_big"], g["v_big"], g["a_big"]
    N = len(q)
    d_tau = regressor_times_parameters(robot, q, v, a, dict(g.param, device_resident=True), g.phi_ref())
    assert isinstance(d_tau, lib.DeviceArray) and d_tau.size == 6 * N
    world = it.transport_wrench(robot.model, q, d_tau, "root_joint", inverse=False, layout_in="stacked", layout_out="sample")
    back = it.transport_wrench(robot.model, q, world, "root_joint", inverse=True, layout_in="sample", layout_out="stacked")
    assert isinstance(world, GpuMatrix) and isinstance(back, lib.DeviceArray)
    tau = d_tau.to_host()
    assert np.abs(back.to_host() - tau).max() <= 1e-12 * np.abs(tau).max()
    assert np.abs(world.numpy() - tau.reshape(6, N).T).max() > 1e-3 * np.abs(tau).max()  # (the world frame is another frame)
    outs = []
    for t in (d_tau, back):
        pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), coupling=g.coupling)
        pipe.set_samples(q, v, a, t)
        outs.append(pipe.run())
    ref, got = outs
    assert got["idx_e"] == ref["idx_e"] and got["idx_base"] == ref["idx_base"] and got["params_base"] == ref["params_base"]
    assert np.abs(got["phi_ls"] - ref["phi_ls"]).max() <= 1e-6 * np.abs(ref["phi_ls"]).max()
    assert np.abs(got["phi_b"] - ref["phi_b"]).max() <= 1.5e-6 * max(1.0, np.abs(ref["phi_b"]).max())
