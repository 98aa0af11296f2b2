"""GPU suite: the device front end of the real-data chain -- figh_medfilt_cols, figh_joint_difference,
figh_gradient_cols and the Python functions on top of them -- against the references of tests/differentiation_common.py.
The median, the plain-joint difference and the gradient are compared BIT FOR BIT; the SO(2) / SE(3) logarithms entry by
entry against the long-double restatement, |device - reference| <= C_TOL S.  Every device output is pre-filled with the
module's sentinel, so padding and spare rows are asserted untouched."""
import os
import warnings

import numpy as np
import pytest

import differentiation_common as dc
from conftest import ROOT, Golden

pytestmark = pytest.mark.gpu

TS = 0.01


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


def _upload(lib, X, ld=None, spare_rows=0, fill=np.nan):
    """X in a rows + spare_rows by ld device buffer, everything outside X set to ``fill``."""
    rows, cols = X.shape
    ld = cols if ld is None else ld
    full = np.full((rows + spare_rows, ld), fill)
    full[:rows, :cols] = X
    return lib.DeviceArray.from_host(full.reshape(-1))


def _sentinel(lib, rows, ld):
    return lib.DeviceArray.from_host(np.full(rows * ld, dc.SENTINEL))


def _download(buf, rows, ld):
    return buf.to_host().reshape(rows, ld)


# ---------------------------------------------------------------------------------------------------------------- medfilt
def _medfilt_data(rng, L, cols, nblocks, kind):
    X = rng.normal(size=(L * nblocks, cols))
    if kind == "ties":
        X = np.round(X * 2) / 2
    elif kind == "inf":
        X[rng.random(X.shape) < 0.1] = np.inf
        X[rng.random(X.shape) < 0.1] = -np.inf
    elif kind == "big":
        X *= 2.0 ** 40
    elif kind == "tiny":
        X *= 2.0 ** -40
    for b in range(nblocks):  # neighbours of a block boundary are far from the zero padding: bleeding moves the median
        X[b * L:(b + 1) * L] += (100.0 if kind in ("plain", "ties") else 0.0) * (b + 1)
    return X


@pytest.mark.parametrize("k", dc.MEDFILT_SIZES)
def test_medfilt_bit_equal_to_scipy(lib, k):
    from scipy import signal
    rng = np.random.default_rng(100 + k)
    kinds = ("plain", "ties", "inf", "big", "tiny")
    case = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # SciPy: "kernel_size exceeds volume extent" -- the zero padding under test
        for L in dc.GPU_MEDFILT_LENGTHS(k):
            for cols in dc.GPU_MEDFILT_COLS:
                for nblocks in (1, 3):
                    kind = kinds[case % len(kinds)]
                    case += 1
                    X = _medfilt_data(rng, L, cols, nblocks, kind)
                    rows = L * nblocks
                    ldx, ldy = cols + (case % 3), cols + ((case + 1) % 3)
                    d_x, d_y = _upload(lib, X, ldx), _sentinel(lib, rows + 1, ldy)
                    lib.medfilt_cols(d_x.ptr, rows, cols, ldx, nblocks, k, d_y.ptr, ldy)
                    Y = _download(d_y, rows + 1, ldy)
                    want = dc.medfilt_blocks_emul(X, k, nblocks)
                    assert np.array_equal(Y[:rows, :cols], want), (k, L, cols, nblocks, kind)
                    assert np.all(Y[:rows, cols:] == dc.SENTINEL) and np.all(Y[rows] == dc.SENTINEL)
                    for b in range(nblocks):  # SciPy itself, sequence by sequence (a sample of the columns of wide cases)
                        for c in sorted({0, cols // 2, cols - 1}):
                            seq = X[b * L:(b + 1) * L, c]
                            assert np.array_equal(Y[b * L:(b + 1) * L, c], signal.medfilt(seq, k))
                    if nblocks == 3 and 3 <= k <= 2 * L and kind in ("plain", "ties"):  # (a window wider than that is mostly padding)
                        assert not np.array_equal(want, dc.medfilt_blocks_emul(X, k, 1)), "the data cannot show bleeding"


def test_medfilt_refusals_launch_nothing(lib):
    X = np.random.default_rng(1).normal(size=(12, 4))
    d_x, d_y = _upload(lib, X), _sentinel(lib, 12, 4)
    for args in ((12, 4, 4, 1, 4, 4), (12, 4, 4, 1, 65, 4), (12, 4, 4, 1, 0, 4), (12, 4, 3, 1, 3, 4), (12, 4, 4, 1, 3, 3),
                 (12, 4, 4, 5, 3, 4)):
        rows, cols, ldx, nb, k, ldy = args
        with pytest.raises(lib.FighError) as e:
            lib.medfilt_cols(d_x.ptr, rows, cols, ldx, nb, k, d_y.ptr, ldy)
        assert e.value.code == lib.ERR_INVALID
    assert np.all(d_y.to_host() == dc.SENTINEL)
    from figaroh_plus_amd.identification.identification_tools import median_filter_columns
    with pytest.raises(ValueError, match="Each element of kernel_size should be odd."):
        median_filter_columns(X, 4)


# ------------------------------------------------------------------------------------------------- plain-joint difference
@pytest.mark.parametrize("name", ["ur10", "tx40"])
def test_plain_joint_difference_bit_equal_to_numpy(lib, name):
    model = dc.get_model(name)
    handle = lib.ModelHandle(model.to_flat())
    tile = lib.joint_difference_tile(model.nq, model.nv)
    for npairs in dc.gpu_plain_npairs(tile):
        N = npairs + 1
        q, dt = dc.gpu_plain_case(model, npairs)
        d_q = _upload(lib, q, spare_rows=1)  # row N is all NaN: a read one row too far poisons the output
        d_dt = lib.DeviceArray.from_host(dt)
        for form in dc.GPU_DT_FORMS:
            d_dq = _sentinel(lib, npairs + 1, model.nv)
            lib.joint_difference(handle, N, d_q.ptr, TS, d_dt.ptr if form == "dt" else None, d_dq.ptr)
            got = _download(d_dq, npairs + 1, model.nv)
            want = np.diff(q, axis=0) / (TS if form == "ts" else dt[:, None])
            assert np.array_equal(got[:npairs], want), (name, npairs, form)
            assert np.array_equal(got[:npairs], dc.simple_difference_emul(q, TS if form == "ts" else dt))
            assert np.all(got[npairs] == dc.SENTINEL)


# --------------------------------------------------------------------------------------------------------------- gradient
def test_gradient_bit_equal_to_numpy(lib):
    rng = np.random.default_rng(6)
    cols = 7
    for rows in (2, 3, 64, 65, 4097):
        F = rng.normal(size=(rows, cols)) * 2.0 ** rng.integers(-20, 20, size=cols)
        hrow = rng.uniform(0.005, 0.02, size=rows)
        d_h = lib.DeviceArray.from_host(hrow)
        for ld, ldg in ((cols, cols), (cols + 2, cols + 3)):
            d_f = _upload(lib, F, ld)
            for nactive in (0, cols - 1, cols):
                for per_row in (False, True):
                    d_g = _sentinel(lib, rows + 1, ldg)
                    lib.gradient_cols(d_f.ptr, rows, cols, ld, nactive, TS, d_h.ptr if per_row else None, d_g.ptr, ldg)
                    G = _download(d_g, rows + 1, ldg)
                    h = hrow if per_row else TS
                    for c in range(nactive):
                        assert np.array_equal(G[:rows, c], np.gradient(F[:, c], edge_order=1) / h), (rows, c, nactive, per_row)
                    assert np.array_equal(G[:rows, :cols], _gradient_want(F, h, nactive))
                    quiet = G[:rows, nactive:cols]
                    assert np.all(quiet == 0.0) and not np.any(np.signbit(quiet))  # +0.0, bit for bit
                    assert np.all(G[:rows, cols:] == dc.SENTINEL) and np.all(G[rows] == dc.SENTINEL)
    d_f, d_g = _upload(lib, np.ones((1, cols))), _sentinel(lib, 1, cols)
    with pytest.raises(lib.FighError) as e:
        lib.gradient_cols(d_f.ptr, 1, cols, cols, cols, TS, None, d_g.ptr, cols)
    assert e.value.code == lib.ERR_INVALID and np.all(d_g.to_host() == dc.SENTINEL)


def _gradient_want(F, h, nactive):
    G = np.zeros_like(F)
    for c in range(nactive):
        G[:, c] = dc.gradient_emul(F[:, c]) / h
    return G


# ------------------------------------------------------------------------------------------- free-flyer and continuous joints
@pytest.mark.parametrize("name", dc.GPU_DIFF_MODELS)
def test_logarithms_entry_by_entry(lib, name):
    worst = {}
    for npairs in dc.GPU_DIFF_NPAIRS:
        model, q, tags = dc.gpu_diff_case(name, npairs)
        handle = lib.ModelHandle(model.to_flat())
        special = dc.special_mask(model)
        N = npairs + 1
        dt = np.random.default_rng(npairs).uniform(0.005, 0.02, size=npairs)
        d_q, d_dt = _upload(lib, q, spare_rows=1), lib.DeviceArray.from_host(dt)
        for form in dc.GPU_DT_FORMS:
            div = TS if form == "ts" else dt
            d_dq = _sentinel(lib, npairs + 1, model.nv)
            lib.joint_difference(handle, N, d_q.ptr, TS, d_dt.ptr if form == "dt" else None, d_dq.ptr)
            got = _download(d_dq, npairs + 1, model.nv)
            assert np.all(got[npairs] == dc.SENTINEL)
            got = got[:npairs]
            ref, S, _ = dc.reference_rows(model, q, div)
            assert np.array_equal(got[:, ~special], dc.plain_difference_emul(model, q, div)[:, ~special])  # same launch
            err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
            for i, tag in enumerate(tags):
                if tag == "identical":
                    assert np.all(got[i, special] == 0.0), (name, npairs, form, i)
                ratio = float((err[i, special] / np.where(S[i, special] > 0, S[i, special], np.inf)).max())
                worst[tag or "between"] = max(worst.get(tag or "between", 0.0), ratio)
            print("%s N-1=%d %s: largest |device - long double| / S = %.4f" % (name, npairs, form,
                                                                                  (err[:, special] / np.maximum(S[:, special], 1e-300)).max()))
            bad = err[:, special] > dc.C_TOL * S[:, special]
            assert not bad.any(), (name, npairs, form, np.argwhere(bad)[:5], worst)
    print("%s: largest ratio per regime %s (C_TOL = %g)" % (name, {k: round(v, 4) for k, v in sorted(worst.items())}, dc.C_TOL))


# -------------------------------------------------------------------------------------------- the reference's own output
def test_reference_fixture_through_the_device_path(lib):
    from figaroh_plus_amd.device import GpuMatrix
    from figaroh_plus_amd.identification.identification_tools import calculate_first_second_order_differentiation
    z = np.load(os.path.join(ROOT, "tests", "golden", "human_differentiation.npz"))
    model = dc.get_model("human")
    param = {"is_joint_torques": False, "is_external_wrench": True, "ts": float(z["ts"])}
    for dt, kdq, kddq in ((None, "dq", "ddq"), (z["dt"], "dq_dt", "ddq_dt")):
        q, dq, ddq = calculate_first_second_order_differentiation(model, GpuMatrix.from_host(z["q"]), param, dt=dt)
        assert all(isinstance(x, GpuMatrix) for x in (q, dq, ddq))
        assert np.array_equal(q.numpy(), z["q_out"])
        assert np.abs(dq.numpy() - z[kdq]).max() <= 1e-12 * np.abs(z[kdq]).max()
        assert np.abs(ddq.numpy() - z[kddq]).max() <= 1e-12 * np.abs(z[kddq]).max()
    # param["device_resident"] takes the same path from a host array
    q2, dq2, _ = calculate_first_second_order_differentiation(model, z["q"], dict(param, device_resident=True), dt=z["dt"])
    assert isinstance(q2, GpuMatrix) and np.array_equal(dq2.numpy(), dq.numpy())
    # fixed base: the reference's range(model.nq - 1) leaves the last joint's acceleration at +0.0
    ur10 = dc.get_model("ur10")
    qu, dtu = dc.gpu_plain_case(ur10, 65)  # (the case the host suite plants its errors in)
    pu = {"is_joint_torques": True, "is_external_wrench": False, "ts": TS}
    for dt in (None, dtu):
        div = TS if dt is None else dt
        hq, hdq, hddq = calculate_first_second_order_differentiation(ur10, qu, pu, dt=dt)
        gq, gdq, gddq = calculate_first_second_order_differentiation(ur10, GpuMatrix.from_host(qu), pu, dt=dt)
        assert np.array_equal(gq.numpy(), hq) and np.array_equal(gdq.numpy(), hdq) and np.array_equal(gddq.numpy(), hddq)
        step = dc.simple_difference_emul(qu, div)
        assert np.array_equal(gdq.numpy(), step[:-1])
        assert np.array_equal(gddq.numpy(), dc.gradient_cols_emul(step, div, 5)[:-1])
        last = gddq.numpy()[:, 5]
        assert np.all(last == 0.0) and not np.any(np.signbit(last))


# ---------------------------------------------------------------------------------------------------------------- residency
def _raw_positions(model, N, seed):
    """Smooth joint motion at 100 Hz with measurement noise and a few outliers (what the median filter is there for)."""
    rng = np.random.default_rng(seed)
    t = np.arange(N) * TS
    q = np.zeros((N, model.nq))
    for j in model.joints[1:]:
        iq = j.idx_q
        if j.jtype in (0, 1):
            q[:, iq] = sum(rng.uniform(0.2, 0.6) * np.sin(2 * np.pi * f * t + rng.uniform(0, 6)) for f in (0.3, 0.7, 1.1))
        elif j.jtype == 3:
            q[:, iq:iq + 3] = np.c_[0.3 * np.sin(0.5 * t), 0.2 * np.cos(0.4 * t), 1.0 + 0.1 * np.sin(0.9 * t)]
            ang = 0.4 * np.sin(0.6 * t)
            ax = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
            q[:, iq + 3:iq + 6] = np.sin(ang / 2)[:, None] * ax
            q[:, iq + 6] = np.cos(ang / 2)
    q += 1e-4 * rng.normal(size=q.shape)
    spikes = rng.choice(N, 20, replace=False)
    q[spikes, rng.integers(0, model.nq, size=20)] += 0.5
    return q


class _NoTransfers:
    """DeviceArray.to_host / from_host raise while this is active: nothing may cross PCIe."""

    def __init__(self, monkeypatch, lib):
        self.mp, self.lib = monkeypatch, lib

    def __enter__(self):
        def boom(*a, **k):
            raise AssertionError("a host transfer inside the resident chain")
        self.mp.setattr(self.lib.DeviceArray, "to_host", boom)
        self.mp.setattr(self.lib.DeviceArray, "from_host", classmethod(boom))

    def __exit__(self, *exc):
        self.mp.undo()
        return False


def _host_chain(model, raw, param):
    from figaroh_plus_amd.identification import identification_tools as it
    x = it.median_filter_columns(raw, 5)
    x = it.low_pass_filter_data(x, param)
    return it.calculate_first_second_order_differentiation(model, x, param)


def _device_chain(raw_dev, model, param):
    from figaroh_plus_amd.identification import identification_tools as it
    x = it.median_filter_columns(raw_dev, 5)
    x = it.low_pass_filter_data(x, param)
    return it.calculate_first_second_order_differentiation(model, x, param)


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def test_resident_chain_ur10(lib, monkeypatch):
    from figaroh_plus_amd.device import GpuMatrix
    from figaroh_plus_amd.identification import identification_tools as it
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from scipy import signal
    g = Golden("cfg2_ur10")
    robot = g.robot()
    model = robot.model
    param = dict(g.param, ts=TS, cut_off_frequency_butterworth=10.0)
    raw = _raw_positions(model, 4200 + 2 + 50, 31)
    q, v, a = _host_chain(model, raw, param)
    assert q.shape == (4200, 6)
    # host-array calls return what the untouched code paths return
    assert np.array_equal(it.median_filter_columns(raw, 5), np.column_stack([signal.medfilt(raw[:, c], 5) for c in range(6)]))
    assert np.array_equal(it.gradient_columns(v, TS)[:, :3], np.column_stack([np.gradient(v[:, c], edge_order=1) / TS
                                                                             for c in range(3)]))
    step = np.diff(raw, axis=0) / TS
    hq, hdq, hddq = it.calculate_first_second_order_differentiation(model, raw, param)
    assert np.array_equal(hq, raw[:-2]) and np.array_equal(hdq, step[:-1])
    assert np.array_equal(hddq[:, :5], np.column_stack([np.gradient(step[:, c], edge_order=1) / TS for c in range(5)])[:-1])

    def run_host(tau):
        pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), fuse=False)
        pipe.set_samples(q, v, a, tau)
        return pipe
    first = run_host(None)
    first.set_tau_from_parameters(g.phi_ref(), noise_std=0.05, seed=3)
    tau = first.d_tau.to_host()
    out_a, out_b = run_host(tau).run(), run_host(tau).run()

    d_raw, d_tau = GpuMatrix.from_host(raw), lib.DeviceArray.from_host(tau)
    pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std(), fuse=False)
    with _NoTransfers(monkeypatch, lib):
        dq_, dv_, da_ = _device_chain(d_raw, model, param)
        pipe.set_samples(dq_, dv_, da_, d_tau)
    out = pipe.run()
    for got, want in ((dq_, q), (dv_, v), (da_, a)):  # the inputs of K1 are bit-identical to the host chain's
        assert np.array_equal(got.numpy(), want)
    assert set(out) == set(out_a)
    loose = [key for key in out_a if not _same(out_a[key], out_b[key])]
    print("outputs two host-chain runs do not reproduce bit for bit:", loose)
    assert set(loose) <= {"col_norm", "phi_ls", "phi_b"}, loose  # the outputs the suite has a tolerance for (checked below)
    for key in out_a:
        if key not in loose:  # reproduced bit for bit by the host chain: bit for bit here too
            assert _same(out[key], out_a[key]), key
    assert np.abs(out["col_norm"] - out_a["col_norm"]).max() <= 1e-12 * out_a["col_norm"].max()
    assert np.abs(out["phi_ls"] - out_a["phi_ls"]).max() <= 1e-6 * np.abs(out_a["phi_ls"]).max()
    assert np.abs(out["phi_b"] - out_a["phi_b"]).max() <= 1.5e-6 * max(1.0, np.abs(out_a["phi_b"]).max())


def test_resident_chain_human(lib, monkeypatch):
    from figaroh_plus_amd.device import GpuMatrix
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    g = Golden("cfg5_human")
    robot = g.robot()
    model = robot.model
    param = dict(g.param, ts=TS, cut_off_frequency_butterworth=10.0)
    raw = _raw_positions(model, 600 + 2 + 50, 32)
    q, v, a = _host_chain(model, raw, param)
    assert q.shape == (600, model.nq) and v.shape == (600, model.nv)
    ref = IdentificationPipeline(robot, g.param, params_std=g.params_std())
    ref.set_samples(q, v, a)
    ref.set_tau_from_parameters(g.phi_ref(), noise_std=0.05, seed=4)
    tau = ref.d_tau.to_host()
    ref.set_samples(q, v, a, tau)
    want = ref.run()

    d_raw, d_tau = GpuMatrix.from_host(raw), lib.DeviceArray.from_host(tau)
    pipe = IdentificationPipeline(robot, g.param, params_std=g.params_std())
    with _NoTransfers(monkeypatch, lib):
        dq_, dv_, da_ = _device_chain(d_raw, model, param)
        before = [lib.DeviceArray((x.rows * x.cols,), np.float64) for x in (dq_, dv_, da_)]
        for b, x in zip(before, (dq_, dv_, da_)):
            lib.check(lib.load().figh_memcpy_d2d(b.ptr, x.ptr, 8 * x.rows * x.cols))
        pipe.set_samples(dq_, dv_, da_, d_tau)  # tree model: the samples are repacked, the caller's matrices stay
    for b, x in zip(before, (dq_, dv_, da_)):
        assert getattr(x.buf, "base", x.buf).ptr is not None  # (a window's owner is its base: DeviceArray.free clears ptr)
        assert np.array_equal(x.numpy().reshape(-1), b.to_host())
    assert np.array_equal(dq_.numpy(), q)
    special = dc.special_mask(model)
    assert np.array_equal(dv_.numpy()[:, ~special], v[:, ~special])
    assert np.abs(dv_.numpy() - v).max() <= 1e-12 * np.abs(v).max()
    out = pipe.run()
    assert out["idx_e"] == want["idx_e"] and out["idx_base"] == want["idx_base"]
    assert out["params_base"] == want["params_base"]
    assert np.abs(out["phi_ls"] - want["phi_ls"]).max() <= 1e-6 * np.abs(want["phi_ls"]).max()
    assert np.abs(out["phi_b"] - want["phi_b"]).max() <= 1.5e-6 * max(1.0, np.abs(want["phi_b"]).max())
