"""GPU suite: figh_singular_values_batch (csrc/figh_singular.hip) against the long-double run of its NumPy mirror on the
graded matrices of tests/singular_common.py, value by value: |sigma_k - ref_k| <= C_SV (1 - 2^-11) r 2^-53 sigma_max.  Every
input has NaN below the diagonal and sentinels between the matrices of a padded stride; sigma and status are pre-filled with
sentinels, have a padded leading dimension and spare rows, and the padding is asserted untouched."""
import numpy as np
import pytest

import singular_common as sc

pytestmark = pytest.mark.gpu
STATUS_SENTINEL = -77


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


def _run(lib, mats, max_sweeps=sc.MAX_SWEEPS, pad=5, ld_pad=3, spare=2):
    """The raw entry on B matrices (B x r x r, NaN below the diagonal added here): ``pad`` sentinel doubles between the
    matrices, sigma rows of r + ld_pad doubles, ``spare`` rows behind sigma and status.  Returns (sigma (B, r) as written,
    status (B, 2)); the padding is checked here."""
    mats = sc.with_nan_below(np.asarray(mats, dtype=np.float64))
    B, r = mats.shape[0], mats.shape[-1]
    stride, ld = r * r + pad, r + ld_pad
    host = np.full((B, stride), sc.SENTINEL)
    host[:, :r * r] = mats.reshape(B, r * r)
    d_R = lib.DeviceArray.from_host(host.reshape(-1))
    d_sigma = lib.DeviceArray.from_host(np.full((B + spare) * ld, sc.SENTINEL))
    d_status = lib.DeviceArray.from_host(np.full(2 * (B + spare), STATUS_SENTINEL, dtype=np.int32))
    lib.singular_values_batch(d_R, B, r, stride, max_sweeps, d_sigma, ld, d_status)
    sigma = d_sigma.to_host().reshape(B + spare, ld)
    status = d_status.to_host().reshape(B + spare, 2)
    assert np.all(sigma[:B, r:] == sc.SENTINEL) and np.all(sigma[B:] == sc.SENTINEL)
    assert np.all(status[B:] == STATUS_SENTINEL)
    assert np.array_equal(d_R.to_host(), host.reshape(-1), equal_nan=True)  # the input is only read
    return sigma[:B, :r].copy(), status[:B].copy()


def _check(sigma, status, refs, tag):
    worst = 0.0
    for b, ref in enumerate(refs):
        assert status[b, 1] == 1 and 1 <= status[b, 0] <= sc.MAX_SWEEPS, (tag, b, status[b])
        assert np.isfinite(sigma[b]).all() and np.all(sigma[b] >= 0.0), (tag, b)
        worst = max(worst, sc.ratio_to_reference(sigma[b], ref))
    print("%s: largest ratio %.4f (bound %.4f), sweeps %s" % (tag, worst, sc.C_SV * (1 - 2.0 ** -11), status[:, 0].tolist()))
    assert worst <= sc.C_SV * (1 - 2.0 ** -11), (tag, worst)
    return worst


@pytest.mark.parametrize("r", sc.SIZES)
def test_singular_values_entrywise(lib, r):
    """B = 1 (each matrix alone) and B = 3 (the three ratios in one launch); two calls and copies of one matrix at different
    b give equal bits.  The float64 mirror states the kernel's operations in its order (the unit is compiled without
    contraction); whether the two agree to the bit is printed, not asserted."""
    from figaroh_plus_amd._host import jacobi_singular_values_mirror
    kinds = [k for rr, k in sc.cases() if rr == r]
    mats = np.stack([sc.matrix_of(r, k) for k in kinds])
    refs = [sc.reference(r, k) for k in kinds]
    sigma, status = _run(lib, mats)
    _check(sigma, status, refs, "r = %d, B = %d" % (r, len(kinds)))
    again, status2 = _run(lib, mats)
    assert np.array_equal(sigma, again) and np.array_equal(status, status2)
    for b in range(len(kinds)):
        s1, st1 = _run(lib, mats[b:b + 1], pad=0, ld_pad=0)
        assert np.array_equal(s1[0], sigma[b]) and np.array_equal(st1[0], status[b])
    mirror, sweeps, _ = jacobi_singular_values_mirror(sc.with_nan_below(mats))  # (for the record: no assertion hangs on it)
    print("float64 mirror: sweeps %s, bit-equal to the device %s" % (sweeps.tolist(), np.array_equal(mirror, sigma)))
    copies = np.stack([mats[-1], mats[0], mats[-1], mats[-1]])
    s4, st4 = _run(lib, copies)
    assert np.array_equal(s4[0], s4[2]) and np.array_equal(s4[0], s4[3]) and np.array_equal(s4[0], sigma[-1])
    assert np.array_equal(st4[0], st4[2]) and np.array_equal(st4[0], st4[3])


def test_singular_values_more_matrices_than_workgroups(lib):
    """B = 300 at r = 16 (more matrices than compute units) and, at r = 3, more matrices than the launch has workgroups
    (SINGULAR_VALUES_WGS_PER_CU per compute unit at most): the persistent loop.  The matrices repeat with period 3 or 4, so
    every copy must carry the bits of the first."""
    for r, B in ((16, 300), (3, lib.SINGULAR_VALUES_WGS_PER_CU * lib.device_info()["cu_count"] + 5)):
        kinds = [k for rr, k in sc.cases() if rr == r]
        base = np.stack([sc.matrix_of(r, k) for k in kinds])
        mats = base[np.arange(B) % len(kinds)]
        sigma, status = _run(lib, mats)
        first, first_status = _run(lib, base)
        _check(first, first_status, [sc.reference(r, k) for k in kinds], "r = %d, first %d of B = %d" % (r, len(kinds), B))
        assert np.array_equal(sigma, first[np.arange(B) % len(kinds)])
        assert np.array_equal(status, first_status[np.arange(B) % len(kinds)])


def test_singular_values_special_and_refusals(lib):
    sp = sc.special_cases()
    s, st = _run(lib, sp["zero"][None])
    assert np.all(s == 0.0) and not np.any(np.signbit(s)) and st.tolist() == [[1, 1]]
    s, st = _run(lib, sp["zero_column"][None])
    assert st[0, 1] == 1 and s[0, 1] == 0.0 and not np.signbit(s[0, 1]) and np.count_nonzero(s[0]) == 2
    assert np.allclose(np.sort(s[0])[::-1], np.linalg.svd(sp["zero_column"], compute_uv=False), rtol=1e-14, atol=0)
    s, st = _run(lib, sp["identity"][None])
    assert np.all(s == 1.0) and st.tolist() == [[1, 1]]
    # a matrix that does not converge ends by the sweep cap, beside one that does
    pair = np.stack([sp["nan"], sc.matrix_of(3, 1e3)])
    s, st = _run(lib, pair, max_sweeps=5)
    assert st[0].tolist() == [5, 0] and st[1, 1] == 1 and st[1, 0] <= 5
    assert sc.ratio_to_reference(s[1], sc.reference(3, 1e3)) <= sc.C_SV * (1 - 2.0 ** -11)

    r, B = 5, 2
    d_R = lib.DeviceArray.from_host(np.tile(np.eye(r).reshape(-1), B))
    d_sigma = lib.DeviceArray.from_host(np.full(B * r, sc.SENTINEL))
    d_status = lib.DeviceArray.from_host(np.full(2 * B, STATUS_SENTINEL, dtype=np.int32))

    def call(B=B, r=r, stride=r * r, max_sweeps=40, ld_sigma=r):
        lib.singular_values_batch(d_R, B, r, stride, max_sweeps, d_sigma, ld_sigma, d_status)

    cases = [("r 0", dict(r=0), lib.ERR_INVALID), ("B 0", dict(B=0), lib.ERR_INVALID),
             ("stride", dict(stride=r * r - 1), lib.ERR_INVALID), ("ld_sigma", dict(ld_sigma=r - 1), lib.ERR_INVALID),
             ("sweeps 0", dict(max_sweeps=0), lib.ERR_INVALID), ("sweeps 1001", dict(max_sweeps=1001), lib.ERR_INVALID),
             ("r 129", dict(r=129, stride=129 * 129, ld_sigma=129), lib.ERR_UNSUPPORTED)]
    lib.profile_enable(level=2)
    try:
        lib.profile_reset()
        for tag, kw, code in cases:
            with pytest.raises(lib.FighError) as e:
                call(**kw)
            assert e.value.code == code, tag
        assert lib.profile_get("singular_values_batch")[0] == 0
        assert np.all(d_sigma.to_host() == sc.SENTINEL) and np.all(d_status.to_host() == STATUS_SENTINEL)
        call()
        assert lib.profile_get("singular_values_batch")[0] == 1 and np.all(d_sigma.to_host() == 1.0)
    finally:
        lib.profile_enable(False)


def test_r_above_cap_takes_host_route(lib):
    """A synthetic r = 130 stack through singular_values_batch_device: bit for bit what singular_values_batch gives on the
    downloaded triangles, nothing launched, no fallback counted."""
    from figaroh_plus_amd import _host
    rng = np.random.default_rng(130)
    mats = np.triu(rng.normal(size=(4, 130, 130)))
    d_R = lib.DeviceArray.from_host(sc.with_nan_below(mats).reshape(-1))
    before = _host.device_singular_value_fallbacks
    lib.profile_enable(level=2)
    try:
        lib.profile_reset()
        got, sweeps, fallbacks = _host.singular_values_batch_device(d_R, 4, 130, return_status=True)
        assert lib.profile_get("singular_values_batch")[0] == 0
    finally:
        lib.profile_enable(False)
    assert np.array_equal(got, _host.singular_values_batch(mats)) and sweeps is None and fallbacks == 0
    assert _host.device_singular_value_fallbacks == before


def test_device_route_sorts_and_falls_back_per_matrix(lib):
    """singular_values_batch_device: descending rows within the bound; a matrix the kernel cannot finish within the cap is
    recomputed on the host from its own triangle and counted."""
    from figaroh_plus_amd import _host
    r = 17
    mats = np.stack([sc.matrix_of(r, k) for k in sc.RATIOS])
    d_R = lib.DeviceArray.from_host(sc.with_nan_below(mats).reshape(-1))
    before = _host.device_singular_value_fallbacks
    s, sweeps, fallbacks = _host.singular_values_batch_device(d_R, 3, r, return_status=True)
    assert fallbacks == 0 and _host.device_singular_value_fallbacks == before and np.all(np.diff(s, axis=1) <= 0)
    for b, k in enumerate(sc.RATIOS):
        assert sc.ratio_to_reference(s[b], sc.reference(r, k)) <= sc.C_SV * (1 - 2.0 ** -11)
    s2, sweeps2, fallbacks2 = _host.singular_values_batch_device(d_R, 3, r, max_sweeps=3, return_status=True)
    slow = np.flatnonzero(sweeps > 3)
    assert len(slow) and fallbacks2 == len(slow) and _host.device_singular_value_fallbacks == before + len(slow)
    for b in slow:
        assert np.array_equal(s2[b], np.linalg.svd(mats[b], compute_uv=False))
