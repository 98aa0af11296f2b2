"""GPU suite: figh_chain_pass_fused as two launches -- the fused kernel, then the merge launch whose last workgroup sums the
column norms and selects the columns -- storing its pack straight into page-locked host memory, against the separate
entries on the same inputs: figh_regressor_tsqr_fused, figh_select_columns, one copy.

``colsq`` and ``sel`` are compared bit for bit (one copy of the summing and selecting code, the same order of the sums).
``rows_k`` of a fused pass is reproduced up to rounding only (which consumer wave takes which tile is decided at run time),
so it is compared as tests/test_chain_pass_native.py compares two fused runs: through the host tail -- index sets and
``beta`` exactly, ``absdiagR`` up to the first dependent column to 1e-11, ``phi_ls`` to 1e-10, ``residual_norm`` to 1e-11.
The merge entry itself (figh_tsqr_merge_base_norms) works on a given stack of triangles in a fixed order of the children:
there the rows are compared bit for bit with figh_tsqr_merge_base, the sums with a NumPy mirror of the summing order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [4096,               # the smallest size that fuses
         4096 + 37,          # ragged last tile, odd number of sample tiles: the two producers differ
         64 * 2 * 256 + 64]  # one workgroup has one tile more than the rest (256 compute units)


@pytest.fixture(scope="module")
def lib():
    from figaroh_plus_amd import _lib
    _lib.load()
    assert _lib.device_count() > 0, "GPU tests need a HIP device"
    return _lib


def _samples(N, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.uniform(-6, 6, (N, 6)) for _ in range(3))


def _upload(lib, pipe, q, v, a):
    for d_arr, h in ((pipe.d_q, q), (pipe.d_v, v), (pipe.d_a, a)):
        h = np.ascontiguousarray(h)
        lib.check(lib.load().figh_memcpy_h2d(d_arr.ptr, h.ctypes.data, h.nbytes))


class _Pass:
    """A pipeline that has run once (kept set learnt, buffers allocated) and the raw entries on its buffers."""

    def __init__(self, lib, g, N, with_tau, seed):
        from figaroh_plus_amd.pipeline import IdentificationPipeline
        self.lib = lib
        pipe = self.pipe = IdentificationPipeline(g.robot(), g.param, params_std=g.params_std(), coupling=g.coupling)
        pipe.set_samples(*_samples(N, seed))
        if with_tau:
            pipe.set_tau_from_parameters(g.phi_ref(), noise_std=0.05, seed=3)
        pipe.run()
        assert pipe.fused_passes == 1
        self.N, self.with_tau = N, with_tau
        self.mask, self.d_kept, self.n = pipe._fused_kept
        self.ncols = pipe.W.ref_cols
        self.nc = self.n + (1 if with_tau else 0)
        self.sel_words = (2 + 2 * self.ncols + 1) // 2
        self.words = self.ncols + self.sel_words + (self.nc + 1) * self.nc
        self.handle, self.flags = pipe._handle(), pipe._flags()[1]
        self.d_pack = lib.DeviceArray((self.words,), np.float64)
        self.pinned = lib.PinnedArray(self.words)
        self.d_colsq = lib.DeviceArray((self.ncols,), np.float64)
        self.d_sel = lib.DeviceArray((2 * self.sel_words,), np.int32)
        self.d_rows = lib.DeviceArray((self.nc + 1, self.nc), np.float64)

    def _tail(self):
        tail = self.lib.HostTail(self.n, self.with_tau)
        s = tail.s
        s.tol_qr, s.total_rows, s.pieces, s.null_rule = self.pipe.tol_qr, 6 * self.N, 1, 0
        return tail

    def _unpack(self, host):
        ncols, sw = self.ncols, self.sel_words
        sel = host[ncols:ncols + sw].view(np.int32)[:2 + 2 * ncols]
        return host[:ncols].copy(), sel.copy(), host[ncols + sw:self.words].reshape(self.nc + 1, self.nc).copy()

    def fused(self, pinned=True, mask=None):
        """figh_chain_pass_fused -> (ok, colsq, sel, rows, tail); the landing buffer is filled with NaN bytes first."""
        p, lib = self.pipe, self.lib
        host = self.pinned.array if pinned else np.empty(self.words)
        host.view(np.uint8)[:] = 0xFF
        lib.check(lib.load().figh_memcpy_h2d(self.d_pack.ptr, host.ctypes.data, host.nbytes))
        tail = self._tail()
        mask = self.mask if mask is None else mask
        ok = lib.chain_pass_fused(self.handle, self.flags, self.N, p.d_q, p.d_v, p.d_a, p.W.buf, p.W.ld, self.d_kept, self.n,
                                  p.d_tau, p.tol_qr, p.tol_e, self.d_pack, host.ctypes.data, 8 * self.words,
                                  np.ascontiguousarray(mask).view(np.uint8), tail)
        assert ok is not None, "the shape did not fuse"
        return (ok,) + self._unpack(host) + (tail,)

    def separate(self):
        """The separate entries on the same inputs -> (colsq, sel, rows, tail)."""
        p, lib = self.pipe, self.lib
        assert lib.regressor_tsqr_fused(self.handle, self.flags, self.N, p.d_q, p.d_v, p.d_a, p.W.buf, p.W.ld, self.d_colsq,
                                        self.d_kept, self.n, p.d_tau, p.tol_qr, self.d_rows)
        lib.select_columns(self.d_colsq, self.ncols, p.tol_e, 14, self.d_sel)
        colsq, sel, rows = self.d_colsq.to_host(), self.d_sel.to_host()[:2 + 2 * self.ncols], self.d_rows.to_host()
        tail = self._tail()
        lib.chain_host_tail(tail, rows)
        return colsq, sel, rows, tail


def _same_tail(a, b, n, with_tau):
    """Two factorisations of the same matrix through the host tail, with the tolerances of tests/test_chain_pass_native.py."""
    r = a.s.n_base
    assert r == b.s.n_base and a.s.status == b.s.status == 0
    assert np.array_equal(a.idx, b.idx)
    assert np.array_equal(a.beta[:r * (n - r)], b.beta[:r * (n - r)])
    dep = sorted(a.idx[r:].tolist())
    first_dep = dep[0] if dep else n
    d_a, d_b = a.absdiag[:first_dep], b.absdiag[:first_dep]
    print("absdiag: max rel difference %.3g" % (np.abs(d_a - d_b).max() / d_a.max()))
    assert np.abs(d_a - d_b).max() <= 1e-11 * d_a.max()
    if with_tau:
        print("phi_ls: max rel difference %.3g, residual %.3g" % (
            np.abs(a.phi_ls[:r] - b.phi_ls[:r]).max() / np.abs(a.phi_ls[:r]).max(),
            abs(a.s.residual_norm - b.s.residual_norm) / a.s.residual_norm))
        assert np.abs(a.phi_ls[:r] - b.phi_ls[:r]).max() <= 1e-10 * np.abs(a.phi_ls[:r]).max()
        assert np.array_equal(b.phi_b[:r], np.round(b.phi_ls[:r], 6))
        assert abs(a.s.residual_norm - b.s.residual_norm) <= 1e-11 * a.s.residual_norm


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _check_against_separate(ps, got, want):
    ok, colsq, sel, rows, tail = got
    colsq_s, sel_s, rows_s, tail_s = want
    assert ok
    assert np.array_equal(_bits(colsq), _bits(colsq_s)), "colsq is not bit-identical"
    assert np.array_equal(sel, sel_s), "sel is not bit-identical"
    assert np.array_equal(sel[2 + ps.ncols:] != 0, ps.mask)
    # nothing of the NaN fill is left, and the rows of dependent columns are exact zeros (the zero fill arrived, and first)
    assert np.all(np.isfinite(rows))
    dep = tail_s.idx[tail_s.s.n_base:]
    assert np.all(rows[dep] == 0.0) and np.all(rows_s[dep] == 0.0)
    _same_tail(tail_s, tail, ps.n, ps.with_tau)


_PASSES = {}  # (N, with_tau) -> _Pass: set up once, shared by the tests of that shape


@pytest.fixture(params=[(N, t) for N in SIZES for t in (True, False)], ids=lambda p: "N%d-%s" % (p[0], "tau" if p[1] else "notau"))
def ps(request, lib, golden_ur10):
    N, with_tau = request.param
    if request.param not in _PASSES:
        _PASSES[request.param] = _Pass(lib, golden_ur10, N, with_tau, 900 + N)
    return _PASSES[request.param]


def test_two_launch_pass_equals_the_separate_entries(ps):
    _check_against_separate(ps, ps.fused(pinned=True), ps.separate())


def test_pageable_landing_buffer_gives_the_same_pack(ps):
    """h_pack without a device address: the pack goes through d_pack and one copy.  Same bytes of colsq | sel."""
    zero_copy, staged = ps.fused(pinned=True), ps.fused(pinned=False)
    assert np.array_equal(_bits(zero_copy[1]), _bits(staged[1])) and np.array_equal(zero_copy[2], staged[2])
    _check_against_separate(ps, staged, ps.separate())
    _same_tail(zero_copy[4], staged[4], ps.n, ps.with_tau)


def test_three_passes_on_the_same_buffers_return_their_own_results(lib, golden_ur10):
    ps = _Pass(lib, golden_ur10, 4096 + 37, True, 41)
    seen = []
    for rep in range(3):
        q, v, a = _samples(ps.N, 50 + rep)
        _upload(lib, ps.pipe, q, v, a)
        got, want = ps.fused(pinned=True), ps.separate()
        _check_against_separate(ps, got, want)
        seen.append((got[1], got[3]))
    for i in range(3):
        for j in range(i):  # other samples, other numbers: no pass returned its predecessor's pack
            assert not np.array_equal(seen[i][0], seen[j][0]) and not np.array_equal(seen[i][1], seen[j][1])


def test_changed_kept_set_is_reported_with_the_new_mask(lib, golden_ur10):
    ps = _Pass(lib, golden_ur10, 4096, True, 77)
    q, v, a = _samples(ps.N, 78)
    for x in (q, v, a):
        x[:, :3] = 0.0
    _upload(lib, ps.pipe, q, v, a)
    for pinned in (True, False):
        ok, colsq, sel, rows, tail = ps.fused(pinned=pinned)
        colsq_s, sel_s, _, _ = ps.separate()
        assert ok is False
        assert np.array_equal(_bits(colsq), _bits(colsq_s)) and np.array_equal(sel, sel_s)
        mask_now = sel[2 + ps.ncols:] != 0
        assert not np.array_equal(mask_now, ps.mask) and int(sel[0]) == int(mask_now.sum()) != ps.n
        assert np.array_equal(mask_now, ~(colsq < ps.pipe.tol_e))
    # the same buffers with the columns they were launched for again: one call, not changed
    _upload(lib, ps.pipe, *_samples(ps.N, 79))
    _check_against_separate(ps, ps.fused(pinned=True), ps.separate())


# ---- the merge entry on a given stack: one launch with the epilogue workgroup, or the separate steps

def _tree_workgroups(count, fan=16):
    total = 0
    while True:
        nb = -(-count // fan)
        total += nb
        if nb == 1:
            return total
        count = nb


def _sum_mirror(part):
    """The library's order: thread t sums the blocks t, t + 256, ...; then the halving tree over the 256 threads."""
    s = np.zeros((256, part.shape[1]))
    for b in range(part.shape[0]):
        s[b % 256] += part[b]
    w = 128
    while w:
        s[:w] += s[w:2 * w]
        w //= 2
    return s[0].copy()


def _merge_case(lib, count, nc, nblocks, ncols, seed):
    rng = np.random.default_rng(seed)
    part = rng.uniform(0.0, 4.0, (nblocks, ncols)) * rng.choice([0.0, 1.0, 1e-3], ncols)  # (first: the same for every count)
    stack = np.triu(rng.standard_normal((count, nc, nc)))
    stack[:, :, 3] = stack[:, :, 1] - 2.0 * stack[:, :, 2]  # one dependent column: the rank decision has something to decide
    stack = np.triu(stack)
    tol_e, tol_qr = 1e-2 * nblocks, 1e-8
    d_stack, d_part = lib.DeviceArray.from_host(stack), lib.DeviceArray.from_host(part)
    d_colsq = lib.DeviceArray.from_host(np.full(ncols, np.nan))
    d_sel, d_sel_ref = (lib.DeviceArray.from_host(np.full(2 + 2 * ncols, -1, np.int32)) for _ in range(2))
    d_rows, d_rows_ref = (lib.DeviceArray.from_host(np.full((nc + 1, nc), np.nan)) for _ in range(2))
    lib.tsqr_merge_base_norms(d_stack, count, nc, nc, tol_qr, d_part, nblocks, ncols, tol_e, d_colsq, d_sel, d_rows)
    colsq = d_colsq.to_host()
    want = _sum_mirror(part)
    assert np.array_equal(_bits(colsq), _bits(want)), "the sums do not follow the fixed order"
    lib.select_columns(lib.DeviceArray.from_host(want), ncols, tol_e, 14, d_sel_ref)
    assert np.array_equal(d_sel.to_host(), d_sel_ref.to_host())
    lib.tsqr_merge_base(d_stack, count, nc, nc, tol_qr, d_rows_ref)
    rows, rows_ref = d_rows.to_host(), d_rows_ref.to_host()
    assert np.all(np.isfinite(rows)) and np.array_equal(_bits(rows), _bits(rows_ref))
    assert np.all(rows[3] == 0.0) and rows[2, 2] != 0.0 and abs(rows[nc, 3]) <= tol_qr < abs(rows[nc, 2])
    return colsq, d_sel.to_host(), rows


@pytest.mark.parametrize("nblocks,ncols", [(1, 1), (255, 84), (512, 84), (513, 98), (700, 128), (300, 129)])
def test_merge_launch_with_norms_small_tree(lib, nblocks, ncols):
    """One resident launch (three merge workgroups + regrouping + epilogue); 129 columns are more than the epilogue
    workgroup takes: the separate steps.  Blocks below, at and above one and two rounds of the 256 summing threads; column
    counts that fill the last round of eight columns per thread group partly, fully and not at all."""
    _merge_case(lib, 37, 8, nblocks, ncols, 1000 + nblocks + ncols)


def test_merge_launch_with_norms_refused_residency(lib):
    """Triangle counts around the residency bound of the one-launch tree: tree + regrouping + epilogue workgroup equal to
    the compute units (taken), one more (the epilogue does not fit: separate steps, the tree still one launch), and a
    tree that does not fit at all (level-by-level fallback).  Same answers in all three."""
    cus = lib.device_info()["cu_count"]
    nc, nblocks, ncols = 8, 300, 84
    fits = max(c for c in range(2, 16 * cus) if _tree_workgroups(c) + 2 <= cus)
    no_epilogue = max(c for c in range(2, 16 * cus) if _tree_workgroups(c) + 1 <= cus)
    assert _tree_workgroups(no_epilogue) + 2 > cus
    out = [_merge_case(lib, count, nc, nblocks, ncols, 7) for count in (fits, no_epilogue, 16 * cus + 5)]
    for colsq, sel, _ in out[1:]:  # (the same partials in all three)
        assert np.array_equal(_bits(colsq), _bits(out[0][0])) and np.array_equal(sel, out[0][1])
