"""Host suite: the case table of tests/test_streamed_columnwise.py reaches every branch of the chunk loop of
regressor_tsqr_impl (csrc/figh_stream.hip), as seen through its host mirror stream_common.stream_plan -- the pattern of
test_qr_structured_graded.test_batch_cases_reach_every_path -- within the budgets the reference can afford, the
mirror's formulas against three records worked out by hand, and the mirror against the library's own plan function
(csrc/figh_stream_plan.h, compiled for the host through tools/stream_plan_host.cpp)."""
import os
import shutil
import subprocess

import pytest

import stream_common as sc

PLANS = {c.id: sc.case_plan(c) for c in sc.CASES}


def _rows(case):
    param, coupling = sc.case_param(case)
    return sc.facts(case.model, param, coupling).rps * case.N


def test_cases_reach_every_branch():
    P = PLANS
    chained = [p for p in P.values() if p.chained]
    assert any(p.chain_wgs >= 2 and p.nc <= 96 for p in chained), "narrow multi-workgroup chain"
    assert any(p.chain_wgs >= 2 and p.nc >= 170 for p in chained), "medium multi-workgroup chain"
    for name in ("c_narrow_ragged", "c_narrow_last1", "c_medium_ragged", "c_medium_last1"):
        assert P[name].chained and P[name].chain_wgs >= 2 and not P[name].split
    assert P["c_narrow_last1"].last == 1 and P["c_medium_last1"].last == 1  # all but one workgroup idle
    split = [p for p in P.values() if p.split]
    assert any(p.ncf <= 80 for p in split) and any(p.ncf > 80 for p in split)
    assert all(p.chained and 3 * p.cs >= 16 * p.nc for p in split)
    assert any(p.last == p.cs for p in split) and any(p.last == 1 for p in split)
    assert any(1 < p.last and 3 * p.last < 16 * p.nc for p in split), "a split chunk below the split's own threshold"
    assert any(p.nc == p.n for p in split) and any(p.nc == p.n + 1 for p in split), "with and without tau"
    # the split is switched off by nf == n and by weights, on the models that otherwise split
    assert not P["d_off_force_only"].split and P["d_off_force_only"].nc > 80 and P["d_wide_force"].split
    assert not P["d_off_weights"].split and P["d_ragged"].split
    assert sc.CASE["d_off_weights"].weights is not None and P["d_off_weights"].chained
    assert sc.CASE["c_weighted"].weights is not None and P["c_weighted"].chain_wgs >= 2  # weights with chains
    # link-compact and its fallback, each chunked and wide
    assert P["e_compact"].link_compact is True and P["e_fallback"].link_compact == "fallback"
    assert all(P[k].nchunks > 1 and P[k].nc > 80 and P[k].chained for k in ("e_compact", "e_fallback"))
    assert any(p.padded and p.link_compact is False for p in P.values())
    assert any(not p.padded for p in P.values())
    # the structure hint: on, off for an unsorted list of the same columns, dropped in a short last chunk, never for cs < 64
    assert all(P["b_sorted"].hinted) and not any(P["b_unsorted"].hinted)
    assert sorted(sc.column_list(sc.CASE["b_sorted"])) == sorted(sc.column_list(sc.CASE["b_unsorted"]))
    assert P["b_sorted"].nc <= 80 and P["b_sorted"].padded
    assert P["a_last37"].hinted == [True, True, False] and P["a_last37"].last == 37
    assert 6 * 37 < 8 * P["a_last37"].nc  # fewer rows than 8 nc: one wave
    assert P["a_chunk50"].cs < 64 and not any(P["a_chunk50"].hinted)
    assert 64 < P["a_tx40_ragged"].nc <= 80 and all(P["a_tx40_ragged"].hinted)
    # chunk shapes
    lasts = [p.last for p in P.values() if p.nchunks > 1]
    assert 1 in lasts and any(1 < x < 64 for x in lasts) and any(64 <= x for x in lasts)
    assert any(p.last == p.cs and p.nchunks == 3 for p in P.values())
    assert any(p.cs % 64 for p in P.values() if p.nchunks > 1)
    assert P["a_one_chunk"].nchunks == 1 and sc.CASE["a_one_chunk"].chunk > sc.CASE["a_one_chunk"].N
    # tile-blocked inputs: accepted shapes only (the refusal is a test of its own)
    blocked = [c for c in sc.CASES if c.flags & sc.FLAG_BLOCKED_INPUTS]
    assert blocked and all(P[c.id].nchunks > 1 and P[c.id].cs % 64 == 0 and P[c.id].last % 64 for c in blocked)
    assert any(P[c.id].chained for c in blocked) and any(all(P[c.id].hinted) for c in blocked)
    # every model of the issue
    assert {c.model for c in sc.CASES} >= {"ur10", "tx40", "tiago", "talos", "human", "fork", "fork-ff"}
    assert sc.FULL_RANK <= set(P) and any(P[k].split for k in sc.FULL_RANK) and any(all(P[k].hinted) for k in sc.FULL_RANK)
    assert set(sc.ENTRY.values()) == {"norms", "gram"} and P["d_gram"] == P["d_even"]


def test_cases_stay_within_the_budgets():
    for c in sc.CASES:
        p = PLANS[c.id]
        assert p.nchunks <= sc.MAX_CHUNKS, c.id
        assert _rows(c) * p.nc ** 2 <= sc.MAX_GRAM_WORK, c.id
        assert _rows(c) * 2.0 ** -64 <= 1e-14, c.id  # the long-double Gram's own error: a tenth of TOL_BACKWARD
        # the one device-dependent term of the plan -- chain_wgs <= workgroups of the blocked kernel -- cannot bind
        assert p.chain_wgs <= sc.MAX_CHAIN_WGS, c.id
        assert p.level0_launches == p.nchunks * (2 if p.split else 1)
        assert len(set(sc.column_list(c).tolist())) == p.n


JT, EW = sc.MODE_JOINT_TORQUE, sc.MODE_EXT_WRENCH
# free-flyer tree of 8 links, link 3 without a segment, slots 0 .. 11 of the others = 84 columns (7 x 6 = 42 with slot >= 6)
_FF8_COLS = [14 * l + s for l in range(8) if l != 3 for s in range(12)]
_FF8_LIVE = [l != 3 for l in range(8)]
# the calls of test_plan_against_hand_computed_records (the arguments of stream_plan), in its order
HAND_CALLS = [
    (6, 84, 6, True, JT, 0, False, True, list(range(0, 98, 2)), True, False, 549, 256, None),
    (24, 336, 24, False, JT, 7, False, True, list(range(179)), True, True, 375, 128, None),
    (6, 112, 8, False, EW, 0, True, False, _FF8_COLS, False, False, 1025, 512, _FF8_LIVE),
    (6, 112, 8, False, EW, 0, True, False, _FF8_COLS + [14 * 3], False, True, 1025, 512, _FF8_LIVE),
    (6, 84, 6, True, JT, 0, False, True, None, False, False, 1000, 0, None),
]


def test_plan_against_hand_computed_records():
    """Three calls worked out from the source of regressor_tsqr_impl by hand."""
    # UR10-like chain: 6 rows per sample, 49 sorted columns + tau, N = 549 in chunks of 256 -> 256, 256, 37
    p = sc.stream_plan(*HAND_CALLS[0])
    assert p == sc.Plan(49, 50, 256, 3, 37, False, False, [True, True, False], False, False, 0, 1, 0, 3, 18)
    # TIAGo-like tree: 24 rows per sample, 179 columns + tau, weights, N = 375 in chunks of 128 -> 128, 128, 119;
    # chain_wgs = 24 * 128 / (8 * 180) = 2.13 -> 2
    p = sc.stream_plan(*HAND_CALLS[1])
    assert p == sc.Plan(179, 180, 128, 3, 119, True, False, [False] * 3, True, False, 0, 1, 2, 3, 72)
    # the free-flyer tree of 8 links, no tau, N = 1025 in chunks of 512: 3 * 512 = 1536 >= 16 * 84 = 1344 -> split,
    # nf = ncf = 42; chained, 6 * 512 / 2 / (8 * 84) = 2.29 -> 2 workgroups; 3 chunks (512, 512, 1), 6 level-0 launches
    p = sc.stream_plan(*HAND_CALLS[2])
    assert p == sc.Plan(84, 84, 512, 3, 1, True, True, [False] * 3, True, True, 42, 42, 2, 6, 18)
    # the same list with one column of the dead link: the link-padded fallback; with weights: no split, 4 workgroups
    p = sc.stream_plan(*HAND_CALLS[3])
    assert p.link_compact == "fallback" and not p.split and p.chain_wgs == 6 * 512 // (8 * 85) == 4
    # chunk_samples = 0: the default chunk, 2e9 / (8 * 6 * 84) = 496 031 -> 496 000 = 7750 * 64; one chunk
    p = sc.stream_plan(*HAND_CALLS[4])
    assert sc.default_chunk(6, 84) == 496000 and (p.cs, p.nchunks, p.n, p.chained) == (1000, 1, 84, False)


# ------------------------------------------------------------------------------ the mirror against the library's own plan
NO_CAP = 1 << 20  # a chain capacity that cannot bind (the mirror has none)
NATIVE_FIELDS = ("n nc cs nchunks last padded compact_applies compact nlive ldc chained split nf ncf chain_wgs "
                 "level0_launches pieces").split()


def _call_line(call, capacity):
    """A call of stream_plan as a line of tools/stream_plan_host.cpp: the library sees nv and njoints where the mirror is told
    `single_dof` (a free-flyer root alone has six velocities), and the link map where the mirror is told which links live."""
    rps, ncols, nlinks, is_chain, mode, flags, free_flyer, single_dof, cols, with_tau, weighted, N, chunk, live = call
    cols = list(range(ncols)) if cols is None else [int(c) for c in cols]
    nv = nlinks if single_dof else nlinks + 5
    words = [rps, ncols, nlinks, nv, nlinks + 1, is_chain, free_flyer, mode, flags, with_tau, weighted, N, chunk, capacity]
    if live is None:
        words.append(-1)
    else:
        pos, k = [], 0
        for x in live:
            pos.append(k if x else -1)
            k += bool(x)
        words += [k] + pos
    return " ".join(str(int(w)) for w in words + [len(cols)] + cols)


def _native_plans(tmp_path, calls_and_caps):
    """Compile tools/stream_plan_host.cpp (the host compiler alone) and run it over the calls: one dict per call."""
    cxx = shutil.which(os.environ.get("CXX", "c++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "stream_plan_host")
    subprocess.run([cxx, "-std=c++17", "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "figaroh_plus_amd", "csrc"),
                    os.path.join(root, "tools", "stream_plan_host.cpp"), "-o", exe], check=True)
    text = "".join(_call_line(call, cap) + "\n" for call, cap in calls_and_caps)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(calls_and_caps)
    plans = []
    for line in out:
        w = [int(x) for x in line.split()]
        k = len(NATIVE_FIELDS)
        assert len(w) == k + 1 + w[k]
        plans.append(dict(zip(NATIVE_FIELDS, w[:k]), first=w[k + 1:]))
    return plans


def _expected_native(call, p, capacity):
    """The native plan's fields from the mirror's Plan `p` of the same call (and, for what the mirror does not hold -- ldc,
    nlive, the hint's first columns -- from their definitions)."""
    rps, ncols, nlinks, _, _, _, _, _, cols, _, _, N, _, live = call
    cols = list(range(ncols)) if cols is None else [int(c) for c in cols]
    used = p.link_compact is True
    nlive = sum(bool(x) for x in live) if used else -1
    sizes = [p.cs] * (p.nchunks - 1) + [p.last]
    assert sum(sizes) == N
    first = [sum(c < 14 * j for c in cols) for j in range(rps)] if p.hinted[0] else []
    e = dict(n=p.n, nc=p.nc, cs=p.cs, nchunks=p.nchunks, last=p.last, padded=int(p.padded),
             compact_applies=int(p.link_compact is not False), compact=int(used), nlive=nlive,
             ldc=16 * (nlive if used else nlinks) if p.padded else ncols, chained=int(p.chained), split=int(p.split), nf=p.nf,
             ncf=p.ncf, chain_wgs=min(p.chain_wgs, capacity), level0_launches=p.level0_launches, pieces=p.pieces, first=first)
    return e, sizes


def test_mirror_against_the_native_plan(tmp_path):
    """figh::stream_plan (csrc/figh_stream_plan.h), compiled for the host, gives the plan of the Python mirror, field by field,
    for all cases of the table and the hand-computed calls; and, with a chain capacity that binds, two plans worked out by
    hand.  No library, no device."""
    calls = [(c.id, sc.case_call(c)) for c in sc.CASES] + [("hand%d" % i, call) for i, call in enumerate(HAND_CALLS)]
    assert len(sc.CASES) == 33
    # A. TIAGo-like tree (24 rows per sample, 24 links, joint torques), 179 columns + tau = 180, N = 3000 in chunks of 1200
    #    -> 1200, 1200, 600: chained, no split (joint torques), no hint (more than 80 columns); 24 * 1200 / (8 * 180) = 20
    #    workgroups wanted, a capacity of 7 -> 7.  Link-padded: ldc = 16 * 24 = 384.  3 launches, 24 * 3 = 72 pieces.
    bound_a = (24, 336, 24, False, JT, 7, False, True, list(range(179)), True, False, 3000, 1200, None)
    want_a = dict(n=179, nc=180, cs=1200, nchunks=3, last=600, padded=1, compact_applies=0, compact=0, nlive=-1, ldc=384,
                  chained=1, split=0, nf=0, ncf=1, chain_wgs=7, level0_launches=3, pieces=72, first=[])
    # B. the free-flyer tree of 8 links (7 with a segment: link-compact, ldc = 16 * 7 = 112), 84 columns, no tau, N = 5000
    #    in chunks of 2048 -> 2048, 2048, 904: 3 * 2048 = 6144 >= 16 * 84 = 1344 -> split, nf = ncf = 42; chained over the
    #    torque half of the rows, 6 * 2048 / 2 / (8 * 84) = 9.14 -> 9 workgroups wanted, a capacity of 5 -> 5.
    #    2 launches per chunk = 6, 6 * 3 = 18 pieces.
    bound_b = (6, 112, 8, False, EW, 0, True, False, _FF8_COLS, False, False, 5000, 2048, _FF8_LIVE)
    want_b = dict(n=84, nc=84, cs=2048, nchunks=3, last=904, padded=1, compact_applies=1, compact=1, nlive=7, ldc=112,
                  chained=1, split=1, nf=42, ncf=42, chain_wgs=5, level0_launches=6, pieces=18, first=[])
    native = _native_plans(tmp_path, [(call, NO_CAP) for _, call in calls] + [(bound_a, 7), (bound_b, 5)])
    for (tag, call), got in zip(calls, native):
        p = sc.stream_plan(*call)
        want, sizes = _expected_native(call, p, NO_CAP)
        for key in NATIVE_FIELDS + ["first"]:
            assert got[key] == want[key], "%s: %s is %r natively, %r in the mirror" % (tag, key, got[key], want[key])
        # a chunk is hinted when there is a hint and it has at least 64 samples
        assert [bool(got["first"]) and s >= 64 for s in sizes] == p.hinted, tag
    assert native[-2] == want_a and native[-1] == want_b
    # ... and the mirror, which has no capacity, agrees with both up to that term (20 and 9 workgroups)
    for call, want, wgs in ((bound_a, want_a, 20), (bound_b, want_b, 9)):
        assert _expected_native(call, sc.stream_plan(*call), NO_CAP)[0] == dict(want, chain_wgs=wgs)
