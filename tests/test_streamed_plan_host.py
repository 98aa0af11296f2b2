"""Host suite: the case table of tests/test_streamed_columnwise.py reaches every branch of the chunk loop of
regressor_tsqr_impl (csrc/figh_stream.hip), as seen through its host mirror stream_common.stream_plan -- the pattern of
test_qr_structured_graded.test_batch_cases_reach_every_path -- within the budgets the reference can afford, and the
mirror's formulas against three records worked out by hand."""
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


def test_plan_against_hand_computed_records():
    """Three calls worked out from the source of regressor_tsqr_impl by hand."""
    JT, EW = sc.MODE_JOINT_TORQUE, sc.MODE_EXT_WRENCH
    # UR10-like chain: 6 rows per sample, 49 sorted columns + tau, N = 549 in chunks of 256 -> 256, 256, 37
    p = sc.stream_plan(6, 84, 6, True, JT, 0, False, True, list(range(0, 98, 2)), True, False, 549, 256, None)
    assert p == sc.Plan(49, 50, 256, 3, 37, False, False, [True, True, False], False, False, 0, 1, 0, 3, 18)
    # TIAGo-like tree: 24 rows per sample, 179 columns + tau, weights, N = 375 in chunks of 128 -> 128, 128, 119;
    # chain_wgs = 24 * 128 / (8 * 180) = 2.13 -> 2
    p = sc.stream_plan(24, 336, 24, False, JT, 7, False, True, list(range(179)), True, True, 375, 128, None)
    assert p == sc.Plan(179, 180, 128, 3, 119, True, False, [False] * 3, True, False, 0, 1, 2, 3, 72)
    # free-flyer tree of 8 links, link 3 without a segment, slots 0 .. 11 of the others = 84 columns (7 x 6 = 42 with slot
    # >= 6), no tau, N = 1025 in chunks of 512: 3 * 512 = 1536 >= 16 * 84 = 1344 -> split, nf = ncf = 42; chained,
    # 6 * 512 / 2 / (8 * 84) = 2.29 -> 2 workgroups; 3 chunks (512, 512, 1), 6 level-0 launches
    cols = [14 * l + s for l in range(8) if l != 3 for s in range(12)]
    live = [l != 3 for l in range(8)]
    p = sc.stream_plan(6, 112, 8, False, EW, 0, True, False, cols, False, False, 1025, 512, live)
    assert p == sc.Plan(84, 84, 512, 3, 1, True, True, [False] * 3, True, True, 42, 42, 2, 6, 18)
    # the same list with one column of the dead link: the link-padded fallback; with weights: no split, 4 workgroups
    p = sc.stream_plan(6, 112, 8, False, EW, 0, True, False, cols + [14 * 3], False, True, 1025, 512, live)
    assert p.link_compact == "fallback" and not p.split and p.chain_wgs == 6 * 512 // (8 * 85) == 4
    # chunk_samples = 0: the default chunk, 2e9 / (8 * 6 * 84) = 496 031 -> 496 000 = 7750 * 64; one chunk
    p = sc.stream_plan(6, 84, 6, True, JT, 0, False, True, None, False, False, 1000, 0, None)
    assert sc.default_chunk(6, 84) == 496000 and (p.cs, p.nchunks, p.n, p.chained) == (1000, 1, 84, False)
