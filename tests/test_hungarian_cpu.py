"""The Hungarian batteries of tests/hungarian_reference.py, proven on the CPU: every case lands in the dispatch path of
axtrack_amd/csrc/hungarian.hip that its name claims, forces real augmenting searches, has a unique optimum, and the judge
that the GPU tests rely on rejects every seeded fault at the step that describes it. Oracle and SciPy only."""
import numpy as np
import pytest

import hungarian_reference as hr
from oracle import oracle as orc

CASES = hr.all_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _pair_stats(case):
    """Per pair: (t, gap, rows taking part, columns taking part, rows that need a search, links)."""
    dm = hr.dummy_costs(case.counts, case.thr_units)
    out = []
    for (t, g), p in case.reference.pairs.items():
        sub = case.costs[(t, g)][np.ix_(p['rows'], p['cols'])]
        out.append((t, g, len(p['rows']), len(p['cols']), hr.needs_search(sub, dm[t][p['rows']]), int((p['match'] >= 0).sum())))
    return out


# ---------------------------------------------------------------------------------------------- the helper itself
def test_vector_costs_equal_the_oracles():
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 1 << 22, 200), rng.integers(0, 1 << 22, 200)
    units = rng.integers(0, 2 * hr.THR_UNITS, 200)
    for kind in (1, 3):
        got = hr.arc_cost_vec(units, kind, a, b)
        assert [int(v) for v in got] == [orc.arc_cost_int(u / orc.COST_SCALE, kind, x, y) for u, x, y in zip(units, a, b)]
    thr = orc.DEFAULTS['MCF_EDGE_COST_THR']
    assert [int(v) for d in hr.dummy_costs([3, 0, 4]) for v in d] == [orc.arc_cost_int(thr, 1, k, 0) for k in range(7)]
    assert hr.NO_LINK == 0x3fffffffffffffff and hr.THR_UNITS == 700000


def test_dispatch_bounds():
    """The thresholds of axt_hungarian_pairs, derived from its lds_base expression (restated in hr.dispatch)."""
    assert [hr.dispatch(c) for c in (64, 192, 193, 576, 577)] == [(3, 64), (3, 96), (9, 96), (9, 96), (0, 96)]
    c0 = hr.first_cap_without_cache()
    assert hr.dispatch(c0 - 1) == (0, 96) and hr.dispatch(c0) == (0, 0) and hr.dispatch(2048) == (0, 0)
    assert 577 < c0 <= 2048
    assert hr.pair_path(144, 75, 75) == (3, 2, True) and hr.pair_path(192, 180, 20) == (3, 1, False)


@pytest.mark.parametrize('name', ['a64', 'a192_alternating', 'c192_masked_three_slots'])
def test_reference_from_table_agrees_with_the_oracle(name):
    """The new reference, run on a table filled from the oracle's geometric costs, gives oracle.hungarian_assoc's list."""
    c = BY_NAME[name]
    tab = hr.costs_to_table(c.costs, c.counts, c.cap)
    ref = hr.reference_from_table(tab, c.counts)
    assert ref.trajs == orc.hungarian_assoc(c.dets, c.H, c.W, mask=c.mask)
    assert ref.trajs == c.reference.trajs


def test_needs_search_counts_lost_contests():
    NL = hr.NO_LINK
    cost = np.array([[5, 9, NL], [4, 8, NL], [7, NL, 3], [NL, NL, NL], [2, 1, 9]], np.int64)
    dummy = np.array([10, 10, 10, 10, 1], np.int64)
    # row 0 takes column 0; row 1 wants column 0 too: lost; row 2 takes 2; row 3 and row 4 (a tie goes to the dummy) take dummies
    assert hr.needs_search(cost, dummy) == 1


# ---------------------------------------------------------------------------------------------- conditions on the fixtures
@pytest.mark.parametrize('case', CASES, ids=repr)
def test_case_lands_where_its_name_claims(case):
    nc, cdim = hr.dispatch(case.cap)
    if case.name.startswith(('a64', 'a144', 'a192', 'c192')) or case.name.startswith(('b64_', 'b192_')):
        assert nc == 3
    elif case.name.startswith(('a193', 'a576', 'c256', 'b576_')):
        assert nc == 9
    else:
        assert nc == 0
    assert (cdim == 0) == ('no_cache' in case.name or 'sparse' in case.name)
    gap1 = [(case.counts[t], case.counts[t + 1]) for t in range(len(case.counts) - 1)]
    for claim in case.claims:
        hit = [(n, m) for n, m in gap1 if n and m
               and hr.pair_path(case.cap, n, m)[2] == claim['cached']
               and ('slots' not in claim or hr.pair_path(case.cap, n, m)[1] == claim['slots'])
               and claim.get('n_min', 0) <= n <= claim.get('n_max', 1 << 30) and m <= claim.get('m_max', 1 << 30)]
        assert hit, f'{case.name}: no gap-1 pair lands in {claim} (pairs {gap1})'
    stats = _pair_stats(case)
    # real searches: a quarter of some pair's rows lose the initialisation's contest. Not asked of the sparse scenes and of
    # the tables 'no_link' and 'one_row_per_column', where by construction no two rows can want the same column.
    assert case.crowded or 'sparse' in case.name or case.pattern in ('no_link', 'one_row_per_column')
    if case.crowded:
        assert any(n and 4 * lost >= n for _, _, n, _, lost, _ in stats), f'{case.name}: {stats}'
    if case.gap2:
        ok = [s for s in stats if s[1] == 2 and 10 * s[2] >= case.counts[s[0]] > 0 and 10 * s[3] >= case.counts[s[0] + 2] > 0
              and s[5] >= 1]
        assert ok, f'{case.name}: no crowded gap-2 pair: {stats}'
    if case.kind == 'ctab' and case.max_gap == 2 and case.pattern not in ('no_link',):
        assert any(s[1] == 2 and s[5] >= 1 for s in stats), f'{case.name}: no gap-2 link: {stats}'


def test_batteries_cover_every_row_of_the_dispatch_table():
    """One look at the whole: which cases prove which path (slots and cache per NC), empty frames, lattice, conn8."""
    seen = set()
    for c in CASES:
        for t in range(len(c.counts) - 1):
            n, m = c.counts[t], c.counts[t + 1]
            if n and m:
                seen.add(hr.pair_path(c.cap, n, m) + (hr.dispatch(c.cap)[1] == 0, c.kind if c.kind == 'ctab' else ('dtab' if c.mask is not None else 'open')))
    for nc, slots in ((3, 1), (3, 2), (3, 3), (9, None), (0, None)):
        for cached in ((False,) if slots == 3 else (True, False)):      # three slots: m > 128 > cdim, never cached
            assert any(s[:3] == (nc, slots, cached) and s[4] == 'open' for s in seen), (nc, slots, cached)
        assert any(s[:2] == (nc, slots) and s[4] == 'ctab' for s in seen), (nc, slots)
    assert any(s[0] == 0 and s[3] for s in seen)                                    # no cache at all
    assert {s[0] for s in seen if s[4] == 'dtab'} == {3, 9}
    holes = [c for c in hr.battery_a() if c.counts[-1] == 0 and 0 in c.counts[1:-1]]
    assert len(holes) >= 2
    for c in hr.battery_a():                           # every clustered scene runs 8-connected too
        if not c.conn8 and 'sparse' not in c.name and 'lattice' not in c.name:
            assert BY_NAME[c.name + '_conn8'].conn8 and BY_NAME[c.name + '_conn8'].counts == c.counts


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_optimum_is_unique(case):
    """The matching of every pair is unchanged under three random permutations of its rows and columns: the identity hash
    makes the optimum unique, so an exact solver has one answer."""
    rng = np.random.default_rng(5)
    dm = hr.dummy_costs(case.counts, case.thr_units)
    for (t, g), p in case.reference.pairs.items():
        rows, cols = p['rows'], p['cols']
        if len(rows) == 0 or len(cols) == 0:
            continue
        sub, d = case.costs[(t, g)][np.ix_(rows, cols)], dm[t][rows]
        match0, total0 = hr.pair_reference(sub, d)
        for _ in range(3):
            pr, pc = rng.permutation(len(rows)), rng.permutation(len(cols))
            match, total = hr.pair_reference(sub[np.ix_(pr, pc)], d[pr])
            back = np.full(len(rows), -1, np.int64)
            back[pr] = np.where(match >= 0, pc[np.maximum(match, 0)], -1)
            assert total == total0 and np.array_equal(back, match0), f'{case.name}: pair ({t},{t + g}) has two optima'


@pytest.mark.parametrize('case', [c for c in CASES if c.kind == 'ctab' and c.pattern == 'above_dummy'], ids=repr)
def test_above_dummy_case_holds_what_it_says(case):
    """Admitted links that cost more than the dummy, some of them a row's only links; the optimum still links rows."""
    dm = hr.dummy_costs(case.counts, case.thr_units)
    c = case.costs[(0, 1)]
    assert ((c != hr.NO_LINK) & (c > dm[0][:, None])).mean() > 0.25
    assert all(int((p['match'] >= 0).sum()) > 0 for p in case.reference.pairs.values())


# ---------------------------------------------------------------------------------------------- the judge
def _fault_case():
    return BY_NAME['a192_three_slots']


def _judge(case, track, n):
    return hr.judge(case.costs, case.counts, track, n, name=case.name, thr_units=case.thr_units, max_gap=case.max_gap,
                    ref=case.reference)


def _swap_tails(track, counts, ta, ia, tb, ib):
    """Exchange what follows (ta, ia) on its track with what follows (tb, ib) on its own (ta == tb)."""
    ka, kb = int(track[ta, ia]), int(track[tb, ib])
    out = track.copy()
    later = np.arange(track.shape[0])[:, None] > ta
    out[later & (track == ka)] = kb
    out[later & (track == kb)] = ka
    return out


@pytest.mark.parametrize('case', [BY_NAME[n] for n in ('a64', 'a192_three_slots', 'a576_nc9_deep_conn8', 'b192_machol_wien_gap2',
                                                       'b64_above_dummy')], ids=repr)
def test_judge_accepts_the_reference(case):
    ref = case.reference
    _judge(case, hr.track_table(ref.trajs, case.counts, case.cap), len(ref.trajs))


def test_judge_rejects_seeded_faults():
    case = _fault_case()
    ref, counts, costs = case.reference, case.counts, case.costs
    good = hr.track_table(ref.trajs, counts, case.cap)
    n = len(ref.trajs)
    succ, gap = ref.succ, ref.succ_gap

    def step_of(track, n_tracks):
        with pytest.raises(hr.JudgeError) as e:
            _judge(case, track, n_tracks)
        return e.value.step, str(e.value)

    # swap the successors of two rows (both new links admitted): a matching of admitted links, but not the cheapest
    t = 0
    rows = [i for i in range(counts[t]) if gap[t][i] == 1]
    i, k = next((i, k) for i in rows for k in rows if i < k and costs[(t, 1)][i, succ[t][k]] != hr.NO_LINK
                and costs[(t, 1)][k, succ[t][i]] != hr.NO_LINK)
    step, msg = step_of(_swap_tails(good, counts, t, i, t, k), n)
    assert step == 3 and 'pair (0,1) gap 1, n=180 m=180' in msg and 'optimum' in msg, msg
    # drop one link: the rest of the track becomes a track of its own
    t, i = next((t, i) for t in range(len(counts)) for i in range(counts[t]) if gap[t][i] == 1)
    dropped = good.copy()
    later = np.arange(good.shape[0])[:, None] > t
    dropped[later & (good == good[t, i])] = n
    assert step_of(dropped, n + 1)[0] == 3
    # add a link that is not admitted: the end of one track to the start of a track of the next frame
    ends = [(tr[-1], k) for k, tr in enumerate(ref.trajs)]
    (t, i), ka, kb = next(((t, i), ka, kb) for (t, i), ka in ends for kb, tr in enumerate(ref.trajs)
                          if tr[0][0] == t + 1 and costs[(t, 1)][i, tr[0][1]] == hr.NO_LINK)
    added = good.copy()
    added[good == kb] = ka
    added[good > kb] -= 1
    assert step_of(added, n - 1)[0] == 2
    # link through an occupied column: a second row takes a column that has a predecessor already
    t = 0
    i, k = rows[0], rows[1]
    occupied = good.copy()
    later = np.arange(good.shape[0])[:, None] > t
    occupied[later & (good == good[t, i])] = good[t, k]
    assert step_of(occupied, n)[0] == 1
    # renumber two tracks
    renum = good.copy()
    renum[good == 0], renum[good == 1] = 1, 0
    assert step_of(renum, n)[0] == 4
    # a slot beyond count set to 0
    t = next(t for t in range(len(counts)) if counts[t] < case.cap)
    beyond = good.copy()
    beyond[t, counts[t]] = 0
    assert step_of(beyond, n)[0] == 5
    # one track too many reported
    assert step_of(good, n + 1)[0] == 5


# ---------------------------------------------------------------------------------------------- chain numbering reference
def test_chain_walk_on_a_hand_made_example():
    count = np.array([2, 2, 1, 2], np.int32)
    p1 = np.full((4, 3), -1, np.int32)
    p2 = np.full((4, 3), -1, np.int32)
    p1[1, 0] = 1            # (0,1) -> (1,0)
    p2[3, 1] = 0            # (1,0) -> (3,1), gap 2
    p1[3, 0] = 0            # (2,0) -> (3,0)
    p1[2, 2] = 0            # a link in a slot beyond count: ignored
    track, n = hr.chain_walk(count, 3, p1, p2)
    assert n == 4 and track.tolist() == [[0, 1, -1], [1, 2, -1], [3, -1, -1], [3, 1, -1]]
    for kind in ('spanning', 'single', 'roots', 'holes'):
        cnt, q1, q2 = hr.chain_scene(17, 9, kind, seed=1)
        tr, k = hr.chain_walk(cnt, 9, q1, q2)
        assert k == (tr.max() + 1) and (tr[np.arange(9)[None, :] < cnt[:, None]] >= 0).all()
        if kind == 'spanning':
            assert (tr[16, :6] < cnt[0]).any() and set(np.unique(q1)) != {-1} and set(np.unique(q2)) != {-1}
        if kind == 'holes':
            assert (cnt == 0).any()
