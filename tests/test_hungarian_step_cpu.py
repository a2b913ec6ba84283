"""The cases of tests/hungarian_step_cases.py are what their names say, on the CPU: which kernel route each one reaches,
which column (or the dummy) wins the step a case is about, that the optimum is tied exactly where a case says so, and
that the minimum formed in two 32-bit phases is the 64-bit minimum -- the rule tests/test_hungarian_step_gpu.py then holds
the kernels to."""
import numpy as np
import pytest

import hungarian_reference as hr
import hungarian_step_cases as sc


# ------------------------------------------------------------------------------------------------ the argmin rule
def _both(words):
    a, b = sc.argmin_64(words), sc.argmin_two_phase(words)
    assert a == b, f'64-bit {a}, two phases {b}'
    return a


def test_two_phase_argmin_equals_the_64_bit_one_on_random_words():
    rng = np.random.default_rng(0)
    for trial in range(400):
        bits = int(rng.integers(1, 51))
        keys = rng.integers(0, 1 << bits, 64)
        if trial % 3 == 0:                       # few distinct high words: the second phase decides
            keys = (keys & ((1 << 21) - 1)) | (int(rng.integers(0, 1 << 29)) << 21)
        if trial % 5 == 0:                       # equal keys in several lanes: the column decides
            keys[rng.integers(0, 64, 8)] = keys.min()
        keys = np.where(rng.random(64) < 0.2, sc.HINF, keys)
        cols = rng.permutation(2048)[:64] if trial % 2 else np.arange(64) + 64 * rng.integers(0, 3, 64)
        key, col = _both(sc.pack(keys, cols))
        live = keys < sc.KEY_LIMIT
        if live.any():
            assert key == keys[live].min() and col == cols[live & (keys == key)].min()
        else:
            assert (key, col) == (sc.HINF, 0x7fffffff)


def test_two_phase_argmin_on_the_edges():
    none = np.full(64, sc.HINF)
    assert _both(sc.pack(none, np.zeros(64, np.int64))) == (sc.HINF, 0x7fffffff)
    keys = none.copy()
    keys[63] = sc.KEY_LIMIT - 1                  # high word 0x3fffffff, low word 0xfffff800 | column
    assert _both(sc.pack(keys, np.full(64, 2047))) == (sc.KEY_LIMIT - 1, 2047)      # a low word of all ones that takes part
    keys[5] = sc.KEY_LIMIT                       # no candidate
    assert _both(sc.pack(keys, np.full(64, 2047))) == (sc.KEY_LIMIT - 1, 2047)
    keys = none.copy()
    keys[[3, 40]] = [(9 << 21) | 5, (8 << 21) | 900]        # the smaller high word carries the larger low word
    assert _both(sc.pack(keys, np.arange(64))) == ((8 << 21) | 900, 40)
    assert _both(sc.pack(np.zeros(64, np.int64), np.arange(64)[::-1])) == (0, 0)


@pytest.mark.parametrize('case', [c for c in sc.pair_cases() if getattr(c, 'pattern', '') != 'machol_wien'], ids=repr)
def test_two_phase_argmin_on_every_step_of_the_cases(case):
    """(not the Machol-Wien ones: thousands of steps each, of the same kind)"""
    for (t, g), pair in sc.model_reference(case.costs, case.counts, case.thr_units, case.max_gap).pairs.items():
        steps = []
        sc.jv_model(case.costs[(t, g)][np.ix_(pair['rows'], pair['cols'])], hr.dummy_costs(case.counts, case.thr_units)[t][pair['rows']], steps)
        for keys in steps:
            _both(sc.lane_words(keys))


# ------------------------------------------------------------------------------------------------ the cases
def _second_step(case):
    steps = []
    dummy = hr.dummy_costs(case.counts, case.thr_units)[0]
    match, total = sc.jv_model(case.costs[(0, 1)], dummy, steps)
    return steps, dummy, match, total


@pytest.mark.parametrize('case', sc.argmin_cases(), ids=repr)
def test_argmin_case_is_decided_in_the_step_it_names(case):
    steps, dummy, match, total = _second_step(case)
    cost = case.costs[(0, 1)]
    assert hr.needs_search(cost, dummy) == 1 and len(steps) == 2
    assert sc.argmin_64(sc.lane_words(steps[0])) == (0, sc.J0)              # the first step takes the contested column
    key, col = sc.argmin_64(sc.lane_words(steps[1]))
    best_dummy = int(dummy.min()) - sc.BASE
    if case.wins == 'dummy':
        assert best_dummy <= key and (match >= 0).sum() == 1
        assert (key == best_dummy) == case.ties
    else:
        assert key < best_dummy and col == case.wins and case.wins in match
        assert (int((steps[1] == key).sum()) > 1) == case.ties
    best, where = sc.enumerated_optimum(cost, dummy)
    assert total == best and (len(where) > 1) == case.ties
    if case.exact == 'scipy':
        assert hr.pair_reference(cost, dummy)[1] == best
    else:                                        # beyond the judge's exact f64 sums: enumeration is the reference
        assert int(cost[cost != sc.HINF].max()) >= hr.EXACT_F64 and len(where) == 1


def test_argmin_cases_cover_what_they_should():
    by = {c.name: c for c in sc.argmin_cases()}
    paths = {hr.pair_path(c.cap, *c.counts) for c in by.values()}
    assert {(3, 1, True), (3, 2, True), (3, 3, False)} <= paths               # one, two, three register slots
    packed = lambda name: sorted(int(sc.pack([k - sc.BASE], [j])[0]) for j, k in
                                 ((j, int(by[name].costs[(0, 1)][:, j].min())) for j in range(by[name].counts[1])) if k != sc.HINF and j != sc.J0)
    hi = lambda ws: [w >> 32 for w in ws]
    lo_key = lambda ws: [(w & 0xFFFFFFFF) >> 11 for w in ws]
    assert len(set(hi(packed('hi_equal_lo_differs')))) == 1 and len(set(lo_key(packed('hi_equal_lo_differs')))) == 3
    assert len(set(hi(packed('lo_equal_hi_differs')))) == 3 and len(set(lo_key(packed('lo_equal_hi_differs')))) == 1
    w = packed('hi_decides_against_lo')
    assert (w[0] & 0xFFFFFFFF) == max(x & 0xFFFFFFFF for x in w)              # the winner has the largest low word
    tied = lambda name: sorted(j for j in range(by[name].counts[1]) if j != sc.J0 and by[name].costs[(0, 1)][:, j].min() != sc.HINF)
    a, b = tied('tie_two_lanes')
    assert a // 16 == b // 16 and a != b
    a, b = tied('tie_two_rows_of_lanes')
    assert a // 16 != b // 16 and b < 64
    a, b = tied('tie_two_slots_one_lane')
    assert a % 64 == b % 64 and a // 64 != b // 64
    assert len({j // 64 for j in tied('tie_three_slots')}) == 3
    assert packed('key_2p51_minus_1')[0] >> 32 == 0x3FFFFFFF


@pytest.mark.parametrize('case', sc.boundary_cases(), ids=repr)
def test_boundary_case_reaches_its_routes_and_searches(case):
    ref = case.reference
    model = sc.model_reference(case.costs, case.counts, case.thr_units, case.max_gap)
    assert model.trajs == ref.trajs                       # unique optimum: the model of the kernel's rules is SciPy's answer
    counts = case.counts
    dummies = hr.dummy_costs(counts, case.thr_units)
    searched = sum(hr.needs_search(case.costs[k][np.ix_(p['rows'], p['cols'])], dummies[k[0]][p['rows']]) for k, p in ref.pairs.items())
    assert searched >= 20, 'the case must force searches'
    assert len(counts) <= 8
    if 'empty' in case.name:
        pairs = [(counts[t], counts[t + 1]) for t in range(len(counts) - 1)]
        assert any(n > 0 and m == 0 for n, m in pairs) and any(n == 0 and m > 0 for n, m in pairs) and (0, 0) in pairs
        assert (ref.pairs[(0, 2)]['match'] >= 0).any(), 'no link across the empty frame'
    elif 'rising' not in case.name:               # (rising counts leave no row without a successor)
        partly = [(t, p) for (t, g), p in ref.pairs.items() if g == 2 and 0 < len(p['rows']) < counts[t] and 0 < len(p['cols']) < counts[t + 2]]
        assert partly, 'no gap-2 pair with rows and columns partly taken'
        assert any((p['match'] >= 0).any() for _, p in partly), 'no gap-2 link'


def test_boundary_cases_cover_the_slot_and_cache_bounds():
    rows, cols, paths = {144: set(), 192: set()}, {144: set(), 192: set()}, set()
    for case in sc.boundary_cases():
        for t in range(len(case.counts) - 1):
            n, m = case.counts[t], case.counts[t + 1]
            rows[case.cap].add(n)
            cols[case.cap].add(m)
            if n and m:
                paths.add(hr.pair_path(case.cap, n, m))
    assert set(sc.BOUNDARY_SIZES_144) <= rows[144] and set(sc.BOUNDARY_SIZES_144) <= cols[144]
    assert {191, 192} <= rows[192] and {191, 192} <= cols[192]
    assert {(3, s, c) for s in (1, 2) for c in (True, False)} | {(3, 3, False)} <= paths
    assert all(hr.dispatch(cap) == (3, 96) for cap in (144, 192))


# ------------------------------------------------------------------------------------------------ chain numbering
def test_chain_shapes_sit_on_both_sides_of_the_bound():
    shapes = sc.chain_shapes()
    slots = [f * c for f, c in shapes]
    assert sc.CHAIN_SMALL_SLOTS in slots and sc.CHAIN_SMALL_SLOTS + 1 in slots
    routes = [sc.chain_route(s) for s in slots]
    assert routes[:2] == ['small', 'launches'] and set(routes[2:]) == {'launches'}
    assert [f for f, _ in shapes[2:]] == [1, 2, 3, 4, 5, 16, 17, 64, 65]


@pytest.mark.parametrize('kind', sc.CHAIN_KINDS)
def test_chain_scenes_are_what_they_say(kind):
    for F, cap in ((5, 40), (16, 33), (17, 9)):
        count, pred1, pred2 = sc.chain_scene(F, cap, kind, seed=F)
        track, n = hr.chain_walk(count, cap, pred1, pred2)
        valid = np.arange(cap)[None, :] < count[:, None]
        assert (track[valid] >= 0).all() and (track[~valid] == -1).all() and n == len(np.unique(track[valid]))
        for p in (pred1, pred2):                 # links end at a detection, and no two at the same one
            for t in range(F):
                src = p[t][p[t] >= 0]
                assert (p[t][~valid[t]] == -1).all() and len(set(src)) == len(src)
        if kind == 'gap2_only':
            assert (pred1 < 0).all() and (pred2 >= 0).any() and n < valid.sum()
        if kind == 'empty_middle':
            assert count[F // 2] == 0 and (pred2[F // 2 + 1] >= 0).any()
        if kind == 'holes':
            assert (count[1:-1] == 0).any()
