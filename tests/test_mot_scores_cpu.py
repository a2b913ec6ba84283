"""The definition of the device tracking scorer (csrc/mot.hip) on the CPU: the reference of
tests/mot_reference.py reaches every route its named cases name, differs from a model with one rule broken, and agrees
with axtrack_amd.mot_metrics wherever a scene has no ties; plus the library's argument checks (no GPU needed)."""
import ctypes

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from axtrack_amd import _lib, mot_metrics as mm
import mot_reference as mr
from mot_reference import assert_scores_equal


def kinds(ref, f=None):
    return sorted(k for (g, k, _, _) in ref['events'] if f is None or g == f)


def test_pair_cost_is_the_arc_cost_hash_under_kind_4():
    """(d2 << 26) | hash16 with the splitmix hash of axt_arc_cost_int (kind 4): the low 16 bits are the library's."""
    lib = _lib.load()
    rng = np.random.default_rng(0)
    for d2, a, b in zip(rng.integers(0, 65026, 50), rng.integers(0, 1 << 24, 50), rng.integers(0, 1 << 24, 50)):
        c = int(mm.pair_cost_int(d2, a, b))
        assert c >> 26 == d2 and (c & 0x3FFFFFF) == lib.axt_arc_cost_int(0.0, 4, int(a), int(b)) & 0xFFFF


def test_named_cases_reach_the_routes_they_name():
    c = mr.named_cases()
    r = {n: mr.reference(s) for n, s in c.items() if s['tracks'].shape[0] == 1}
    assert r['empty_labels']['counts'].tolist() == [0, 0, 0, 3, 0, 0, 3, 0, 0, 0]
    assert r['empty_detections']['counts'].tolist() == [0, 0, 3, 0, 0, 3, 0, 2, 0, 0]
    assert r['both_empty']['counts'].tolist() == [0] * 10 and not r['both_empty']['events']
    assert kinds(r['empty_frame_between']) == [1, 1] and not kinds(r['empty_frame_between'], 1)
    assert r['threshold']['events'] == {(0, 1, 0, 0), (0, 3, 1, -1)} and r['threshold']['fp'] == {(0, 1)}
    assert r['threshold']['counts'][4] == 529
    assert (1, 1, 0, 1) in r['kept_partner']['events'] and r['kept_partner']['fp'] == {(1, 0)}      # 100 kept, 1 refused
    assert r['shared_partner']['claimants'] == [2]
    assert {(2, 1, 0, 0), (2, 2, 1, 1)} <= r['shared_partner']['events']
    assert [kinds(r['switch_after_miss'], f) for f in range(3)] == [[1], [3], [2]]
    assert r['cardinality']['events'] == {(0, 1, 0, 1), (0, 1, 1, 0)} and r['cardinality']['counts'][4] == 625
    assert r['fragmentation']['counts'][8] == 2 and r['fragmentation']['tallies'].tolist() == [[9, 3]]
    for n_lab, n_hyp in ((63, 65), (64, 64), (65, 63), (129, 129)):
        s = c[f'lanes_{n_lab}x{n_hyp}']
        assert (s['gcount'] == n_lab).all() and (s['count'] == n_hyp).all()
        assert r[f'lanes_{n_lab}x{n_hyp}']['counts'][1] > 0                   # switches: step 2 after a lost partner
    s = c['identities_65_k3']
    assert s['tracks'].shape[0] == 3 and s['no'] != s['nh'] and s['no'] > 65
    co = mr.reference(s, 2)['co']
    assert (co.sum(1) == 0).any() and (co.sum(0) == 0).any()                    # identities that never co-occur
    assert len({tuple(mr.reference(s, k)['counts']) for k in range(3)}) == 3
    # the identity matching keeps its state in LDS in every case but the one that names the scratch route
    for n, q in c.items():
        assert (mr.identity_state_bytes(q['no'], q['nh']) > mr.IDENTITY_LDS_LIMIT) == (n == 'identity_state_in_scratch_k3'), n
    far = c['identity_state_in_scratch_k3']
    assert far['nh'] == s['nh'] + 3000 and int(mr.reference(far, 2)['counts'][9]) == int(mr.reference(s, 2)['counts'][9]) > 0
    # the tie case has several optima without the perturbation: the unperturbed sum of another assignment equals it
    assert _has_unperturbed_tie(c['dense_ties'])


def _has_unperturbed_tie(s):
    """Frame 0 of the scene (no partners yet): swapping a label to its other equidistant detection keeps the sum of d2."""
    f = 0
    ng, nd = int(s['gcount'][f]), int(s['count'][f])
    dx = s['gx'][f, :ng, None].astype(np.int64) - s['x'][f, None, :nd]
    dy = s['gy'][f, :ng, None].astype(np.int64) - s['y'][f, None, :nd]
    d2 = dx * dx + dy * dy
    ok = d2 <= s['max_dist'] ** 2
    big = (min(d2.shape) + 1) * (d2[ok].max() + 1)
    r, c = linear_sum_assignment(np.where(ok, d2, big))
    best = np.where(ok, d2, big)[r, c].sum()
    for a, b in zip(r, c):                                   # forbid one chosen pair: is the optimum still reached?
        m = np.where(ok, d2, big).astype(np.float64)
        m[a, b] = big
        r2, c2 = linear_sum_assignment(m)
        if m[r2, c2].sum() == best:
            return True
    return False


@pytest.mark.parametrize('rule, case', [('exclusive_threshold', 'threshold'), ('clear_on_miss', 'switch_after_miss'),
                                        ('sum_before_cardinality', 'cardinality'), ('higher_slot_wins', 'shared_partner'),
                                        ('fragment_outside_span', 'fragmentation')])
def test_a_model_with_one_rule_broken_differs_on_its_named_case(rule, case):
    s = mr.named_cases()[case]
    good, bad = mr.reference(s), mr.reference(s, broken=rule)
    assert good['events'] != bad['events'] or good['counts'].tolist() != bad['counts'].tolist()


def test_the_battery_compared_with_mot_metrics_is_tie_free_and_leaves_no_scene_out():
    battery = mr.tie_free_battery()
    assert len(battery) == len(mr.hand_cases()) + sum(s['tracks'].shape[0] for s in mr.association_scenes())
    for s, k in battery:
        assert mr.is_tie_free(s, k)


def test_scores_from_counts_equal_summarize_on_the_tie_free_battery():
    for s, k in mr.tie_free_battery():
        ref = mr.reference(s, k)
        want = mm.summarize(mr.host_events(s, k)[0])
        assert_scores_equal(mm.scores_from_counts(ref['counts'], ref['tallies']), want)


def test_identity_derivation_max_weight_matching_equals_the_padded_problem():
    """idtp from linear_sum_assignment(-co) equals summarize's padded (no+nh)^2 problem: compared through the scores that
    depend on it alone, on every scene (ties do not matter for the optimum's value)."""
    scenes = [(s, k) for s in list(mr.named_cases().values()) + mr.hand_cases() + mr.association_scenes()
              for k in range(s['tracks'].shape[0])]
    for s, k in scenes:
        ref = mr.reference(s, k)
        want = mm.summarize(mr.host_events(s, k)[0])
        n_obj, n_pred, idtp = int(ref['counts'][5]), int(ref['counts'][6]), float(ref['counts'][9])
        if n_obj + n_pred:
            assert 2 * idtp / (n_obj + n_pred) == pytest.approx(want.idf1, abs=1e-12)
        if n_obj:
            assert idtp / n_obj == pytest.approx(want.idr, abs=1e-12)


# ------------------------------------------------------------------ the integer solver and the limit cases
@pytest.mark.parametrize('name', list(mr.limit_cases()))
def test_limit_cases_have_the_route_facts_they_claim(name):
    case = mr.limit_cases()[name]
    assert case.facts, name
    missing = [f for f in case.facts if f not in mr.facts_of(case)]
    assert not missing, (name, missing)


def test_the_restated_sizes_are_those_the_design_tabulates():
    """The restated lsap_bytes / clear_lds_bytes at the sizes DESIGN.md 6.8g tabulates; the library's own scratch answer
    pins lsap_bytes on both sides of the identity boundary."""
    assert mr.clear_lds_bytes(1024, 1024) == 94208
    assert [mr.clear_lds_bytes(n, n) for n in (712, 713)] == [65504, 65688]
    assert mr.clear_lds_bytes(712, 712) <= mr.DEFAULT_DYNAMIC_LDS < mr.clear_lds_bytes(713, 713)
    assert (mr.clear_lds_bytes(400, 1024), mr.clear_lds_bytes(1024, 400)) == (68624, 62384)
    assert (mr.lsap_bytes(896, 2048), mr.lsap_bytes(897, 2048)) == (65536, 65560) and mr.IDENTITY_LDS_LIMIT == 65536
    lib = _lib.load()
    for no, nh in ((896, 2048), (897, 2048), (1, 1), (7, 21)):
        assert mr.lsap_bytes(no, nh) == mr.identity_state_bytes(no, nh)
        assert _query(lib, K=3, no=no, nh=nh) == (0, 3 * mr.scratch_bytes(no, nh)), (no, nh)


def test_both_solvers_choose_the_same_pairs_on_every_frame_of_every_old_scene():
    scenes = list(mr.named_cases().values()) + mr.hand_cases() + mr.association_scenes()
    n_frames = 0
    for s in scenes:
        for k in range(s['tracks'].shape[0]):
            a, b = mr.reference(s, k, solver='f64'), mr.reference(s, k, solver='int')
            assert a['events'] == b['events'] and a['counts'].tolist() == b['counts'].tolist()
            assert a['step2'].keys() == b['step2'].keys()
            for f in a['step2']:
                assert sorted(a['step2'][f]['pairs']) == sorted(b['step2'][f]['pairs']) and a['step2'][f]['cost'] == b['step2'][f]['cost']
                assert (b['step2'][f]['solver'], a['step2'][f]['solver']) in (('int', 'f64'), ('none', 'none'))
            n_frames += len(a['step2'])
    assert n_frames > 100
    # the broken models still run (on SciPy: the sum-first model has no dummy formulation) and still differ
    for rule in mr.RULES:
        assert mr.reference(mr.named_cases()['cardinality'], broken=rule)['counts'] is not None


def _dense_problem(n, m, seed):
    rng = np.random.default_rng(seed)
    lp, dp = rng.integers(0, 181, (n, 2)), rng.integers(0, 181, (m, 2))
    d2 = ((lp[:, None, :] - dp[None, :, :]) ** 2).sum(2).astype(np.int64)
    cost = mm.pair_cost_int(d2, np.arange(n)[:, None], np.arange(m)[None, :])
    return cost, d2 <= 255 ** 2, (min(n, m) + 1) << mr.PENALTY_SHIFT


@pytest.mark.parametrize('n, m', [(9, 9), (12, 7), (7, 12)])
def test_the_certificate_holds_for_the_optimum_and_rejects_a_swapped_pair(n, m):
    cost, ok, dummy = _dense_problem(n, m, n * m)
    assert ok.all()
    col4row, u, v = mr.solve_int(cost, ok, dummy)
    assert mr.certificate_holds(cost, ok, dummy, col4row, u, v)
    assert (col4row >= 0).sum() == min(n, m)
    # brute force on the small side: no assignment of the same cardinality is cheaper
    r, c = linear_sum_assignment(cost.astype(np.float64))            # < 2^53: 12 pairs below 2^43
    assert sorted(zip(r.tolist(), c.tolist())) == sorted((i, int(j)) for i, j in enumerate(col4row) if j >= 0)
    rows = np.nonzero(col4row >= 0)[0]
    swapped = col4row.copy()
    swapped[rows[0]], swapped[rows[1]] = col4row[rows[1]], col4row[rows[0]]
    assert not mr.certificate_holds(cost, ok, dummy, swapped, u, v)
    # nor does it accept: a column taken twice, a row moved to its dummy, a pair that is not admissible, duals off by one
    twice = col4row.copy(); twice[rows[0]] = col4row[rows[1]]
    assert not mr.certificate_holds(cost, ok, dummy, twice, u, v)
    dropped = col4row.copy(); dropped[rows[0]] = -2
    assert not mr.certificate_holds(cost, ok, dummy, dropped, u, v)
    refused = ok.copy(); refused[rows[0], col4row[rows[0]]] = False
    assert not mr.certificate_holds(cost, refused, dummy, col4row, u, v)
    bumped = u.copy(); bumped[rows[0]] += 1
    assert not mr.certificate_holds(cost, ok, dummy, col4row, bumped, v)


def test_the_integer_solver_refuses_arithmetic_beyond_2_to_the_62():
    cost, ok, dummy = _dense_problem(6, 3, 1)
    with pytest.raises(AssertionError):
        mr.solve_int(cost, ok, 1 << 62)


def test_reading_a_mismatch_tells_a_worse_matching_from_a_tie():
    s = mr.named_cases()['cardinality']
    ref = mr.reference(s)
    assert 'agree' in mr.explain_mismatch(s, 0, ref, ref['events'])
    worse = {(0, 1, 0, 0), (0, 3, 1, -1)}                   # the closer pair alone: one pair fewer than the optimum
    assert 'not the optimum' in mr.explain_mismatch(s, 0, ref, worse)
    assert mr.matching_cost(s, 0, 0, ref['step2'][0]['pairs']) == (2, ref['step2'][0]['cost'])


def test_size_query_at_and_beyond_the_stated_limits():
    lib = _lib.load()
    AXT_EINVAL = -22
    assert _query(lib, cap=mr.MOT_MAX_SIDE, gcap=mr.MOT_MAX_SIDE, max_dist=mr.MOT_MAX_DIST)[0] == 0
    for kw in (dict(cap=1025), dict(gcap=1025), dict(max_dist=256), dict(no=2 ** 24 + 1), dict(nh=2 ** 24 + 1)):
        assert _query(lib, **kw)[0] == AXT_EINVAL, kw
        assert b'axt_mot_scores' in lib.axt_last_error()
    assert _query(lib, no=2 ** 24, nh=1)[0] == 0 and _query(lib, no=1, nh=2 ** 24)[0] == 0


def _query(lib, K=1, F=4, cap=8, gcap=8, no=3, nh=5, max_dist=23):
    need = ctypes.c_size_t(0)
    rc = lib.axt_mot_scores(None, K, None, None, None, F, cap, None, None, None, None, gcap, no, nh, max_dist, None, None,
                            None, None, None, None, ctypes.byref(need), None)
    return rc, need.value


def test_library_exports_mot_scores_and_refuses_bad_shapes():
    lib = _lib.load()
    assert lib.axt_abi_version() == 1
    rc, need = _query(lib)
    assert rc == 0 and need >= 3 * 5 * 4
    assert _query(lib, K=2)[1] == 2 * need
    # the scratch the library asks for is what tests/mot_reference.py restates, on both sides of the LDS limit
    for no, nh in ((3, 5), (70, 270), (70, 2400), (70, 2600), (70, 3270), (1000, 1000)):
        assert _query(lib, no=no, nh=nh) == (0, mr.scratch_bytes(no, nh)), (no, nh)
    assert mr.identity_state_bytes(70, 2400) <= mr.IDENTITY_LDS_LIMIT < mr.identity_state_bytes(70, 2600)
    AXT_EINVAL = -22
    bad = [dict(K=0), dict(F=0), dict(cap=0), dict(cap=1025), dict(gcap=0), dict(gcap=1025), dict(no=0), dict(nh=0),
           dict(max_dist=256), dict(max_dist=-1)]
    for kw in bad:
        assert _query(lib, **kw)[0] == AXT_EINVAL, kw
        assert b'axt_mot_scores' in lib.axt_last_error()
    assert _query(lib, cap=1024, gcap=1024, max_dist=255)[0] == 0
    # the size query needs no scratch; a call with scratch but no arrays is refused
    need = ctypes.c_size_t(1 << 20)
    buf = ctypes.create_string_buffer(8)
    assert lib.axt_mot_scores(None, 1, None, None, None, 4, 8, None, None, None, None, 8, 3, 5, 23, None, None, None, None,
                              None, ctypes.addressof(buf), ctypes.byref(need), None) == AXT_EINVAL
