"""The battery of tests/recon_reference.py is what it claims to be -- proven on the CPU, before tests/test_recon_routes_gpu.py
runs it through the kernels of axtrack_amd/csrc/recon.hip: every named pair reaches the stage its name stands for, every
stage is reached 4- and 8-connected, the reference's paths pass an independent property check, the stages as recon.hip
documents them give the reference's cells on every pair, and each stage with one rule broken does not: the battery would
notice that bug."""
import collections

import numpy as np
import pytest

import recon_reference as rr
import pathsearch_reference as pr
from axtrack_amd.detections import _interp_index


def _moves(case, p):
    """(off, moves) of the reference optimum of a pair on its mask."""
    cost = int(pr.costs_from(case.mask_of(p), case.conn8, *p.S)[p.T[1], p.T[0]])
    return cost // pr.OFF, cost % pr.OFF + cost // pr.OFF


@pytest.mark.parametrize('case', rr.battery(), ids=repr)
def test_every_named_pair_reaches_its_route(case):
    for i, p in enumerate(case.pairs):
        assert rr.route(case, i) == case.claimed(p), f'{case.name}: {p.name} is decided by {rr.route(case, i)}'


@pytest.mark.parametrize('conn8', [False, True])
def test_every_route_is_reached_and_none_is_decided_at_every_stage(conn8):
    """Each stage decides links with a path and, except the classifier, links without one."""
    with_path, none = collections.Counter(), collections.Counter()
    for case in rr.battery():
        if case.conn8 == conn8:
            for i, want in enumerate(rr.expected_paths(case)):
                (none if want is None else with_path)[rr.route(case, i)] += 1
    print(dict(with_path), dict(none))
    for r in rr.ROUTES:
        if r != 'gate':
            assert with_path[r] >= 2, (r, with_path[r])
    for r in ('gate', 'bfs31', 'bfs127', 'key31', 'exact'):
        assert none[r] >= 1, (r, none[r])
    assert with_path['open'] >= 4


@pytest.mark.parametrize('case', rr.battery(), ids=repr)
def test_reference_paths_have_the_properties_of_an_optimal_path(case):
    """Independent of the walk: start, end, neighbouring moves, no cell twice, cost equal to Dijkstra's; 'none' exactly where
    the gate fails or the optimum has max_dist cells or more."""
    H, W = case.shape
    for p, c in zip(case.pairs, rr.expected_paths(case)):
        m = case.mask_of(p)
        (sx, sy), (tx, ty) = p.S, p.T
        inside = 0 <= sx < W and 0 <= sy < H and 0 <= tx < W and 0 <= ty < H
        gate = inside and (tx - sx) ** 2 + (ty - sy) ** 2 < case.max_dist ** 2
        mask = np.ones((H, W), np.uint8) if m is None else m
        if c is None:
            cost = int(pr.costs_from(mask, case.conn8, sx, sy)[ty, tx]) if gate else 0
            assert not gate or cost % pr.OFF + cost // pr.OFF + 1 >= case.max_dist, (case.name, p.name)
            continue
        assert gate and c[0] == sy * W + sx and c[-1] == ty * W + tx, (case.name, p.name)
        r, q = c // W, c % W
        dr, dq = np.abs(np.diff(r)), np.abs(np.diff(q))
        assert np.all((np.maximum(dr, dq) == 1) if case.conn8 else (dr + dq == 1)), (case.name, p.name)
        assert len(set(c.tolist())) == len(c) < case.max_dist
        wgt = np.where(mask == 1, 1, pr.OFF).astype(np.int64).ravel()
        assert wgt[c[1:]].sum() == pr.costs_from(mask, case.conn8, sx, sy)[ty, tx], (case.name, p.name)


def test_pairs_have_the_moves_their_names_say():
    """The figures in the names are the reference's: moves of the optimum, and off-mask cells where the case is about them."""
    for c8 in (False, True):
        sfx = '_conn8' if c8 else ''
        for cname, pname, off, moves in [
                ('bfs_steps', 'straight_31', 0, 31), ('bfs_steps', 'straight_32', 0, 32), ('bfs_steps', 'straight_127', 0, 127),
                ('bfs_steps', 'straight_128', 0, 128), ('bfs_steps', 'left_31', 0, 31), ('bfs_steps', 'left_32', 0, 32),
                ('bfs_steps', 'detour_31', 0, 31), ('bfs_steps', 'detour_32', 0, 32),
                ('no_path_rule_20', 'on_18', 0, 18), ('no_path_rule_20', 'on_19_none', 0, 19),
                ('no_path_rule_20', 'detour_18', 0, 18), ('no_path_rule_20', 'detour_19_none', 0, 19),
                ('no_path_rule_20', 'off_source_18', 0, 18), ('no_path_rule_20', 'off_source_19_none', 0, 19),
                ('no_path_rule_20', 'off_source_island_to_bar', 3, 7 if not c8 else None),
                ('no_path_rule_100', 'on_98', 0, 98), ('no_path_rule_100', 'on_99_none', 0, 99),
                ('no_path_rule_100', 'detour_98', 0, 98), ('no_path_rule_100', 'detour_99_none', 0, 99),
                ('no_path_rule_100', 'off_source_98', 0, 98), ('no_path_rule_100', 'off_source_99_none', 0, 99),
                ('key_accept', 'off_target_m31', 2, 31), ('key_accept', 'off_target_m32', 2, 32),
                ('key_accept', 'off_target_m63', 2, 63), ('key_accept', 'off_target_m64', 2, 64),
                ('key_accept', 'other_component_m31', 3, 31), ('key_accept', 'other_component_m32', 3, 32),
                ('key_accept', 'void_metric_bound', 15 if c8 else 19, 15 if c8 else 19),
                ('key_accept', 'off_source_crosses_component', 3, 20 if c8 else 24),
                ('key_reject_off', 'long_route', 1, None), ('key_reject_off', 'long_route_too_long_none', 1, None)]:
            case = rr.case(cname + sfx)
            o, m = _moves(case, case.pair(pname))
            assert o == off and (moves is None or m == moves), f'{case.name}: {pname} has (off, moves) = {(o, m)}'
            want = rr.expected_paths(case)[case.pairs.index(case.pair(pname))]
            assert (want is None) == pname.endswith('_none'), f'{case.name}: {pname}'
    # the cheap detours stay within Chebyshev distance 31 of their sources: only the moves send them on
    for name in ('bfs_steps', 'bfs_steps_conn8'):
        p = rr.case(name).pair('detour_32')
        assert max(abs(p.S[0] - p.T[0]), abs(p.S[1] - p.T[1])) <= 31


@pytest.mark.parametrize('conn8', [False, True])
def test_certificate_cases_are_built_as_described(conn8):
    sfx = '_conn8' if conn8 else ''
    # key_reject_off: the field says one off-mask cell, the windows see three
    case = rr.case('key_reject_off' + sfx)
    for name in ('long_route', 'long_route_too_long_none'):
        p = case.pair(name)
        for R in (31, 63):
            info = _window(case, p, R)
            assert info == dict(o=3, m=3, lb=1), (name, R, info)
    assert 100 < len(rr.expected_paths(case)[0]) < case.max_dist and rr.expected_paths(case)[1] is None
    # key_reject_moves: the radius-31 window holds a path with the bound's off-mask cells and more than 31 moves ...
    case = rr.case('key_reject_moves' + sfx)
    for name in ('winding_inside_window', 'optimum_leaves_window'):
        p = case.pair(name)
        w31, w63 = _window(case, p, 31), _window(case, p, 63)
        assert w31['o'] == w31['lb'] == 1 and w31['m'] > 31 and w63['o'] == 1 and w63['m'] <= 63, (name, w31, w63)
        assert (w63['o'], w63['m']) == _moves(case, p)
        # ... and for the second pair the grid's optimum leaves that window and has fewer moves
        assert (w63['m'] < w31['m']) == (name == 'optimum_leaves_window'), (name, w31, w63)
    c = rr.expected_paths(case)[case.pairs.index(case.pair('optimum_leaves_window'))]
    assert (np.abs(c % case.shape[1] - 50) > 31).any()
    # exhausted: the source's on-mask neighbours are a component without the target; the frontier runs out
    case = rr.case('exhausted' + sfx)
    p = case.pair('island_to_corridor')
    field = rr.bfs_field(case.masks[0], conn8, *p.S)
    assert np.isfinite(field).sum() == 3 and not np.isfinite(field[p.T[1], p.T[0]])
    # components: 64 keep the fields, 65 do not
    for n in (64, 65):
        label, n_comp, d_off = rr.component_fields(rr.case(f'components_{n}' + sfx).masks[0], conn8)
        assert n_comp == n and (d_off is None) == (n == 65)
        counts = rr.stage_counts(rr.case(f'components_{n}' + sfx))[0]
        assert (counts['key31'] + counts['key63'] > 0) == (n == 64)


def _window(case, p, R):
    """(o, m, lb) of the key window of radius R, whatever the certificate says: the model with both clauses dropped takes
    the first window the pair fits in, so ask for the radius alone."""
    m = case.mask_of(p)
    H, W = m.shape
    (sx, sy), (tx, ty) = p.S, p.T
    x0, y0, x1, y1 = max(sx - R, 0), max(sy - R, 0), min(sx + R, W - 1), min(sy + R, H - 1)
    cost = int(pr.costs_from(np.ascontiguousarray(m[y0:y1 + 1, x0:x1 + 1]), case.conn8, sx - x0, sy - y0)[ty - y0, tx - x0])
    label, n_comp, d_off = rr.component_fields(m, case.conn8)
    assert m[sy, sx] == 1
    return dict(o=cost // pr.OFF, m=cost % pr.OFF + cost // pr.OFF, lb=int(d_off[label[sy, sx] - 1, ty, tx]))


def test_component_fields_agree_with_the_path_search_reference():
    """Two labellings (flood fill here, scipy there) and the same fields."""
    for name in ('key_accept', 'key_reject_moves_conn8', 'components_64', 'components_65_conn8', 'no_path_rule_20'):
        case = rr.case(name)
        label, n_comp, d_off = rr.component_fields(case.masks[0], case.conn8)
        f = pr.Fields(case.masks[0], case.conn8)
        assert n_comp == f.n_comp and np.array_equal(label, f.label)
        assert (d_off is None) == (f.off is None) and (d_off is None or np.array_equal(d_off, f.off))


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


@pytest.mark.parametrize('case', rr.battery(), ids=repr)
def test_documented_stages_give_the_reference_cells(case):
    """The breadth-first field, the window keys with their certificate and the no-path rule, as recon.hip states them, end
    in the whole-grid reference's cells on every pair: the shortcuts are sound on this battery."""
    for p, want in zip(case.pairs, rr.expected_paths(case)):
        if case.mask_of(p) is not None:
            r, got, info = rr.stage_model(case.mask_of(p), case.conn8, case.max_dist, p.S, p.T)
            assert _same(got, want), f'{case.name}: {p.name} ({r}, {info})'


def _differs(case_name, pair_name, broken):
    case = rr.case(case_name)
    p = case.pair(pair_name)
    want = rr.expected_paths(case)[case.pairs.index(p)]
    r, got, info = rr.stage_model(case.mask_of(p), case.conn8, case.max_dist, p.S, p.T, broken)
    return not _same(got, want), (r, info)


@pytest.mark.parametrize('broken, case_name, pair_name', [
    ('diagonals_first', 'bfs_plaza_conn8', 'octant_7_3'),                      # (bfs stage)
    ('diagonals_first', 'key_accept_conn8', 'void_metric_bound'),              # (key stage)
    ('diagonals_first', 'components_65_conn8', 'void_many_ties'),            # (exact search)
    ('no_o_eq_lb', 'key_reject_off', 'long_route'), ('no_o_eq_lb', 'key_reject_off_conn8', 'long_route'),
    ('no_o_eq_lb', 'key_reject_off', 'long_route_too_long_none'),
    ('no_m_le_R', 'key_reject_moves', 'optimum_leaves_window'), ('no_m_le_R', 'key_reject_moves_conn8', 'optimum_leaves_window'),
    ('rule_for_off_source', 'no_path_rule_20', 'off_source_island_to_bar'),
    ('rule_for_off_source', 'no_path_rule_20_conn8', 'off_source_island_to_bar'),
    ('limit_R', 'no_path_rule_20', 'on_19_none'), ('limit_R', 'no_path_rule_20_conn8', 'detour_19_none'),
    ('limit_R', 'no_path_rule_100', 'on_99_none'), ('limit_R', 'no_path_rule_100_conn8', 'detour_99_none')])
def test_a_broken_rule_is_caught_by_a_named_pair(broken, case_name, pair_name):
    differs, why = _differs(case_name, pair_name, broken)
    assert differs, f'{case_name}: {pair_name} gives the reference cells with {broken} ({why})'


def test_a_dropped_moves_clause_is_caught_by_one_pair_only():
    """'optimum_leaves_window' is the pair the m <= R clause is there for: no other pair of the battery notices."""
    hits = [(c.name, p.name) for c in rr.battery() for p in c.pairs
            if c.mask_of(p) is not None and _differs(c.name, p.name, 'no_m_le_R')[0]]
    assert sorted(hits) == [('key_reject_moves', 'optimum_leaves_window'), ('key_reject_moves_conn8', 'optimum_leaves_window')]


# ----------------------------------------------------------------------------------------------------- links and cells
def test_links_table_has_the_shapes_it_is_there_for():
    track, count = rr.links_table()
    F, cap = track.shape
    assert F > 1024 and cap > rr.EMIT_CHUNK and count.max() > cap and (count[[10, 11, 500]] > rr.EMIT_CHUNK).all()
    assert (track[10] >= 0).sum() > rr.EMIT_CHUNK and (track[11] == -1).sum() > 50
    for max_gap in (1, 2, 3):
        rows = rr.track_links(track, count, max_gap)
        assert np.array_equal(rows, rr.links_model(track, count, max_gap))
        assert (np.diff(rows[:, 0]) > 0).all() and set(rows[:, 2].tolist()) == set(range(1, max_gap + 1))
        tails = {int(a): (int(b), int(g)) for a, b, g in rows}
        # id 900: frames 80 -> 81, 20 -> 22, 40 -> 43, 60 -> 64: linked iff the gap is within max_gap
        for f0, g in ((80, 1), (20, 2), (40, 3), (60, 4)):
            slot = f0 * cap + int(np.flatnonzero(track[f0, :count[f0]] == 900)[0])
            assert (slot in tails) == (g <= max_gap) and (g > max_gap or tails[slot][1] == g)
        # links of the second chunk of a frame, a frame with links in both chunks, the last frame as a head
        assert ((rows[:, 0] // cap == 10) & (rows[:, 0] % cap >= rr.EMIT_CHUNK)).any()
        assert ((rows[:, 0] // cap == 10) & (rows[:, 0] % cap < rr.EMIT_CHUNK)).any()
        assert (rows[:, 1] // cap == F - 1).any()
        # an id in consecutive frames at different slots; ids beyond the count never link
        assert ((rows[:, 2] == 1) & (rows[:, 0] % cap != rows[:, 1] % cap)).any()
        assert (rows[:, 0] % cap < np.minimum(count, cap)[rows[:, 0] // cap]).all()
        assert (rows[:, 1] % cap < np.minimum(count, cap)[rows[:, 1] // cap]).all()
        # the broken kernels differ
        assert not np.array_equal(rows, rr.links_model(track, count, max_gap, 'no_chunk_carry'))
        wider = rr.links_model(track, count, max_gap, 'gap_plus_one')
        assert len(wider) > len(rows) and (wider[:, 2] == max_gap + 1).any()


def test_links_and_cells_on_a_hand_made_table():
    """The reference against values worked out by hand, the rule of test_axon_reconstruction._expected_links (consecutive
    appearances of an id at most max_gap frames apart) and detections._interp_index."""
    #                 slot 0  1  2
    track = np.array([[3, 7, -1],           # frame 0
                      [7, 3, 5],            # frame 1: both ids again, in other slots
                      [-1, 5, 9],           # frame 2: 9 lies beyond the count
                      [3, 9, 7]], np.int32)  # frame 3: 3 after two frames, 7 after two frames
    count = np.array([3, 3, 2, 5], np.int32)
    want2 = [(0, 4, 1), (1, 3, 1), (3, 11, 2), (4, 9, 2), (5, 7, 1)]
    assert rr.track_links(track, count, 2).tolist() == [list(r) for r in want2]
    assert rr.track_links(track, count, 1).tolist() == [list(r) for r in want2 if r[2] == 1]
    assert rr.track_links(track, count, 3).tolist() == [list(r) for r in want2]
    for max_gap in (1, 2, 3):
        cnt = np.minimum(count, 3)
        rule = set()
        for k in (3, 5, 7):
            fr = [f for f in range(4) if k in track[f, :cnt[f]]]
            for f0, f1 in zip(fr[:-1], fr[1:]):
                if f1 - f0 <= max_gap:
                    rule.add((f0 * 3 + list(track[f0]).index(k), f1 * 3 + list(track[f1]).index(k), f1 - f0))
        assert set(map(tuple, rr.track_links(track, count, max_gap).tolist())) == rule
    # cells: paths of 5, 4 and 2 cells, one link without a path; gaps 2, 3, 2, 3 at max_gap = 3
    paths = [np.array([10, 11, 12, 13, 14]), np.array([20, 21, 22, 23]), None, np.array([30, 31])]
    lens, gaps = np.array([5, 4, 100, 2]), np.array([2, 3, 2, 3])
    cell_ptr, cells, interp = rr.link_cells(lens, paths, gaps, 100, 3)
    assert cell_ptr.tolist() == [0, 5, 9, 9, 11] and cells.tolist() == [10, 11, 12, 13, 14, 20, 21, 22, 23, 30, 31]
    # 1*4/2 = 2; 1*3/3 = 1, 2*3/3 = 2; none; 1*1/3 -> 0, 2*1/3 = 0.67 -> 1
    assert interp.tolist() == [[12, -1], [21, 22], [-1, -1], [30, 31]]
    for L in range(1, 40):
        for g in (1, 2, 3, 4):
            for k in range(1, g):
                assert rr.interp_index(k, L, g) == _interp_index(k, L, g)
    # rounding half down moves the anchor where k (L - 1) / g ends in one half: 1 * 3 / 2
    assert rr.interp_index(1, 4, 2) == 2 and rr.interp_index(1, 4, 2, half_down=True) == 1
    for c in rr.cells_battery():
        if c.max_gap > 1:
            lens, cell_ptr, cells, interp = c.expected()
            paths = [cells[a:b] if b > a else None for a, b in zip(cell_ptr[:-1], cell_ptr[1:])]
            assert not np.array_equal(interp, rr.link_cells(lens, paths, c.links[:, 2], c.max_dist, c.max_gap, half_down=True)[2])


@pytest.mark.parametrize('case', rr.cells_battery(), ids=repr)
def test_cells_cases_have_the_shapes_they_are_there_for(case):
    lens, cell_ptr, cells, interp = case.expected()
    has = lens < case.max_dist
    assert len(lens) > 1024 and lens[has].max() > 128 and (lens == 1).any() and 50 < (~has).sum() < has.sum()
    assert set(case.links[:, 2].tolist()) == set(range(1, case.max_gap + 1))
    assert interp.shape == (len(lens), case.max_gap - 1) and cell_ptr[-1] == len(cells) == lens[has].sum()
    if case.max_gap > 1:
        assert (interp[~has] == -1).all() and (interp[has & (case.links[:, 2] == 3)] >= 0).all()
        assert (interp[has & (case.links[:, 2] == 1)] == -1).all()


def test_open_staircase_orders():
    """4-connected: columns, then rows; 8-connected: the diagonal, then straight."""
    W = 20
    assert rr.open_staircase(2, 3, 4, 1, W, False).tolist() == [3 * W + 2, 3 * W + 3, 3 * W + 4, 2 * W + 4, 1 * W + 4]
    assert rr.open_staircase(2, 3, 5, 1, W, True).tolist() == [3 * W + 2, 2 * W + 3, 1 * W + 4, 1 * W + 5]
    assert rr.open_staircase(5, 1, 4, 4, W, True).tolist() == [1 * W + 5, 2 * W + 4, 3 * W + 4, 4 * W + 4]
