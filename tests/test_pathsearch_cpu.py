"""The battery of tests/pathsearch_reference.py is what it claims to be -- proven on the CPU, before tests/test_pathsearch_gpu.py
runs it through the kernels of axtrack_amd/csrc/path_bfs.hip: the Dijkstra reference agrees with the project's C oracle,
every case lands in the routes its name says, every deciding route decides enough pairs on both sides of the length limit,
and the pairs the cases were built around have the lengths they were built for."""
import collections

import numpy as np
import pytest

import pathsearch_reference as pr
from oracle import oracle as orc


def _frame(case, t):
    xs = np.array([p[0] for p in case.frames[t]], np.int64)
    ys = np.array([p[1] for p in case.frames[t]], np.int64)
    return None, xs, ys


@pytest.mark.parametrize('case', [c for c in pr.battery() if c.group in 'ACDF'], ids=repr)
def test_dijkstra_reference_equals_the_c_oracle(case):
    """Two independent implementations agree on every frame pair before either judges a kernel."""
    H, W = case.shape
    for g in range(1, case.max_gap + 1):
        for t in range(len(case.frames) - g):
            a, b = _frame(case, t), _frame(case, t + g)
            if len(a[1]) == 0 or len(b[1]) == 0:
                continue
            want = orc.path_matrix(a, b, H, W, case.mask, case.max_dist, case.conn8)
            got = np.array([[pr.path_length(case.mask, case.conn8, sx, sy, tx, ty, case.max_dist) for tx, ty in case.frames[t + g]]
                            for sx, sy in case.frames[t]], np.int32)
            assert np.array_equal(got, want), f'{case.name} frames ({t},{t + g}): {np.argwhere(got != want)[:5]}'


@pytest.mark.parametrize('case', pr.battery_x(), ids=repr)
def test_exact_cases_equal_the_c_oracle_and_their_names(case):
    H, W = case.mask.shape
    src = (None, np.array([p[0] for p in case.sources], np.int64), np.array([p[1] for p in case.sources], np.int64))
    dst = (None, np.array([p[0] for p in case.targets], np.int64), np.array([p[1] for p in case.targets], np.int64))
    want = orc.path_matrix(src, dst, H, W, case.mask, case.max_dist, case.conn8)
    got = case.expected()
    assert np.array_equal(got, want)
    for name, (i, j, L) in case.named.items():
        assert got[i, j] == (case.max_dist if L is None else L), f'{case.name}: {name} is {got[i, j]}'


@pytest.mark.parametrize('case', pr.battery(), ids=repr)
def test_case_takes_the_routes_its_name_says(case):
    """The dispatch model sends the case's sources where the case claims, every route the case is there for decides at
    least one of its pairs, and the grid has the component count its name says."""
    m = pr.model(case)
    for key, want in case.source_route.items():
        assert m.source_route[key] == want, f'{case.name}: source {key} takes {m.source_route[key]}'
    seen = collections.Counter(p.route for p in m.pairs)
    for r in case.routes:
        assert seen[r] > 0, f'{case.name}: no pair decided by {r}: {dict(seen)}'
    if case.name.startswith('F_64'):
        assert m.n_comp == 64 and m.n_general == 0
    if case.name.startswith('F_65') or 'no_fields' in case.name:
        assert m.n_comp == 65 and m.n_windowed == 0 and m.n_general > 0
    if case.name.startswith('F_empty'):
        assert m.n_comp == 0 and set(m.source_route.values()) == {'plain'} and m.n_windowed > 0
    if case.name.startswith('G_cap1157'):
        assert m.off_mode_ok
    if case.name.startswith('G_cap1158') or case.env:
        assert not m.off_mode_ok
    if case.fill:       # real detections in slot 0 and in the last slots, everything else out of the grid, count == cap
        x, y, cnt = case.arrays()
        assert (cnt == case.cap).all() and (x[1:, [0, case.cap - 2, case.cap - 1]] >= 0).all() and (x[:, 1:case.cap - 2] == -1).all()


def test_every_route_decides_pairs_on_both_sides_of_the_limit():
    """Over the battery each deciding route gives at least 8 arcs and at least 8 refusals that are due to the length, not
    the gate. The all-off front is the exception, by geometry: a target it settles has P <= kv, an all-off walk of P moves
    whose off-cell count no path over the mask beats. If P exceeded the lower bound of the gate, every shortest walk of the
    open grid would cross a mask cell, have fewer than P off-mask cells and touch a component within 251 cells of the
    source (so unsaturated), giving some a_C + d_off[C][T] < P: the pair would be ambiguous or have kv < P. Hence P + 1 ==
    lower <= dmax and the all-off front never refuses a pair that passed the gate; that count is asserted to be 0."""
    arcs, long_ = collections.Counter(), collections.Counter()
    for case in pr.battery():
        for p in pr.model(case).pairs:
            if p.route in pr.ROUTES:
                (arcs if p.arc else long_)[p.route] += 1
    print(dict(arcs), dict(long_))
    for r in pr.ROUTES:
        assert arcs[r] >= 8, (r, arcs[r])
        if r == 'front_off':
            assert long_[r] == 0
        else:
            assert long_[r] >= 8, (r, long_[r])


@pytest.mark.parametrize('case', [c for c in pr.battery() if c.named], ids=repr)
def test_pairs_called_out_by_name(case):
    """251 / 252 and 86 / 87 on every route, s == kv and s == kv + 1, the rejected window result, the detours: each with
    the reference value it was placed for."""
    arcs = pr.expected_arcs(case)
    offs = case.offsets()
    for name, ((t, i), (tb, j), L) in case.named.items():
        got = arcs.get((int(offs[t] + i), int(offs[tb] + j)))
        if L is None:
            assert got is None, f'{case.name}: {name} has an arc {got}'
        else:
            assert got == (L, tb - t), f'{case.name}: {name} is {got}, placed for {L}'
    by_pair = {(p.t, p.i, p.t + p.gap, p.j): p for p in pr.model(case).pairs}
    for name, ((t, i), (tb, j), L) in case.named.items():
        p = by_pair[(t, i, tb, j)]
        if name.endswith('s_eq_kv'):
            assert p.route == 'front_off' and p.info['s'] == p.info['kv'], (case.name, name, p)
        if name.endswith('s_eq_kv_plus_1'):
            assert p.route == 'front_mask' and p.info['s'] == p.info['kv'] + 1, (case.name, name, p)
        if name == 'tie' or name == 'rejected':
            assert p.route == 'windowed', (case.name, name, p)
        if name in ('on_251', 'on_252', 'on_86', 'on_87'):
            assert p.route == ('plain' if case.name.startswith('F_65') else 'tight'), (case.name, name, p)
        if name in ('off_251', 'off_252', 'off_86', 'off_87'):
            assert p.route == ('front_mask' if pr.model(case).off_mode_ok else 'plain'), (case.name, name, p)


@pytest.mark.parametrize('conn8', [False, True])
def test_rejected_window_result_is_a_shorter_path_with_more_off_cells(conn8):
    """The pair 'rejected': the optimum has one off-mask cell and more than 251 cells; across the wall there is a path of
    4 cells with two off-mask cells, which a search limited to the window finds."""
    case = pr.case('D_rejected_window' + ('_conn8' if conn8 else ''))
    (sx, sy), (tx, ty) = case.frames[0][0], case.frames[1][0]
    assert pr.lengths_from(case.mask, conn8, sx, sy)[ty, tx] > 251
    assert (sx, sy + 3) == (tx, ty) and list(case.mask[sy:ty + 1, sx]) == [0, 0, 0, 1]      # 4 cells, two of them entered off the mask
    f = pr.fields(case)
    on_s = int(case.mask[sy, sx] == 1)
    assert min(f.off[a, sy, sx] - (1 - on_s) + f.off[a, ty, tx] for a in range(f.n_comp)) == 1       # kA = 1 < 2


@pytest.mark.parametrize('conn8', [False, True])
def test_saturation_sources(conn8):
    """The sources of case E see off-cell fields of 253, 254, 255 (saturated) and 255 (290 cells away); the last two have
    no component at all and run the all-off front only."""
    case = pr.case('E_saturation' + ('_conn8' if conn8 else ''))
    m = pr.model(case)
    info = [m.source_info[(0, i)] for i in range(4)]
    assert [min(s['v']) for s in info] == [253, 254, 255, 255]
    assert [s['best_comp'] for s in info] == [1, 1, 0, 0] and [s['best_a'] for s in info[:2]] == [252, 253]
    assert all(p.route in ('front_off', 'gate') for p in m.pairs if p.t == 0)


def test_all_ones_mask_has_the_closed_form():
    for conn8 in (False, True):
        case = pr.case('F_all_ones_mask' + ('_conn8' if conn8 else ''))
        x, y, _ = case.arrays()
        offs = case.offsets()
        for (a, b), (L, g) in pr.expected_arcs(case).items():
            t = int(np.searchsorted(offs, a, 'right') - 1)
            i, j = a - offs[t], b - offs[t + g]
            dx, dy = abs(int(x[t, i]) - int(x[t + g, j])), abs(int(y[t, i]) - int(y[t + g, j]))
            assert L == (max(dx, dy) if conn8 else dx + dy) + 1
