"""Every dispatch path of the masked-grid path-length searches (axtrack_amd/csrc/path_bfs.hip) against the Dijkstra reference
of tests/pathsearch_reference.py: sources on the mask (tight steps), off it (two fronts), the plain dilation, the windowed
and the general search, at the edges only the kernels have -- word carries of the bit-parallel dilation, the floor-aligned
and clipped window, W % 32, lengths exactly at dmax and at the 250-move depth, saturated off-cell fields, the LDS layout at
its limit. tests/test_pathsearch_cpu.py proves on the CPU that each case lands in the route its name claims; here the kernels
run them: the arcs must equal the reference set exactly, and the numbers of sources the kernels hand to the windowed and the
general search (AXT_PATH_DEBUG) must equal what the dispatch model predicts."""
import re

import numpy as np
import pytest
import torch

import hungarian_reference as hr
import pathsearch_reference as pr
import recon_reference as rr
from axtrack_amd import hotpath as hp, params

pytestmark = pytest.mark.gpu

_RUNS = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _environment(case, monkeypatch):
    monkeypatch.delenv('AXT_PATH_NO_OFFMODE', raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


def _run(case, monkeypatch, capfd):
    """The case through hp.build_arcs, once per session: ({(tail, head): (length, gap)}, n windowed, n general, duplicates)."""
    if case.name in _RUNS:
        return _RUNS[case.name]
    _environment(case, monkeypatch)
    monkeypatch.setenv('AXT_PATH_DEBUG', '1')
    x, y, cnt = case.arrays()
    H, W = case.shape
    grid = hp.Grid(case.mask, case.conn8)
    src = dev(np.asarray(case.src_count, np.int32)) if case.src_count is not None else None
    capfd.readouterr()
    row_ptr, col, length, gap, _ = hp.build_arcs(dev(x), dev(y), dev(cnt), H, W, case.dmax, None, grid, case.max_dist, case.conn8,
                                                 src_count=src)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    n_det = int(case.offsets()[-1])
    rp = row_ptr[:n_det + 1].cpu().numpy()
    col, length, gap = col.cpu().numpy(), length.cpu().numpy(), gap.cpu().numpy()
    assert rp[0] == 0 and rp[-1] == len(col) and (np.diff(rp) >= 0).all()
    tail = np.searchsorted(rp, np.arange(len(col)), 'right') - 1
    arcs = {(int(a), int(b)): (int(d), int(g)) for a, b, d, g in zip(tail, col, length, gap)}
    m = re.search(r'masked arcs: (\d+) sources off the mask or without component fields \(windowed search\)', err)
    n = re.search(r'masked arcs: (\d+) sources left for the general search', err)
    # the first pass counts, the second fills: the table is built once, so each line appears at most once
    _RUNS[case.name] = (arcs, int(m.group(1)) if m else 0, int(n.group(1)) if n else 0, len(col) - len(arcs))
    return _RUNS[case.name]


def _differences(case, got, want):
    """The first differing pairs, each with the route the dispatch model assigns to it."""
    offs = case.offsets()
    route = {(int(offs[p.t] + p.i), int(offs[p.t + p.gap] + p.j)): (p.route, p.info) for p in pr.model(case).pairs}
    x, y, _ = case.arrays()

    def where(k):
        t = int(np.searchsorted(offs, k, 'right') - 1)
        return f'frame {t} slot {int(k - offs[t])} ({x[t, k - offs[t]]},{y[t, k - offs[t]]})'

    lines = []
    for k in sorted(set(got) | set(want)):
        if got.get(k) != want.get(k):
            lines.append(f'{where(k[0])} -> {where(k[1])}: kernel {got.get(k)}, reference {want.get(k)}, route {route.get(k)}')
    return f'{case.name}: {len(lines)} pairs differ (length, gap):\n' + '\n'.join(lines[:12])


@pytest.mark.parametrize('case', pr.battery(), ids=repr)
def test_arcs_equal_the_reference(case, monkeypatch, capfd):
    """The set of (tail, head, length, gap) of hp.build_arcs on the masked grid equals the reference set: no pair left out,
    no tolerance."""
    got, _, _, dup = _run(case, monkeypatch, capfd)
    want = pr.expected_arcs(case)
    assert dup == 0, f'{case.name}: {dup} arcs listed twice'
    assert got == want, _differences(case, got, want)


@pytest.mark.parametrize('case', pr.battery(), ids=repr)
def test_route_counts_equal_the_dispatch_model(case, monkeypatch, capfd):
    """The sources the kernels hand to the windowed and to the general search are as many as the model says: the model that
    proves the battery's coverage describes what the kernels really dispatch."""
    _, n_windowed, n_general, _ = _run(case, monkeypatch, capfd)
    m = pr.model(case)
    assert (n_windowed, n_general) == (m.n_windowed, m.n_general), f'{case.name}: kernels (windowed, general) = ' \
        f'{(n_windowed, n_general)}, model {(m.n_windowed, m.n_general)}'


def test_lds_limit_cases_agree(monkeypatch, capfd):
    """The same anchors in the last slots at cap 1157 (four bitmaps: 159 KiB of LDS exactly), cap 1158 (three bitmaps) and
    at cap 8 without the two fronts: one arc set, whatever the layout."""
    sets = []
    for name in ('G_cap1157_four_bitmaps', 'G_cap1158_three_bitmaps', 'G_cap8_no_offmode'):
        case = pr.case(name)
        rank = {t * case.cap + s: (t, k) for t in range(len(case.frames)) for k, s in enumerate(case.slots(t))}
        sets.append({(rank[a], rank[b]): v for (a, b), v in _run(case, monkeypatch, capfd)[0].items()})
    assert sets[0] == sets[1] == sets[2] and len(sets[0]) > 0


def _link_costs(case):
    """{(t, gap): i64 [n, m]} link costs from the REFERENCE lengths, as hungarian_reference.geometric_costs builds them from
    the oracle's."""
    from oracle import oracle as orc
    P = orc.DEFAULTS
    counts = [len(f) for f in case.frames]
    offs = hr.offsets(counts)
    out = {}
    for g in (1, 2):
        for t in range(len(counts) - g):
            n, m = counts[t], counts[t + g]
            D = np.array([[pr.path_length(case.mask, case.conn8, sx, sy, tx, ty, case.max_dist) for tx, ty in case.frames[t + g]]
                          for sx, sy in case.frames[t]], np.int32).reshape(n, m)
            c = orc.transition_cost(D, g, P['MCF_MISS_RATE'])
            adm = c < P['MCF_EDGE_COST_THR']
            units = np.rint(np.where(adm, c, 0.0) * orc.COST_SCALE).astype(np.int64)
            cost = hr.arc_cost_vec(units, 3, offs[t] + np.arange(n)[:, None], offs[t + g] + np.arange(m)[None, :])
            out[(t, g)] = np.where(adm, cost, hr.NO_LINK)
    return out


@pytest.mark.parametrize('case', [c for c in pr.battery() if c.group in 'ADF'], ids=repr)
def test_hungarian_on_the_same_table(case, monkeypatch):
    """hp.hungarian_assoc fills the same path-length table (axt_hungarian_pairs with a grid): judged by hungarian_reference.judge
    on costs taken from the reference lengths."""
    from axtrack_amd.detections import transition_cost_table
    _environment(case, monkeypatch)
    table, dmax = transition_cost_table(params.DEPLOYED)
    assert [int(d) for d in dmax] == case.dmax
    units = np.where(np.isfinite(table), np.rint(table * 1e6), 0).astype(np.int64)
    x, y, cnt = case.arrays()
    H, W = case.shape
    track, n = hp.hungarian_assoc(dev(x), dev(y), dev(cnt), H, W, dmax, units, hr.THR_UNITS, conn8=case.conn8,
                                  mask=hp.Grid(case.mask, case.conn8))
    torch.cuda.synchronize()
    hr.judge(_link_costs(case), [len(f) for f in case.frames], track.cpu().numpy(), int(n.item()), name=case.name)


def _xy(points):
    return dev(np.array([p[0] for p in points], np.int32)), dev(np.array([p[1] for p in points], np.int32))


@pytest.mark.parametrize('case', pr.battery_x(), ids=repr)
def test_exact_search_lengths(case):
    """hp.path_cost on its own: optimum lengths 499, 500 and 501 at max_dist = 500, the staircase 4- and 8-connected."""
    H, W = case.mask.shape
    D = hp.path_cost(*_xy(case.sources), *_xy(case.targets), H, W, dev(case.mask), case.max_dist, case.conn8).cpu().numpy()
    want = case.expected()
    assert np.array_equal(D, want), f'{case.name}: kernel\n{D}\nreference\n{want}'


@pytest.mark.parametrize('case', pr.battery_x(), ids=repr)
def test_exact_search_paths(case):
    """hp.path_cells: every path starts at its source, ends at its target, moves between neighbouring cells, visits no cell
    twice, has the reference's number of cells and costs exactly what the reference's Dijkstra finds; and its cells are
    the reference walk's (recon_reference.path_cells): among equally cheap paths the one the neighbour order of csrc/grid.h
    fixes."""
    H, W = case.mask.shape
    D, cells = hp.path_cells(*_xy(case.sources), *_xy(case.targets), H, W, dev(case.mask), case.max_dist, case.conn8)
    D, cells = D.cpu().numpy(), cells.cpu().numpy()
    assert np.array_equal(D, case.expected())
    wgt = np.where(case.mask == 1, 1, pr.OFF).astype(np.int64).ravel()
    checked = 0
    for i, (sx, sy) in enumerate(case.sources):
        for j, (tx, ty) in enumerate(case.targets):
            if D[i, j] >= case.max_dist:
                assert (cells[i, j] == -1).all()
                continue
            c = cells[i, j, :D[i, j]]
            assert (cells[i, j, D[i, j]:] == -1).all()
            assert c[0] == sy * W + sx and c[-1] == ty * W + tx
            r, q = c // W, c % W
            dr, dq = np.abs(np.diff(r)), np.abs(np.diff(q))
            assert np.all((np.maximum(dr, dq) == 1) if case.conn8 else (dr + dq == 1))
            assert len(set(c.tolist())) == len(c)
            assert wgt[c[1:]].sum() == pr.costs_from(case.mask, case.conn8, sx, sy)[ty, tx]
            want = rr.path_cells(case.mask, case.conn8, sx, sy, tx, ty, case.max_dist)
            assert np.array_equal(c, want), f'{case.name}: {(sx, sy)} -> {(tx, ty)}: kernel {c.tolist()}, reference {want.tolist()}'
            checked += 1
    assert checked >= 4
