"""Every route of the link-path and track-link kernels (axtrack_amd/csrc/recon.hip) against the reference of
tests/recon_reference.py: the classifier's gate, the breadth-first windows of radius 31 and 127, the key windows of radius
31 and 63 with their certificate, the exact whole-grid search, the staircase of the all-ones grid, and the launch shapes
of axt_track_links and axt_link_cells. tests/test_recon_routes_cpu.py proves on the CPU that each named pair reaches the
stage its name stands for; here the kernels run them: lengths, cell_ptr, cells and interpolation anchors must equal the
reference exactly, and the number of links each stage decides (AXT_PATH_DEBUG) must equal the dispatch model's."""
import re

import numpy as np
import pytest
import torch

import recon_reference as rr
from axtrack_amd import hotpath as hp

pytestmark = pytest.mark.gpu

_RUNS = {}
_STAGES = re.compile(r'link paths: (\d+) links selected: (\d+) gate, (\d+) bfs31, (\d+) bfs127, (\d+) key31, (\d+) key63, (\d+) exact')


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # (a copy: the battery's arrays are read-only)


def _run(case, monkeypatch, capfd):
    """The case through hp.link_paths, once per session: (len, cell_ptr, cells, interp, stage lines)."""
    if case.name in _RUNS:
        return _RUNS[case.name]
    monkeypatch.setenv('AXT_PATH_DEBUG', '1')
    x, y, links = case.arrays()
    H, W = case.shape
    grids = [None if m is None else hp.Grid(m, case.conn8) for m in case.masks]
    head_group = None if case.head_group is None else dev(np.asarray(case.head_group, np.int32))
    capfd.readouterr()
    out = hp.link_paths(dev(links), dev(x), dev(y), H, W, grids, head_group, case.max_dist, case.conn8, max_gap=2)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    _RUNS[case.name] = tuple(t.cpu().numpy().astype(np.int64) for t in out) + ([tuple(map(int, m)) for m in _STAGES.findall(err)],)
    return _RUNS[case.name]


def _differences(case, length, cell_ptr, cells):
    """The first differing pairs by name, each with the stage the dispatch model assigns to it."""
    lines = []
    for i, (p, want) in enumerate(zip(case.pairs, rr.expected_paths(case))):
        got = cells[cell_ptr[i]:cell_ptr[i + 1]] if 0 < length[i] < case.max_dist else None
        if length[i] != (case.max_dist if want is None else len(want)) or not (
                (got is None and want is None) or (got is not None and want is not None and np.array_equal(got, want))):
            lines.append(f'{p.name} {p.S} -> {p.T}, route {rr.route(case, i)}: kernel len {length[i]} cells '
                         f'{None if got is None else got.tolist()}, reference {None if want is None else want.tolist()}')
    return f'{case.name}: {len(lines)} pairs differ:\n' + '\n'.join(lines[:8])


@pytest.mark.parametrize('case', rr.battery(), ids=repr)
def test_link_paths_equal_the_reference(case, monkeypatch, capfd):
    """len, cell_ptr, cells and interp of hp.link_paths equal the reference's: every pair, no tolerance."""
    length, cell_ptr, cells, interp, _ = _run(case, monkeypatch, capfd)
    w_len, w_ptr, w_cells, w_interp = rr.expected_arrays(case)
    same = (np.array_equal(length, w_len) and np.array_equal(cell_ptr, w_ptr) and np.array_equal(cells, w_cells))
    assert same, _differences(case, length, cell_ptr, cells)
    assert np.array_equal(interp, w_interp), f'{case.name}: anchors differ at links {np.argwhere(interp != w_interp)[:8].tolist()}'


@pytest.mark.parametrize('case', rr.battery(), ids=repr)
def test_stage_counts_equal_the_dispatch_model(case, monkeypatch, capfd):
    """The links each stage decides are as many as the model says, one line per masked grid of the case."""
    lines = _run(case, monkeypatch, capfd)[4]
    assert len(lines) == sum(m is not None for m in case.masks), f'{case.name}: stage lines {lines}'
    want, n = rr.stage_counts(case)
    got = dict(zip(rr.ROUTES, np.sum([l[1:] for l in lines], 0).tolist()))
    assert (sum(l[0] for l in lines), got) == (n, want), f'{case.name}: kernels {got}, model {want}'


@pytest.mark.parametrize('case', [c for c in rr.battery() if c.head_group is None], ids=repr)
def test_path_cells_gives_the_same_cells(case):
    """The same pairs through hp.path_cells (the exact search alone): the same lengths and cells."""
    H, W = case.shape
    mask = case.masks[0]
    sources = sorted({p.S for p in case.pairs})
    targets = sorted({p.T for p in case.pairs})
    xy = lambda pts: (dev(np.array([q[0] for q in pts], np.int32)), dev(np.array([q[1] for q in pts], np.int32)))
    D, cells = hp.path_cells(*xy(sources), *xy(targets), H, W, dev(mask), case.max_dist, case.conn8)
    D, cells = D.cpu().numpy(), cells.cpu().numpy()
    for p in case.pairs:
        i, j = sources.index(p.S), targets.index(p.T)
        want = rr.expected_paths(case)[case.pairs.index(p)]
        if want is None:
            assert D[i, j] == case.max_dist and (cells[i, j] == -1).all(), f'{case.name}: {p.name}'
        else:
            assert D[i, j] == len(want) and np.array_equal(cells[i, j, :D[i, j]], want) and (cells[i, j, D[i, j]:] == -1).all(), \
                f'{case.name}: {p.name}: kernel {cells[i, j, :D[i, j]].tolist()}, reference {want.tolist()}'


@pytest.mark.parametrize('max_gap', [1, 2, 3])
def test_track_links_equal_the_reference(max_gap):
    """hp.track_links on 1030 frames (two per partition of the scan) of up to 300 slots (two chunks of the compaction, a
    count above cap): the same rows in the same order."""
    track, count = rr.links_table()
    got = hp.track_links(dev(track), dev(count), max_gap).cpu().numpy()
    want = rr.track_links(track, count, max_gap)
    assert got.shape == want.shape, f'{len(got)} links, reference {len(want)}'
    assert np.array_equal(got, want), f'first differing rows {np.flatnonzero((got != want).any(1))[:8].tolist()}'


@pytest.mark.parametrize('case', rr.cells_battery(), ids=repr)
def test_link_cells_equal_the_reference(case):
    """hp.link_paths on the all-ones grid with more links than the scan has partitions, paths longer than the fill's 64
    threads, links without a path mixed in and gaps 1 .. max_gap: len, cell_ptr, cells and anchors equal the reference's."""
    H, W = case.shape
    out = hp.link_paths(dev(case.links), dev(case.x), dev(case.y), H, W, [None], None, case.max_dist, case.conn8, max_gap=case.max_gap)
    length, cell_ptr, cells, interp = (t.cpu().numpy().astype(np.int64) for t in out)
    w_len, w_ptr, w_cells, w_interp = case.expected()
    assert np.array_equal(length, w_len), f'lengths differ at links {np.flatnonzero(length != w_len)[:8].tolist()}'
    assert np.array_equal(cell_ptr, w_ptr), f'cell_ptr differs from entry {np.flatnonzero(cell_ptr != w_ptr)[:1].tolist()}'
    assert np.array_equal(cells, w_cells), f'cells differ from {np.flatnonzero(cells != w_cells)[:1].tolist()}'
    assert interp.shape == w_interp.shape and np.array_equal(interp, w_interp), \
        f'anchors differ at {np.argwhere(interp != w_interp)[:8].tolist()}'
