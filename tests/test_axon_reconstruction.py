"""Axon reconstructions: the links of the tracks (axt_track_links), one minimum-cost path per link (axt_link_paths /
axt_link_cells) and the public API on AxonDetections (reconstruction_arrays, get_axon_reconstructions, get_axon_growth;
the reference's stubs at AxonDetections.py:924-934, read by video_plotting.py:164-168,301-304)."""
import time

import numpy as np
import pandas as pd
import pytest

from axtrack_amd import synth, params
from axtrack_amd.detections import _interp_index, _recon_segments, _recon_frame, _growth_table
from recon_reference import open_staircase

MAX_DIST = 500


# ----------------------------------------------------------------------------------------------------- CPU only
def test_interp_index_rule_rounds_half_up():
    # k (L-1) / g: 1*4/2 = 2; 1*3/2 = 1.5 -> 2; 1*5/3 = 1.67 -> 2; 2*5/3 = 3.33 -> 3; 1*1/2 = 0.5 -> 1; L = 1 -> 0
    assert _interp_index(1, 5, 2) == 2
    assert _interp_index(1, 4, 2) == 2
    assert _interp_index(1, 6, 3) == 2 and _interp_index(2, 6, 3) == 3
    assert _interp_index(1, 2, 2) == 1
    assert _interp_index(1, 1, 2) == 0
    k, L, g = np.array([1, 1, 2]), np.array([10, 7, 7]), np.array([2, 3, 3])
    assert list(_interp_index(k, L, g)) == [5, 2, 4]          # 4.5 -> 5, 2, 4


def _hand_recon():
    """Two axons on a 10 x 12 grid: axon 3 in frames 0 -> 1 (gap 1, path of 3 cells) -> 3 (gap 2, 5 cells), axon 7 in
    frames 1 -> 3 (gap 2, no path)."""
    W = 12
    paths = [[(2, 1), (3, 1), (4, 1)], [(4, 1), (4, 2), (4, 3), (4, 4), (5, 4)]]
    cells = np.array([y * W + x for p in paths for (x, y) in p], np.int64)
    L = np.array([3, 5, MAX_DIST])
    r = dict(tail_frame=np.array([0, 1, 1]), head_frame=np.array([1, 3, 3]), axon_id=np.array([3, 3, 7]), gap=np.array([1, 2, 2]),
             len=L, cell_ptr=np.array([0, 3, 8, 8]), cells=cells, max_dist=MAX_DIST, shape=(10, W))
    # the interpolated frame of the gap link with a path: index 2 of 5 cells -> (4, 3)
    r.update(interp_axon_id=np.array([3]), interp_frame=np.array([2]), interp_x=np.array([4]), interp_y=np.array([3]),
             interp_link=np.array([1]), interp_index=np.array([2]))
    return r


def test_reconstruction_frame_on_hand_made_arrays():
    r = _hand_recon()
    df = _recon_frame(_recon_segments(r, True), r['cells'], r['shape'], None, None, True, 0, 0, 0, 0)
    assert df.columns.names == ['axonID', 'coord', 'frameID']
    assert list(df.columns.unique(0)) == ['Axon_003']                     # axon 7's only link has no path
    a = df['Axon_003']
    assert sorted(a.X.columns) == [1, 2, 3]
    assert list(a.X[1].dropna()) == [2, 3, 4] and list(a.Y[1].dropna()) == [1, 1, 1]
    assert list(a.X[2].dropna()) == [4, 4, 4] and list(a.Y[2].dropna()) == [1, 2, 3]      # up to the interpolated anchor
    assert list(a.X[3].dropna()) == [4, 4, 5] and list(a.Y[3].dropna()) == [3, 4, 4]
    # the reference consumer's expressions (video_plotting.py:301-304)
    draw_y = df['Axon_003'].Y.unstack().dropna().astype(int)
    draw_x = df['Axon_003'].X.unstack().dropna().astype(int)
    assert len(draw_y) == len(draw_x) == 9
    # without interpolation: the gap link is one segment at its head frame
    df = _recon_frame(_recon_segments(r, False), r['cells'], r['shape'], None, None, True, 0, 0, 0, 0)
    assert sorted(df['Axon_003'].X.columns) == [1, 3]
    assert list(df['Axon_003'].Y[3].dropna()) == [1, 2, 3, 4, 4]
    # t / include_history / names / cropping
    seg = _recon_segments(r, True)
    assert sorted(_recon_frame(seg, r['cells'], r['shape'], 2, None, True, 0, 0, 0, 0)['Axon_003'].X.columns) == [1, 2]
    assert sorted(_recon_frame(seg, r['cells'], r['shape'], 2, None, False, 0, 0, 0, 0)['Axon_003'].X.columns) == [2]
    assert _recon_frame(seg, r['cells'], r['shape'], None, ['Axon_007'], True, 0, 0, 0, 0).shape[1] == 0
    c = _recon_frame(seg, r['cells'], r['shape'], None, 'Axon_003', True, 2, 4, 3, 0)       # y in [2, 4), x >= 3
    assert c['Axon_003'].X[2].isna().tolist() == [True, False, False]
    assert list(c['Axon_003'].X[2].dropna()) == [1, 1] and list(c['Axon_003'].Y[2].dropna()) == [0, 1]


def test_growth_table_on_hand_made_arrays():
    r = _hand_recon()
    # IDed detections: axon 3 at frames 0, 1, 3; axon 7 at frames 1, 3
    frame, ids = np.array([0, 1, 1, 3, 3]), np.array([3, 3, 7, 3, 7])
    conf = np.array([.9, .8, .7, .95, .6], np.float32)
    x, y = np.array([2, 4, 9, 5, 9]), np.array([1, 1, 8, 4, 2])
    g = _growth_table(frame, ids, conf, x, y, r, _recon_segments(r, True), 0.5, 5.0)
    a = g.loc['Axon_003']
    assert list(a.index) == [0, 1, 2, 3]
    assert list(a.interpolated) == [False, False, True, False]
    assert np.isnan(a.conf[2]) and a.conf[3] == pytest.approx(.95)
    assert list(a.step_px) == [0, 2, 2, 2] and list(a.length_px) == [0, 2, 4, 6]
    assert (a.anchor_x[2], a.anchor_y[2]) == (4, 3)
    assert list(a.length_um) == [0, 1, 2, 3]
    assert a.speed_um_per_min[1] == pytest.approx(2 * 0.5 / 5.0) and np.isnan(a.speed_um_per_min[0])
    b = g.loc['Axon_007']
    assert b.step_px[1] == 0 and np.isnan(b.step_px[3]) and np.isnan(b.length_px[3])
    # without interpolation (as reconstruction_arrays(False) gives them: no interpolated frames): one step of 4 over two frames
    r = {k: (v[:0] if k.startswith('interp_') else v) for k, v in r.items()}
    g = _growth_table(frame, ids, conf, x, y, r, _recon_segments(r, False), 0.5, None)
    a = g.loc['Axon_003']
    assert list(a.index) == [0, 1, 3] and list(a.step_px) == [0, 2, 4] and 'speed_um_per_min' not in g.columns
    g = _growth_table(frame, ids, conf, x, y, r, _recon_segments(r, False), None, 5.0)
    assert 'length_um' not in g.columns and 'speed_um_per_min' not in g.columns


# ----------------------------------------------------------------------------------------------------- GPU
def _ad(d, H, W, P, mask=None, n_input=5, dt=None, pixelsize=None):
    import torch
    import axtrack_amd
    dev = torch.device('cuda', 0)
    tl = axtrack_amd.Timelapse(torch.zeros((n_input, H, W)), name='recon', mask=mask, device=dev, dt=dt, pixelsize=pixelsize)
    ad = axtrack_amd.AxonDetections(None, tl, P, None)
    ad.set_detections(*(torch.from_numpy(d[k]).to(dev) for k in ('conf', 'x', 'y', 'count')))
    return ad


def _params(conn8=False, assoc='mcf'):
    P = params.load_parameters()
    P['ASTAR_8_CONNECTED'] = conn8
    P['ASSOCIATION'] = assoc
    P['MCF_MAX_FLOW'] = 100000
    P['MCF_MIN_FLOW'] = 1
    return P


def _path(r, l):
    return r['cells'][r['cell_ptr'][l]:r['cell_ptr'][l + 1]]


def _expected_links(ad):
    frame, ids, _, _, _ = ad.ided_arrays()
    gaps = ad.P['MCF_MAX_NUM_MISSES'] + 1
    cnt, _, x, y = ad._host_dets()
    cap = ad.d_x.shape[1]
    track = ad._track_dev().cpu().numpy()
    out = set()
    for k in np.unique(ids):
        fr = np.sort(frame[ids == k])
        for f0, f1 in zip(fr[:-1], fr[1:]):
            if f1 - f0 <= gaps:
                i = int(np.nonzero(track[f0, :cnt[f0]] == k)[0][0]); j = int(np.nonzero(track[f1, :cnt[f1]] == k)[0][0])
                out.add((int(f0), i, int(f1), j, int(k)))
    return out


def _check_open(ad, conn8):
    r = ad.reconstruction_arrays()
    got = set(zip(r['tail_frame'].tolist(), r['tail_slot'].tolist(), r['head_frame'].tolist(), r['head_slot'].tolist(),
                  r['axon_id'].tolist()))
    assert got == _expected_links(ad) and len(got) == len(r['len'])
    assert np.all(np.diff(r['tail_frame'] * ad.d_x.shape[1] + r['tail_slot']) > 0)          # ascending tail order
    assert (r['gap'] == 2).sum() > 0, 'the scene should have misses'
    paths = ad.astar_dets_paths()
    cnt, _, x, y = ad._host_dets()
    W = ad.dataset.sizex
    for l in range(len(r['len'])):
        fa, i, fb, j = (int(r[k][l]) for k in ('tail_frame', 'tail_slot', 'head_frame', 'head_slot'))
        coo = paths[f'{ad.dataset.name}_t:{fb:0>3}-t:{fa:0>3}'][i][j]
        c = _path(r, l)
        if coo is None:
            assert r['len'][l] == MAX_DIST and len(c) == 0
            continue
        assert r['len'][l] == coo.getnnz() == len(c)
        assert set(c.tolist()) == set((coo.row * W + coo.col).tolist())
        assert np.array_equal(c, open_staircase(int(x[fa, i]), int(y[fa, i]), int(x[fb, j]), int(y[fb, j]), W, conn8))
    return r


@pytest.mark.gpu
@pytest.mark.parametrize('conn8', [False, True])
def test_open_grid_mcf_links_and_staircases(conn8):
    d = synth.synth_detections(40, 512, 512, n_alive=14, seed=3, p_detect=0.85)
    ad = _ad(d, 512, 512, _params(conn8))
    ad.assign_ids()
    _check_open(ad, conn8)


@pytest.mark.gpu
def test_open_grid_hungarian_links_and_staircases():
    d = synth.synth_detections(40, 512, 512, n_alive=14, seed=4, p_detect=0.85)
    ad = _ad(d, 512, 512, _params(False, 'hungarian'))
    ad.assign_ids()
    _check_open(ad, False)


def _graph(mask, conn8):
    from scipy.sparse import coo_matrix
    H, W = mask.shape
    wgt = np.where(mask, 1.0, 65536.0)
    idx = np.arange(H * W).reshape(H, W)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn8 else [])
    s, t, w = [], [], []
    for dy, dx in steps:
        ys, xs = np.mgrid[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)]
        s.append(idx[ys, xs].ravel()); t.append(idx[ys + dy, xs + dx].ravel()); w.append(wgt[ys + dy, xs + dx].ravel())
    return coo_matrix((np.concatenate(w), (np.concatenate(s), np.concatenate(t))), (H * W, H * W)).tocsr(), wgt


def _check_path_props(c, src, dst, W, conn8):
    assert c[0] == src and c[-1] == dst
    r, q = c // W, c % W
    dr, dq = np.abs(np.diff(r)), np.abs(np.diff(q))
    assert np.all((np.maximum(dr, dq) == 1) if conn8 else (dr + dq == 1))
    assert len(set(c.tolist())) == len(c)


def _check_masked(ad, mask_of_link, conn8, oracle=True, sample=None):
    """Every link's cells equal hp.path_cells of that single pair; lengths equal the oracle's; cost equals Dijkstra's."""
    import torch
    from axtrack_amd import hotpath as hp
    from oracle import oracle as orc
    from scipy.sparse.csgraph import dijkstra
    r = ad.reconstruction_arrays()
    cnt, _, x, y = ad._host_dets()
    H, W = ad.dataset.sizey, ad.dataset.sizex
    n = len(r['len'])
    ls = range(n) if sample is None else np.random.default_rng(0).choice(n, min(sample, n), replace=False)
    stats = dict(off_target=0, crosses=0, none=0)
    graphs = {}
    for l in ls:
        fa, i, fb, j = (int(r[k][l]) for k in ('tail_frame', 'tail_slot', 'head_frame', 'head_slot'))
        m = mask_of_link(fb)
        xa, ya, xb, yb = (np.array([v], np.int32) for v in (x[fa, i], y[fa, i], x[fb, j], y[fb, j]))
        c = _path(r, l)
        if m is None:
            assert np.array_equal(c, open_staircase(int(xa[0]), int(ya[0]), int(xb[0]), int(yb[0]), W, conn8))
            continue
        D, cells = hp.path_cells(*(torch.from_numpy(v).cuda() for v in (xa, ya, xb, yb)), H, W,
                                 torch.from_numpy(m.astype(np.uint8)).cuda(), MAX_DIST, conn8)
        D, cells = int(D.cpu()[0, 0]), cells.cpu().numpy()[0, 0]
        assert r['len'][l] == D
        if D >= MAX_DIST:
            stats['none'] += 1
            assert len(c) == 0
            continue
        assert np.array_equal(c, cells[:D])
        stats['off_target'] += int(not m[yb[0], xb[0]])
        stats['crosses'] += int((~m.ravel()[c[1:-1]]).any())
        _check_path_props(c, int(ya[0]) * W + int(xa[0]), int(yb[0]) * W + int(xb[0]), W, conn8)
        if oracle:
            ref = orc.path_matrix((None, xa, ya), (None, xb, yb), H, W, m, MAX_DIST, conn8)
            assert int(ref[0, 0]) == D
            key = m.tobytes()
            if key not in graphs:
                graphs[key] = _graph(m, conn8)
            G, wgt = graphs[key]
            best = dijkstra(G, indices=int(c[0]))
            assert wgt.ravel()[c[1:]].sum() == best[c[-1]]
    return r, stats


def _masked_scene(H=96, W=130):
    mask = synth.corridor_mask(H, W, width=10, pitch=34)
    mask[40:52, :] = False
    mask[44:47, 60:70] = True                                    # an island inside the gap
    return mask


@pytest.mark.gpu
@pytest.mark.parametrize('conn8', [False, True])
def test_masked_grid_link_paths_equal_path_cells(conn8):
    H, W = 96, 130
    mask = _masked_scene(H, W)
    d = synth.synth_detections(24, H, W, n_alive=6, seed=5, p_detect=0.85, max_step=14.0, min_dist=15)
    ad = _ad(d, H, W, _params(conn8), mask=mask)
    ad.assign_ids()
    r, stats = _check_masked(ad, lambda t: mask, conn8)
    assert len(r['len']) > 50
    assert stats['off_target'] > 0 and stats['crosses'] > 0, stats


@pytest.mark.gpu
def test_interpolation_anchors_and_split_segments():
    d = synth.synth_detections(40, 512, 512, n_alive=14, seed=3, p_detect=0.85)
    ad = _ad(d, 512, 512, _params(False))
    ad.assign_ids()
    before = ad.IDed_dets_all.copy()
    r = ad.reconstruction_arrays(True)
    W = 512
    gap2 = np.nonzero((r['gap'] == 2) & (r['len'] < MAX_DIST))[0]
    assert len(gap2) > 0 and len(r['interp_frame']) == len(gap2)
    for q, l in enumerate(r['interp_link']):
        c = _path(r, l)
        idx = (2 * (len(c) - 1) + 2) // 4
        assert r['interp_index'][q] == idx
        assert (r['interp_y'][q] * W + r['interp_x'][q]) == c[idx]
        assert r['interp_frame'][q] == r['tail_frame'][l] + 1
    df = ad.get_axon_reconstructions(interpolate_missing=True)
    df0 = ad.get_axon_reconstructions(interpolate_missing=False)
    for l in gap2:
        name = f"Axon_{int(r['axon_id'][l]):0>3}"
        fa, fb = int(r['tail_frame'][l]), int(r['head_frame'][l])
        c = _path(r, l)
        s1 = (df[name].Y[fa + 1].dropna() * W + df[name].X[fa + 1].dropna()).astype(int).to_numpy()
        s2 = (df[name].Y[fb].dropna() * W + df[name].X[fb].dropna()).astype(int).to_numpy()
        assert s1[-1] == s2[0] and np.array_equal(np.concatenate([s1, s2[1:]]), c)
        whole = (df0[name].Y[fb].dropna() * W + df0[name].X[fb].dropna()).astype(int).to_numpy()
        assert np.array_equal(whole, c) and (fa + 1) not in df0[name].X.columns
    assert ad.reconstruction_arrays(False)['interp_frame'].size == 0
    pd.testing.assert_frame_equal(ad.IDed_dets_all, before)


@pytest.mark.gpu
def test_identities_from_cache_give_the_same_reconstruction(tmp_path):
    import torch
    import axtrack_amd
    d = synth.synth_detections(30, 512, 512, n_alive=12, seed=8, p_detect=0.85)
    P = _params(False)
    dev = torch.device('cuda', 0)
    tl = axtrack_amd.Timelapse(torch.zeros((5, 512, 512)), name='recon', device=dev)
    a = axtrack_amd.AxonDetections(None, tl, P, str(tmp_path))
    a.set_detections(*(torch.from_numpy(d[k]).to(dev) for k in ('conf', 'x', 'y', 'count')))
    a.assign_ids(assigedIDs_cache='to')
    b = axtrack_amd.AxonDetections(None, tl, P, str(tmp_path))
    b.set_detections(*(torch.from_numpy(d[k]).to(dev) for k in ('conf', 'x', 'y', 'count')))
    b.assign_ids(assigedIDs_cache='from')
    ra, rb = a.reconstruction_arrays(), b.reconstruction_arrays()
    assert set(ra) == set(rb)
    for k in ra:
        if isinstance(ra[k], np.ndarray):
            assert np.array_equal(ra[k], rb[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize('quirk', [True, False])
def test_time_varying_mask_traces_each_link_on_its_frame_mask(quirk):
    H, W, F = 96, 130, 20
    base = _masked_scene(H, W)
    masks = np.stack([base if (t // 5) % 3 == 0 else (np.roll(base, 17, axis=1) if (t // 5) % 3 == 1 else np.ones_like(base))
                      for t in range(F + 4)])
    d = synth.synth_detections(F, H, W, n_alive=6, seed=6, p_detect=0.85, max_step=14.0, min_dist=15)
    P = _params(False)
    P['REPRODUCE_MASK_FRAME_QUIRK'] = quirk
    ad = _ad(d, H, W, P, mask=masks, n_input=F + 4)
    ad.assign_ids()
    groups, index = ad.dataset.mask_groups(quirk)
    r, _ = _check_masked(ad, lambda t: None if groups[index[t]].all() else groups[index[t]], False, oracle=False)
    assert len(set(index[r['head_frame']].tolist())) == 3


@pytest.mark.gpu
def test_reconstruction_format_for_the_reference_consumer():
    d = synth.synth_detections(20, 512, 512, n_alive=10, seed=9, p_detect=0.85)
    ad = _ad(d, 512, 512, _params(False))
    ad.assign_ids()
    r = ad.reconstruction_arrays()
    W = 512
    df = ad.get_axon_reconstructions()
    pd.testing.assert_frame_equal(ad._reconstruct_axons(), df)
    name = df.columns.unique(0)[0]
    k = int(name.split('_')[1])
    whole = ad.get_axon_reconstructions(interpolate_missing=False)          # every link's path once
    draw_y = whole[name].Y.unstack().dropna().astype(int)
    draw_x = whole[name].X.unstack().dropna().astype(int)
    want = np.concatenate([_path(r, l) for l in np.nonzero((r['axon_id'] == k) & (r['len'] < MAX_DIST))[0]])
    assert sorted((draw_y.to_numpy() * W + draw_x.to_numpy()).tolist()) == sorted(want.tolist())
    t = 10
    hist = ad.get_axon_reconstructions(t=t)
    assert hist.columns.get_level_values(2).max() <= t
    only = ad.get_axon_reconstructions(t=t, include_history=False)
    assert set(only.columns.get_level_values(2)) == {t}
    one = ad.get_axon_reconstructions(axon_name=name)
    assert list(one.columns.unique(0)) == [name]
    two = ad.get_axon_reconstructions(axon_name=list(df.columns.unique(0)[:2]))
    assert list(two.columns.unique(0)) == list(df.columns.unique(0)[:2])
    crop = ad.get_axon_reconstructions(ymin=100, ymax=300, xmin=50, xmax=400)
    X, Y = crop.xs('X', axis=1, level=1).to_numpy(), crop.xs('Y', axis=1, level=1).to_numpy()
    ok = ~np.isnan(X)
    assert ok.any() and (X[ok] >= 0).all() and (X[ok] < 350).all() and (Y[ok] >= 0).all() and (Y[ok] < 200).all()
    full = df.xs('X', axis=1, level=1).to_numpy()
    fy = df.xs('Y', axis=1, level=1).to_numpy()
    inside = (full >= 50) & (full < 400) & (fy >= 100) & (fy < 300)
    assert inside.sum() == ok.sum()


@pytest.mark.gpu
def test_growth_table_steps_lengths_and_units():
    d = synth.synth_detections(30, 512, 512, n_alive=12, seed=10, p_detect=0.85)
    ad = _ad(d, 512, 512, _params(True), pixelsize=0.62, dt=31.0)
    ad.assign_ids()
    g = ad.get_axon_growth()
    df = ad.get_axon_reconstructions()
    assert {'length_um', 'speed_um_per_min'} <= set(g.columns)
    frame, ids, _, _, _ = ad.ided_arrays()
    assert (~g.interpolated).sum() == len(frame)
    for name in df.columns.unique(0)[:10]:
        a = g.loc[name]
        for f in df[name].X.columns:
            n = df[name].X[f].notna().sum()
            assert a.step_px[f] == n - 1
        assert a.step_px.iloc[0] == 0
        assert np.allclose(a.length_px.to_numpy(), np.cumsum(a.step_px.to_numpy()), equal_nan=True)
        assert np.allclose(a.length_um, a.length_px * 0.62, equal_nan=True)
        span = np.diff(a.index.to_numpy())
        assert np.allclose(a.speed_um_per_min.to_numpy()[1:], a.step_px.to_numpy()[1:] * 0.62 / (31.0 * span), equal_nan=True)
    ad2 = _ad(d, 512, 512, _params(True))
    ad2.assign_ids()
    g2 = ad2.get_axon_growth()
    assert 'length_um' not in g2.columns and 'speed_um_per_min' not in g2.columns


@pytest.mark.gpu
def test_config5_share_all_links_reconstructed():
    import torch
    H = W = 1024
    mask = synth.corridor_mask(H, W)
    d = synth.synth_detections(64, H, W, n_alive=330, seed=0)
    ad = _ad(d, H, W, _params(False), mask=mask)
    ad.assign_ids()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = ad.reconstruction_arrays()
    torch.cuda.synchronize()
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    ad.get_axon_reconstructions()
    t_df = time.perf_counter() - t0
    print(f'\nconfig-5 share: {len(r["len"])} links, reconstruction_arrays {t_gpu * 1e3:.1f} ms, DataFrame {t_df * 1e3:.1f} ms')
    assert len(r['len']) == len(_expected_links(ad))
    cnt, _, x, y = ad._host_dets()
    has = np.nonzero(r['len'] < MAX_DIST)[0]
    assert len(has) > 0.9 * len(r['len'])
    for l in has:
        fa, i, fb, j = (int(r[k][l]) for k in ('tail_frame', 'tail_slot', 'head_frame', 'head_slot'))
        _check_path_props(_path(r, l), int(y[fa, i]) * W + int(x[fa, i]), int(y[fb, j]) * W + int(x[fb, j]), W, False)
    _check_masked(ad, lambda t: mask, False, oracle=False, sample=300)


@pytest.mark.gpu
def test_sharded_objects_refuse_reconstructions():
    d = synth.synth_detections(10, 512, 512, n_alive=8, seed=2)
    ad = _ad(d, 512, 512, _params(False))
    ad.assign_ids()
    ad._shard = (0, 5, None)
    with pytest.raises(NotImplementedError, match='single process'):
        ad.get_axon_reconstructions()
