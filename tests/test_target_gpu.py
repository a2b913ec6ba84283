"""Target screens on the GPU (axt_target_field / axt_target_sample / axt_target_paths, the API on AxonDetections and the
target layer of render_frames) against tests/target_reference.py: SciPy's Dijkstra on the reversed grid graph and the
walk rule in numpy. Integer results are compared for equality; there are no tolerances."""
import colorsys

import numpy as np
import pytest

import target_reference as tr
from axtrack_amd import synth, params

pytestmark = pytest.mark.gpu
TC = 2
BOX = 70


def _dev(a, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _field(mask, cells, conn8, rounds=False):
    from axtrack_amd import hotpath as hp
    H, W = mask.shape
    m = None if mask.all() else mask
    out = hp.target_field(_dev(cells), H, W, m, conn8, return_rounds=True)
    off, moves = out[0].cpu().numpy(), out[1].cpu().numpy()
    return (off, moves, out[2]) if rounds else (off, moves)


def _on_off(mask):
    ys, xs = np.nonzero(mask)
    k = len(ys) // 2
    yo, xo = np.nonzero(~mask) if not mask.all() else (ys, xs)
    j = len(yo) // 3
    return (int(ys[k]), int(xs[k])), (int(yo[j]), int(xo[j]))


def _edge_block(mask):
    """A 5 x 5 block of target cells that straddles a mask edge (on an all-ones mask: any block)."""
    H, W = mask.shape
    edge = mask[:, 1:] != mask[:, :-1]
    ys, xs = np.nonzero(edge[2:H - 3, 2:W - 4])
    y, x = (int(ys[len(ys) // 2]) + 2, int(xs[len(xs) // 2]) + 2) if len(ys) else (H // 2, W // 2)
    yy, xx = np.mgrid[y - 2:y + 3, x - 1:x + 4]
    return np.stack([yy.ravel(), xx.ravel()], 1)


MASKS = {
    'ones': lambda: np.ones((96, 130), bool),
    'corridor': lambda: synth.corridor_mask(512, 512),
    'serpentine': lambda: tr.serpentine_mask(256, 256, 12, 24),
    'blobs': lambda: tr.blob_mask(200, 312, seed=7),
}


# ---------------------------------------------------------------------------------------------- 1, 2: the field
@pytest.mark.parametrize('conn8', [False, True])
@pytest.mark.parametrize('name', list(MASKS))
def test_field_equals_the_reference_in_every_cell(name, conn8):
    mask = MASKS[name]()
    H, W = mask.shape
    if name == 'blobs':
        from scipy.ndimage import label
        assert label(mask)[1] >= 3 and label(~mask)[1] >= 2, 'the blob mask should have several components and holes'
    on, off_cell = _on_off(mask)
    block = _edge_block(mask)
    if not mask.all():
        assert mask[on] and not mask[off_cell]
        assert mask[block[:, 0], block[:, 1]].any() and not mask[block[:, 0], block[:, 1]].all()
    targets = {'on-mask cell': [on], 'off-mask cell': [off_cell], 'block across a mask edge': block,
               'two distant cells': [(3, 5), (H - 4, W - 7)], 'border cell': [(H - 1, W // 3)]}
    for what, t in targets.items():
        cells = tr.target_cells(t, W)
        off, moves = _field(mask, cells, conn8)
        roff, rmoves = tr.field(mask, cells, conn8)
        bad = np.argwhere((off != roff) | (moves != rmoves))
        assert len(bad) == 0, (f'{name}, {what}, conn8={conn8}: {len(bad)} cells differ, first {bad[0].tolist()}: '
                               f'({off[tuple(bad[0])]}, {moves[tuple(bad[0])]}) vs ({roff[tuple(bad[0])]}, {rmoves[tuple(bad[0])]})')


def test_field_is_byte_identical_from_run_to_run():
    mask = MASKS['corridor']()
    cells = tr.target_cells([(256, 256), (17, 400)], 512)
    a = _field(mask, cells, True)
    for _ in range(3):
        b = _field(mask, cells, True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---------------------------------------------------------------------------------------------- 3: the package's lengths
@pytest.mark.parametrize('conn8', [False, True])
def test_moves_agree_with_path_cost_of_every_detection(conn8):
    import torch
    from axtrack_amd import hotpath as hp
    H = W = 512
    mask = synth.corridor_mask(H, W)
    d = synth.synth_detections(24, H, W, n_alive=75, seed=3)
    valid = np.arange(d['x'].shape[1])[None, :] < d['count'][:, None]
    x, y = d['x'][valid], d['y'][valid]
    assert len(x) == 1525 and int((~mask[y, x]).sum()) == 830
    off, moves = hp.target_field(_dev([256 * W + 256]), H, W, mask, conn8)
    D = hp.path_cost(_dev(x), _dev(y), _dev([256]), _dev([256]), H, W, torch.from_numpy(mask.astype(np.uint8)), 500, conn8)
    D = D.cpu().numpy()[:, 0]
    assert (D < 500).all(), 'every detection passes the 500 gate: none is excluded'
    got = moves.cpu().numpy()[y, x] + 1
    assert np.array_equal(got, D)


# ---------------------------------------------------------------------------------------------- 4, 5: sampling and paths
@pytest.mark.parametrize('conn8', [False, True])
def test_samples_and_paths_equal_the_reference_walk(conn8):
    import torch
    from axtrack_amd import hotpath as hp
    H, W = 200, 312
    mask = tr.blob_mask(H, W, seed=7)
    d = synth.synth_detections(6, H, W, n_alive=20, seed=9, min_dist=12)
    x, y, count = d['x'].copy(), d['y'].copy(), d['count']
    # detections outside the grid (the decode does not clamp) and slots beyond the count
    x[0, 0], y[1, 1], x[2, 0], y[2, 0] = -4, H + 2, W, -1
    target = np.array([[150, 40], [150, 41], [20, 300]])
    cells = tr.target_cells(target, W)
    off, moves = hp.target_field(_dev(cells), H, W, mask, conn8)
    roff, rmoves = tr.field(mask, cells, conn8)
    d_off, d_moves = hp.target_sample(off, moves, _dev(x), _dev(y), _dev(count))
    F, cap = x.shape
    valid = np.arange(cap)[None, :] < count[:, None]
    eo, em = tr.sample(roff, rmoves, x, y)
    eo, em = np.where(valid, eo, -1), np.where(valid, em, -1)
    assert np.array_equal(d_off.cpu().numpy(), eo) and np.array_equal(d_moves.cpu().numpy(), em)
    assert (em[0, 0], em[1, 1], em[2, 0]) == (-1, -1, -1) and (em[valid] >= 0).sum() == valid.sum() - 3
    grid = hp.Grid(mask, conn8)
    ptr, pc = hp.target_paths([(off, moves)], [grid], _dev(x), _dev(y), d_moves, H, W, None, conn8)
    ptr, pc = ptr.cpu().numpy(), pc.cpu().numpy()
    assert np.array_equal(np.diff(ptr), (em + 1).ravel()) and ptr[0] == 0 and ptr[-1] == len(pc)     # lengths are moves + 1
    tset = set(cells.tolist())
    n_off = 0
    for f in range(F):
        for i in range(cap):
            c = pc[ptr[f * cap + i]:ptr[f * cap + i + 1]].astype(np.int64)
            if em[f, i] < 0:
                assert len(c) == 0                                   # outside the grid or an empty slot: no path
                continue
            assert c[0] == y[f, i] * W + x[f, i] and int(c[-1]) in tset
            r, q = c // W, c % W
            dr, dq = np.abs(np.diff(r)), np.abs(np.diff(q))
            assert np.all((np.maximum(dr, dq) == 1) if conn8 else (dr + dq == 1))
            assert tr.path_key(mask, c) == (eo[f, i], em[f, i])
            assert np.array_equal(c, tr.walk(mask, roff, rmoves, int(y[f, i]), int(x[f, i]), conn8))
            n_off += eo[f, i] > 0
    assert n_off > 0, 'some paths should cross off-mask cells'
    # all-ones mask: grid = None
    off1, moves1 = hp.target_field(_dev(cells), H, W, None, conn8)
    o1, m1 = hp.target_sample(off1, moves1, _dev(x), _dev(y), _dev(count))
    ptr1, pc1 = hp.target_paths([(off1, moves1)], [None], _dev(x), _dev(y), m1, H, W, None, conn8)
    ones = np.ones((H, W), bool)
    r1 = tr.field(ones, cells, conn8)
    ptr1, pc1 = ptr1.cpu().numpy(), pc1.cpu().numpy()
    for s in np.nonzero(valid.ravel())[0][::7]:
        f, i = divmod(int(s), cap)
        assert np.array_equal(pc1[ptr1[s]:ptr1[s + 1]], tr.walk(ones, r1[0], r1[1], int(y[f, i]), int(x[f, i]), conn8))


# ---------------------------------------------------------------------------------------------- 6, 7: the public API
def _ad(d, H, W, mask=None, conn8=False, pixelsize=None, dt=None, frames=None):
    import torch
    import axtrack_amd
    dev = torch.device('cuda', 0)
    F = len(d['count'])
    if frames is None:
        frames = torch.zeros((F + 2 * TC, H, W))
    tl = axtrack_amd.Timelapse(frames, name='target', mask=mask, device=dev, pixelsize=pixelsize, dt=dt)
    P = params.load_parameters()
    P['ASTAR_8_CONNECTED'] = conn8
    P['MCF_MAX_FLOW'] = 100000
    P['MCF_MIN_FLOW'] = 1
    ad = axtrack_amd.AxonDetections(None, tl, P, None)
    ad.set_detections(*(torch.from_numpy(d[k]).to(dev) for k in ('conf', 'x', 'y', 'count')))
    ad.assign_ids()
    return ad


def _scene_mask(H=96, W=130):
    mask = synth.corridor_mask(H, W, width=10, pitch=34)
    mask[40:52, :] = False
    mask[44:47, 60:70] = True
    return mask


def _expected_tables(ad, field_of_frame):
    """The builders fed from the reference: field_of_frame(t) -> (off, moves)."""
    from axtrack_amd.detections import _target_table, _target_summary
    frame, ids, conf, x, y = ad.ided_arrays()
    off, moves = np.zeros(len(frame), np.int64), np.zeros(len(frame), np.int64)
    for t in np.unique(frame):
        sel = frame == t
        off[sel], moves[sel] = tr.sample(*field_of_frame(int(t)), x[sel], y[sel])
    table = _target_table(frame, ids, conf, x, y, off, moves, ad.reach_px, ad.dataset.pixelsize, ad.dataset.dt)
    return table, _target_summary(frame, ids, moves, ad.reach_px), (frame, ids, x, y, off, moves)


@pytest.mark.parametrize('conn8', [False, True])
def test_public_api_on_a_tracked_scene(conn8):
    import pandas as pd
    H, W = 96, 130
    mask = _scene_mask(H, W)
    d = synth.synth_detections(24, H, W, n_alive=6, seed=5, p_detect=0.85, max_step=14.0, min_dist=15)
    d['x'][3, 0] = -2                                                 # one detection outside the grid
    ad = _ad(d, H, W, mask, conn8, pixelsize=0.5, dt=5.0)
    with pytest.raises(ValueError, match='no target'):
        ad.get_target_distances()
    ref = tr.field(mask, [4 * W + 20], conn8)
    valid = np.arange(d['x'].shape[1])[None, :] < d['count'][:, None]
    reach = int(np.median(tr.sample(*ref, d['x'][valid], d['y'][valid])[1]))      # some detections within reach, some not
    ad.set_target((4, 20), reach_px=reach)
    assert ad.structure_outputchannel_coo == (4, 20) and ad.reach_px == reach
    off, moves = ad.target_field()
    assert np.array_equal(off.cpu().numpy(), ref[0]) and np.array_equal(moves.cpu().numpy(), ref[1])
    assert ad.target_field()[1] is moves                              # cached
    table, summary, arrays = _expected_tables(ad, lambda t: ref)
    for a, b in zip(ad.target_arrays(), arrays):
        assert np.array_equal(a, b)
    got = ad.get_target_distances()
    pd.testing.assert_frame_equal(got, table)
    assert got.target_dist_px.isna().sum() == (arrays[5] < 0).sum() <= 1 and got.reached.any() and not got.reached.all()
    assert {'target_dist_um', 'approach_um_per_min'} <= set(got.columns)
    pd.testing.assert_frame_equal(ad.get_target_summary(), summary)
    # get_trg_path: the reference walk of every IDed detection of the frame, cropped and shifted
    frame, ids, x, y, _, m = arrays
    for t in (0, 3, 11, 23):
        sel = frame == t
        paths = ad.get_trg_path(t)
        assert sorted(paths) == sorted(f'Axon_{k:0>3}' for k, mm in zip(ids[sel], m[sel]) if mm >= 0)
        for k, xx, yy, mm in zip(ids[sel], x[sel], y[sel], m[sel]):
            if mm < 0:
                continue
            c = tr.walk(mask, ref[0], ref[1], int(yy), int(xx), conn8)
            ys, xs = paths[f'Axon_{k:0>3}']
            assert np.array_equal(ys, c // W) and np.array_equal(xs, c % W) and ys.dtype.kind == 'i'
            crop = ad.get_trg_path(t, axon_name=f'Axon_{k:0>3}', ymin=10, ymax=70, xmin=5)
            keep = (c // W >= 10) & (c // W < 70) & (c % W >= 5)
            assert list(crop) == [f'Axon_{k:0>3}']
            assert np.array_equal(crop[f'Axon_{k:0>3}'][0], (c // W)[keep] - 10) and np.array_equal(crop[f'Axon_{k:0>3}'][1], (c % W)[keep] - 5)
    # changing the target invalidates the cache
    region = np.zeros((H, W), bool)
    region[60:64, 100:110] = True
    ad.set_target(region)
    assert ad.reach_px == BOX // 2
    ref2 = tr.field(mask, np.nonzero(region.ravel())[0], conn8)
    assert np.array_equal(ad.target_field()[1].cpu().numpy(), ref2[1]) and not np.array_equal(ref2[1], ref[1])
    pd.testing.assert_frame_equal(ad.get_target_distances(), _expected_tables(ad, lambda t: ref2)[0])
    # a frame-sharded object refuses
    ad._shard = (0, 12)
    for call in (ad.target_field, ad.target_arrays, ad.get_target_distances, ad.get_target_summary, lambda: ad.get_trg_path(0)):
        with pytest.raises(NotImplementedError):
            call()


def test_time_varying_mask_reads_each_frames_own_field():
    import pandas as pd
    from oracle import oracle as orc
    F, H, W = 8, 96, 130
    a, b = _scene_mask(H, W), synth.corridor_mask(H, W, width=14, pitch=40)
    m3 = np.stack([a if k < 5 else b for k in range(F + 2 * TC)])
    d = synth.synth_detections(F, H, W, n_alive=6, seed=6, min_dist=15)
    ad = _ad(d, H, W, m3)
    assert ad.dataset.mask3d is not None
    ad.set_target((50, 64))
    with pytest.raises(ValueError, match='frame index'):
        ad.target_field()
    refs = {}

    def field_of_frame(t):
        m = orc.mask_of_frame(m3, t, True)
        return refs.setdefault(m.tobytes(), tr.field(m, [50 * W + 64], False))
    table, summary, arrays = _expected_tables(ad, field_of_frame)
    assert len(refs) == 2, 'two distinct masks'
    for t in (0, 4, 5, 7):
        assert np.array_equal(ad.target_field(t)[1].cpu().numpy(), field_of_frame(t)[1])
    pd.testing.assert_frame_equal(ad.get_target_distances(), table)
    pd.testing.assert_frame_equal(ad.get_target_summary(), summary)
    frame, ids, x, y, _, _ = arrays
    for t in (2, 6):
        sel = frame == t
        paths = ad.get_trg_path(t)
        ro, rm = field_of_frame(t)
        for k, xx, yy in zip(ids[sel], x[sel], y[sel]):
            c = tr.walk(orc.mask_of_frame(m3, t, True), ro, rm, int(yy), int(xx), False)
            assert np.array_equal(paths[f'Axon_{k:0>3}'][0], c // W) and np.array_equal(paths[f'Axon_{k:0>3}'][1], c % W)


# ---------------------------------------------------------------------------------------------- 8: full size
@pytest.mark.parametrize('conn8', [False, True])
@pytest.mark.parametrize('name', ['corridor', 'serpentine'])
def test_full_size_fields_equal_the_reference(name, conn8):
    H = W = 1024
    mask = synth.corridor_mask(H, W) if name == 'corridor' else tr.serpentine_mask(H, W, 24, 48)
    cells = [5 * W + 5]
    roff, rmoves = tr.field(mask, cells, conn8)
    if name == 'serpentine' and not conn8:
        assert rmoves[mask & (roff == 0)].max() == 21536              # the longest on-mask route
    off, moves, rounds = _field(mask, cells, conn8, rounds=True)
    print(f'{name} conn8={conn8}: {rounds} rounds')
    assert np.array_equal(off, roff) and np.array_equal(moves, rmoves)
    assert 0 < rounds < 21536 // 4, 'the rounds scale with the tiles a path crosses, not with its cells'


# ---------------------------------------------------------------------------------------------- 9: rendering
def _palette():
    return np.array([[int(round(c * 255)) for c in colorsys.hsv_to_rgb(k / 20, 1, 1)] for k in range(20)], np.int64)


def _blend(a, C, c):
    return (a * C + (256 - a) * c + 128) >> 8


def _squares(img, ys, xs, rgb):
    H, W = img.shape[:2]
    for y, x in zip(ys, xs):
        img[max(y - 2, 0):max(min(y + 3, H), 0), max(x - 2, 0):max(min(x + 3, W), 0)] = rgb


def _render_oracle(ad, t, sl, subset, trails):
    """DESIGN 6.8b's rules restated (tests/test_render.py) for the layers these tests draw, with the target layer
    between the grid and the trails: frame in red, tile grid, target paths (217), target cells (white), trails, dashed
    boxes; no annotation."""
    ds = ad.dataset
    H, W = ds.sizey, ds.sizex
    (ymin, ymax), (xmin, xmax) = ((0, n) if v is None else v for v, n in zip(sl[1:], (H, W)))
    pal = _palette()
    v = ds.frames[t + TC].cpu().numpy()
    img = np.zeros((H, W, 3), np.int64)
    img[..., 0] = np.rint(np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.int64)
    Y, X = np.mgrid[:H, :W]
    on = (X % ds.tilesize == 0) | (Y % ds.tilesize == 0)
    img[on] = _blend(38, 255, img[on])
    d = ad.get_frame_dets('IDed', t)
    rows = sorted((int(a.split('_')[-1]), int(x), int(y), a) for a, x, y in zip(d.index, d.anchor_x, d.anchor_y)
                  if subset is None or a in subset)
    paths = ad.get_trg_path(t)
    for n, x, y, a in rows:
        if a in paths:
            _squares(img, paths[a][0], paths[a][1], (217, 217, 217))
    tc = ad._target_cells
    _squares(img, tc // W, tc % W, (255, 255, 255))
    if trails:
        rec = ad.get_axon_reconstructions(t=t, include_history=True, axon_name=subset)
        segs = sorted({(int(f), int(a.split('_')[-1]), a) for a, _, f in rec.columns})
        canvas = np.zeros((H, W), np.int64)
        for k, (f, n, a) in enumerate(segs):
            xs, ys = rec[(a, 'X', f)].dropna().astype(int).to_numpy(), rec[(a, 'Y', f)].dropna().astype(int).to_numpy()
            for yy, xx in zip(ys, xs):
                canvas[max(yy - 2, 0):yy + 3, max(xx - 2, 0):xx + 3] = np.maximum(canvas[max(yy - 2, 0):yy + 3, max(xx - 2, 0):xx + 3], k + 1)
        cols = np.array([0] + [n % 20 for _, n, _ in segs])
        img[canvas > 0] = pal[cols[canvas[canvas > 0]]]
    u, w = np.meshgrid(np.arange(BOX), np.arange(BOX))
    border = ((u == 0) | (w == 0) | (u == BOX - 1) | (w == BOX - 1)) & (((u + w) // 4) % 2 == 0)
    for n, x, y, _ in rows:
        yy, xx = w[border] + y - BOX // 2, u[border] + x - BOX // 2
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        img[yy[ok], xx[ok]] = pal[n % 20]
    return img[ymin:ymax, xmin:xmax].astype(np.uint8)


def test_render_target_layer_bytes():
    H, W = 200, 260
    mask = synth.corridor_mask(H, W, width=16, pitch=50)
    d = synth.synth_detections(8, H, W, n_alive=7, seed=4, min_dist=20)
    ad = _ad(d, H, W, mask, frames=synth.synth_frames(8 + 2 * TC, H, W, seed=2))
    base = dict(annotate=False, draw_grid=True)
    with pytest.raises(ValueError, match='no target'):
        ad.render_frames(draw_target_paths=True, **base)
    region = np.zeros((H, W), bool)
    region[100:103, 248:260] = True                                   # at the frame's edge: the squares are clipped
    ad.set_target(region)
    with pytest.raises(ValueError, match='IDed'):
        ad.render_frames(which_dets='all', draw_target_paths=True, **base)
    off = ad.render_frames(**base).cpu().numpy()
    assert np.array_equal(off, ad.render_frames(draw_target_paths=False, **base).cpu().numpy())
    names = list(ad.IDed_dets_all.index[::2])
    crop = ((2, 7), (33, 171), (41, 260))
    for sl, subset, trails in (((None, None, None), None, False), ((None, None, None), None, True), (crop, None, True),
                               ((None, None, None), names, True), (crop, names, False)):
        got = ad.render_frames(t_y_x_slice=sl, axon_subset=subset, draw_axon_reconstructions=trails, draw_target_paths=True,
                               **base).cpu().numpy()
        t0 = 0 if sl[0] is None else sl[0][0]
        for k in range(len(got)):
            exp = _render_oracle(ad, t0 + k, sl, subset, trails)
            bad = np.argwhere((got[k] != exp).any(-1))
            assert got[k].shape == exp.shape and len(bad) == 0, (
                f'frame {t0 + k} slice {sl} subset {subset is not None}: {len(bad)} pixels differ, first at {bad[:3].tolist()}')
    on = ad.render_frames(draw_target_paths=True, **base).cpu().numpy()
    assert (on == 217).all(-1).any() and not np.array_equal(on, off)
    # with the keyword off the bytes are those of the oracle without the layer: the other tests of tests/test_render.py


def test_render_inference_draws_the_target_layer(tmp_path):
    import axtrack_amd
    H, W = 128, 160
    d = synth.synth_detections(4, H, W, n_alive=4, seed=8, min_dist=20)
    ad = _ad(d, H, W, frames=synth.synth_frames(4 + 2 * TC, H, W, seed=2))
    ad.set_target((64, 80))
    a = axtrack_amd.render_inference(ad, dest_dir=str(tmp_path / 'a'), draw_target_paths=True, annotate=False)
    b = axtrack_amd.render_inference(ad, dest_dir=str(tmp_path / 'b'), annotate=False)
    assert len(a) == len(b) == 4
    assert open(a[0], 'rb').read() != open(b[0], 'rb').read()
    with pytest.raises(ValueError, match='draw_trg_paths'):
        axtrack_amd.render_inference(ad, dest_dir=str(tmp_path / 'c'), draw_trg_paths=[1])
