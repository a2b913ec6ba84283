"""Target screens without a GPU: the SciPy reference against the CPU oracle, the numpy table builders, set_target's
validation, the C entry points' argument checks and the rectangle-run compression of the target layer."""
import ctypes

import numpy as np
import pytest

import target_reference as tr
from oracle import oracle as orc


# ------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize('conn8', [False, True])
def test_reference_agrees_with_the_oracle_path_matrix_for_a_single_cell_target(conn8):
    masks = [tr.blob_mask(60, 70, seed=3, n_blobs=6, n_holes=4), tr.serpentine_mask(48, 40, 4, 8),
             np.ones((20, 33), bool)]
    for mask in masks:
        H, W = mask.shape
        for ty, tx in ((H // 3, W // 2), (0, W - 1)):
            off, moves = tr.field(mask, [ty * W + tx], conn8)
            ys, xs = np.mgrid[:H, :W]
            sx, sy = xs.ravel()[::5], ys.ravel()[::5]
            D = orc.path_matrix((None, sx, sy), (None, np.array([tx]), np.array([ty])), H, W, mask=mask, max_dist=500,
                                conn8=conn8)
            assert (D[:, 0] == moves[sy, sx] + 1).all()
            assert off[ty, tx] == 0 and moves[ty, tx] == 0
            # the walk: moves + 1 cells, ends in the target, its recomputed key is the field's
            p = tr.walk(mask, off, moves, H - 1, 0, conn8)
            assert p[0] == (H - 1) * W and p[-1] == ty * W + tx and len(p) == moves[H - 1, 0] + 1
            assert tr.path_key(mask, p) == (off[H - 1, 0], moves[H - 1, 0])


def test_reference_counts_off_mask_cells_entered_target_included():
    mask = np.zeros((3, 6), bool)
    mask[1, :4] = True                                  # a corridor; the target lies two cells beyond its end
    off, moves = tr.field(mask, [1 * 6 + 5])
    assert (off[1, 0], moves[1, 0]) == (2, 5)           # enters (1,4) and the target (1,5), both off the mask
    assert (off[1, 4], moves[1, 4]) == (1, 1)
    assert (off[0, 0], moves[0, 0]) == (2, 6)           # down onto the corridor first: the same two off-mask cells


# ------------------------------------------------------------------------------------ table builders
def _hand():
    """Axon 3 in frames 0, 1, 3 (a gap at frame 2), axon 7 in frames 1, 2, 3 with its frame-2 detection outside the grid."""
    frame = np.array([0, 1, 1, 2, 3, 3])
    ids = np.array([3, 3, 7, 7, 3, 7])
    conf = np.array([.9, .8, .7, .6, .95, .65], np.float32)
    x, y = np.array([2, 4, 9, -3, 5, 9]), np.array([1, 1, 8, 8, 4, 2])
    off = np.array([0, 0, 2, -1, 0, 1])
    moves = np.array([50, 40, 90, -1, 30, 95])
    return frame, ids, conf, x, y, off, moves


def test_target_table_on_hand_made_arrays():
    from axtrack_amd.detections import _target_table
    frame, ids, conf, x, y, off, moves = _hand()
    g = _target_table(frame, ids, conf, x, y, off, moves, 35, 0.5, 5.0)
    assert g.index.names == ['axonID', 'frameID']
    a = g.loc['Axon_003']
    assert list(a.index) == [0, 1, 3]
    assert list(a.target_dist_px) == [50, 40, 30] and list(a.target_off_mask) == [0, 0, 0]
    assert np.isnan(a.approach_px[0]) and list(a.approach_px[[1, 3]]) == [10, 10]
    assert list(a.reached) == [False, False, True] and list(a.on_mask_route) == [True, True, True]
    assert list(a.target_dist_um) == [25, 20, 15]
    # the step over the gap spans two frames
    assert a.approach_um_per_min[1] == pytest.approx(10 * 0.5 / 5.0) and a.approach_um_per_min[3] == pytest.approx(10 * 0.5 / 10.0)
    assert (a.anchor_x[3], a.anchor_y[3]) == (5, 4) and a.conf[3] == pytest.approx(.95)
    b = g.loc['Axon_007']
    assert np.isnan(b.target_dist_px[2]) and np.isnan(b.target_off_mask[2]) and np.isnan(b.approach_px[2])
    assert not b.reached[2] and not b.on_mask_route[2] and not b.on_mask_route[1]
    assert b.approach_px[3] == -5                       # against the previous KNOWN distance (frame 1), over two frames
    assert b.approach_um_per_min[3] == pytest.approx(-5 * 0.5 / 10.0)
    # the unit columns need pixelsize (and dt)
    g = _target_table(frame, ids, conf, x, y, off, moves, 35, 0.5, None)
    assert 'target_dist_um' in g.columns and 'approach_um_per_min' not in g.columns
    g = _target_table(frame, ids, conf, x, y, off, moves, 35, None, 5.0)
    assert 'target_dist_um' not in g.columns and 'approach_um_per_min' not in g.columns
    assert len(_target_table(*(v[:0] for v in _hand()), 35, None, None)) == 0


def test_target_summary_on_hand_made_arrays():
    from axtrack_amd.detections import _target_summary
    frame, ids, _, _, _, _, moves = _hand()
    s = _target_summary(frame, ids, moves, 35)
    assert list(s.index) == ['Axon_003', 'Axon_007'] and s.index.name == 'axonID'
    assert list(s.columns) == ['first_frame', 'last_frame', 'n_frames', 'dist_first', 'dist_last', 'dist_min', 'frame_of_min',
                               'net_approach_px', 'reached_frame']
    a, b = s.loc['Axon_003'], s.loc['Axon_007']
    assert (a.first_frame, a.last_frame, a.n_frames, a.dist_first, a.dist_last, a.dist_min, a.frame_of_min, a.net_approach_px,
            a.reached_frame) == (0, 3, 3, 50, 30, 30, 3, 20, 3)
    assert (b.first_frame, b.last_frame, b.n_frames, b.dist_first, b.dist_last, b.dist_min, b.frame_of_min,
            b.net_approach_px) == (1, 3, 3, 90, 95, 90, 1, -5)
    assert np.isnan(b.reached_frame)


def test_trg_path_dict_crops_and_shifts():
    from axtrack_amd.detections import _trg_path_dict
    W = 12
    cells = np.array([2 * W + 1, 2 * W + 2, 3 * W + 2, 4 * W + 2, 5 * W + 5], np.int64)       # path of slot 0: 4 cells; slot 2: 1
    ptr = np.array([0, 4, 4, 5], np.int64)
    d = _trg_path_dict(np.array([7, 9, 11]), np.array([0, 1, 2]), ptr, cells, (10, W), None, 0, 0, 0, 0)
    assert sorted(d) == ['Axon_007', 'Axon_011']                      # slot 1 (outside the grid) has no path
    assert list(d['Axon_007'][0]) == [2, 2, 3, 4] and list(d['Axon_007'][1]) == [1, 2, 2, 2]
    d = _trg_path_dict(np.array([7, 9, 11]), np.array([0, 1, 2]), ptr, cells, (10, W), ['Axon_007'], 3, 0, 2, 0)
    assert list(d) == ['Axon_007'] and list(d['Axon_007'][0]) == [0, 1] and list(d['Axon_007'][1]) == [0, 0]
    canvas = np.zeros((10, W))
    canvas[_trg_path_dict(np.array([7]), np.array([0]), ptr, cells, (10, W), None, 0, 0, 0, 0)['Axon_007']] = 1   # video_plotting.py:309
    assert canvas.sum() == 4


# ------------------------------------------------------------------------------------ set_target
class _DS:
    name, sizet, sizey, sizex, device, mask2d, mask3d = 'x', 4, 20, 30, 'cpu', None, None


def _ad():
    from axtrack_amd import params
    from axtrack_amd.detections import AxonDetections
    return AxonDetections(None, _DS(), params.load_parameters(), None)


def test_set_target_validation_and_centre():
    ad = _ad()
    with pytest.raises(ValueError, match='no target'):
        ad.target_field()
    with pytest.raises(ValueError, match='no target'):
        ad.get_target_distances()
    ad.set_target((3, 4))
    assert ad.structure_outputchannel_coo == (3, 4) and ad.reach_px == ad.axon_box_size // 2
    assert list(ad._target_cells) == [3 * 30 + 4]
    with pytest.raises(ValueError, match='no identities'):
        ad.get_target_distances()
    with pytest.raises(ValueError, match='no identities'):
        ad.get_trg_path(0)
    for bad in ((20, 4), (3, 30), (-1, 0), np.zeros((20, 30), bool), np.zeros((0, 2), np.int64), np.zeros((5, 5), bool),
                (1, 2, 3), [[1.5, 2.0]]):
        with pytest.raises(ValueError):
            ad.set_target(bad)
    with pytest.raises(ValueError):
        ad.set_target((3, 4), reach_px=-1)
    assert ad.structure_outputchannel_coo == (3, 4)                   # a refused target changes nothing
    # a region: its cell nearest the centroid, ties to the first in row-major order
    m = np.zeros((20, 30), bool)
    m[4:6, 10:12] = True                                              # centroid (4.5, 10.5): four cells tie
    ad.set_target(m, reach_px=7)
    assert ad.structure_outputchannel_coo == (4, 10) and ad.reach_px == 7 and len(ad._target_cells) == 4
    ad.set_target(np.array([[2, 2], [2, 3], [2, 4], [9, 3], [2, 2]]))
    assert ad.structure_outputchannel_coo == (2, 3) and len(ad._target_cells) == 4      # centroid (3.75, 3)
    ad._shard = (0, 2)
    for call in (ad.target_field, ad.target_arrays, ad.get_target_distances, ad.get_target_summary, lambda: ad.get_trg_path(0)):
        with pytest.raises(NotImplementedError):
            call()


# ------------------------------------------------------------------------------------ C ABI
def test_entry_points_are_exported_and_check_arguments_without_a_gpu():
    from axtrack_amd import _lib
    lib = _lib.load()
    assert lib.axt_abi_version() == 1
    assert lib.axt_target_tile_size() >= 8
    EINVAL = -22
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data                                               # (never dereferenced: the checks come first)
    rounds = ctypes.c_int(0)
    n = ctypes.c_int64(0)
    f = lib.axt_target_field
    assert f(None, 8, 8, 0, None, 1, p, p, ctypes.byref(rounds), None) == EINVAL          # null targets
    assert b'axt_target_field' in lib.axt_last_error()
    assert f(None, 8, 8, 0, p, 0, p, p, ctypes.byref(rounds), None) == EINVAL             # empty target
    assert f(None, 0, 8, 0, p, 1, p, p, ctypes.byref(rounds), None) == EINVAL
    assert f(None, 8, -1, 0, p, 1, p, p, None, None) == EINVAL
    assert f(None, 65536, 65536, 0, p, 1, p, p, None, None) == EINVAL                     # cells must fit i32
    assert f(None, 8, 8, 0, p, 1, None, p, None, None) == EINVAL
    assert f(None, 8, 8, 0, p, 1, p, None, None, None) == EINVAL
    s = lib.axt_target_sample
    assert s(None, p, 1, None, 8, 8, p, p, p, 2, 4, p, p, None) == EINVAL
    assert s(p, p, 0, None, 8, 8, p, p, p, 2, 4, p, p, None) == EINVAL
    assert s(p, p, 2, None, 8, 8, p, p, p, 2, 4, p, p, None) == EINVAL                    # two fields, no index
    assert s(p, p, 1, None, 8, 8, p, p, p, 2, 0, p, p, None) == EINVAL
    assert s(p, p, 1, None, 8, 8, p, p, p, 2, 4, p, None, None) == EINVAL
    assert s(p, p, 1, None, 8, 8, p, p, p, 0, 4, p, p, None) == 0                         # no frames: nothing to do
    t = lib.axt_target_paths
    assert t(None, p, p, 8, 8, 0, p, p, 2, 4, p, None, 0, None, None, ctypes.byref(n), None) == EINVAL    # no cell_ptr
    assert t(None, p, p, 8, 8, 0, p, p, 2, 4, None, None, 0, p, None, ctypes.byref(n), None) == EINVAL    # no det_moves
    assert t(None, p, p, 8, 8, 0, p, p, 2, 0, p, None, 0, p, None, ctypes.byref(n), None) == EINVAL
    assert t(None, p, p, 0, 8, 0, p, p, 2, 4, p, None, 0, p, None, ctypes.byref(n), None) == EINVAL
    n.value = 5
    assert t(None, None, p, 8, 8, 0, p, p, 2, 4, p, None, 0, p, p, ctypes.byref(n), None) == EINVAL       # phase 2, no field
    n.value = -1
    assert t(None, p, p, 8, 8, 0, p, p, 2, 4, p, None, 0, p, p, ctypes.byref(n), None) == EINVAL
    n.value = 0
    assert t(None, p, p, 8, 8, 0, p, p, 2, 4, p, None, 0, p, p, ctypes.byref(n), None) == 0               # no cells: nothing to do


# ------------------------------------------------------------------------------------ rendering
def _pixels(rects):
    out = set()
    for x0, y0, w, h in rects:
        out |= {(y, x) for y in range(y0, y0 + h) for x in range(x0, x0 + w)}
    return out


def test_rectangle_runs_cover_exactly_the_per_cell_squares():
    from axtrack_amd.render import _run_rects
    # a hand-made path: 4 cells right, 2 down, a diagonal, one more diagonal; a second path of one cell
    ys = [3, 3, 3, 3, 4, 5, 6, 7, 20]
    xs = [4, 5, 6, 7, 7, 7, 8, 9, 20]
    pid = [0] * 8 + [1]
    k, x0, y0, w, h = _run_rects(ys, xs, pid)
    assert sorted(zip(k, x0, y0, w, h)) == [(0, 2, 1, 8, 5), (3, 5, 1, 5, 7), (6, 6, 4, 5, 5), (7, 7, 5, 5, 5), (8, 18, 18, 5, 5)]
    rng = np.random.default_rng(5)
    for _ in range(30):
        ys, xs, pid, q = [], [], [], 0
        for p in range(4):
            y = x = 12
            for _ in range(int(rng.integers(1, 40))):
                ys.append(y); xs.append(x); pid.append(p)
                q = int(rng.integers(0, 8)) if rng.random() < 0.3 else q          # (mostly straight on: long runs)
                y += tr.DY8[q]; x += tr.DX8[q]
        k, x0, y0, w, h = _run_rects(ys, xs, pid)
        assert _pixels(zip(x0, y0, w, h)) == _pixels((x - 2, y - 2, 5, 5) for y, x in zip(ys, xs))
        assert ((w == 5) | (h == 5)).all() and len(k) <= len(ys)
    # a straight run of k cells is ONE rectangle
    k, x0, y0, w, h = _run_rects([7] * 100, list(range(100)), [0] * 100)
    assert list(zip(x0, y0, w, h)) == [(-2, 5, 104, 5)]
    assert all(len(a) == 0 for a in _run_rects([], [], []))


def test_render_keywords():
    import axtrack_amd
    from axtrack_amd import render
    # the reference's draw_trg_paths stays refused; the new keyword is known to render_inference
    with pytest.raises(ValueError, match='draw_trg_paths'):
        axtrack_amd.render_inference(None, draw_trg_paths=[1])
    with pytest.raises(ValueError, match='dest_dir'):
        render.render_inference(_ad(), draw_target_paths=True)
