"""Mask preparation on the GPU (axt_segment_edges / _histogram / _close / _flood and axtrack_amd/segment.py) against
tests/segment_reference.py: SciPy and numpy in f64. Integer results (histogram, closing, flood, min and max) are compared
for equality; the two float images have bounds derived from the arithmetic, stated where they are used. Every stage is
judged on the GPU's own output of the stage before it, so that no stage inherits another's rounding."""
import numpy as np
import pytest

import segment_reference as sr
import target_reference as tr
from axtrack_amd import synth, params

pytestmark = pytest.mark.gpu
U = 2.0 ** -24                                 # unit roundoff of f32


def _u16(a):
    import torch
    return torch.from_numpy(np.array(a, np.uint16).view(np.int16)).cuda()


def _f32(a):
    import torch
    return torch.from_numpy(np.array(a, np.float32)).cuda()


def _edges(img, sigma):
    from axtrack_amd import hotpath as hp
    P, G, mm = hp.segment_edges(_u16(img), sigma)
    return P.cpu().numpy(), G.cpu().numpy(), mm.cpu().numpy()


def _edge_images(sigma):
    """The three pinned images (no size a multiple of the 32 x 64 tile) and one of exactly 2 radius + 2 rows, in full-range
    noise: 3 x 3 sums up to 3 * 65535, and a halo taller than the image."""
    imgs = {shape: sr.pinned(shape)[1] for shape in sr.PINNED_SHAPES}
    rows = 2 * sr.radius_of(sigma) + 2
    imgs[(rows, 70)] = np.random.default_rng(3).integers(0, 65536, (rows, 70)).astype(np.uint16)
    return imgs


# ------------------------------------------------------------------------------------------------ stages 1 + 2
@pytest.mark.parametrize('sigma', [1.0, 2.5])
def test_edges_and_smoothing_are_within_the_derived_bounds(sigma):
    r = sr.radius_of(sigma)
    assert r == {1.0: 4, 2.5: 10}[sigma]
    for shape, img in _edge_images(sigma).items():
        P, G, mm = _edges(img, sigma)
        assert P.shape == G.shape == shape and P.dtype == G.dtype == np.float32
        # P: the 3 x 3 sums are exact; a division by 3, two squares, an add, an exact halving and a square root remain:
        # (1 + 2 + 1) roundings under the root, halved by it, plus its own: below 8 U
        ref = sr.edge_magnitude(img)
        err = np.abs(P - ref)
        worst = float((err / np.maximum(ref, 1e-300)).max())
        print(f'sigma {sigma} {shape}: max relative error of P {worst / U:.2f} U')
        assert (err <= 8 * U * ref).all(), f'{shape}: P is off by {worst / U:.2f} U > 8 U'
        # G against f64 on the GPU's own P: per pass one rounding for each weight and product and one per addition of
        # non-negative terms, 2 radius + 2 at most; two passes, plus the roundings of the stored row sums and result
        ref = sr.smooth(P, sigma)
        bound = (2 * (2 * r + 2) + 2) * U
        err = np.abs(G - ref)
        worst = float((err / np.maximum(ref, 1e-300)).max())
        print(f'sigma {sigma} {shape}: max relative error of G {worst / U:.2f} U (bound {bound / U:.0f} U)')
        assert (err <= bound * ref).all(), f'{shape}: G is off by {worst / U:.2f} U > {bound / U:.0f} U'
        assert mm.dtype == np.float32 and mm[0] == G.min() and mm[1] == G.max()


def test_edges_of_a_flat_image_are_zero():
    P, G, mm = _edges(np.full((50, 70), 40000, np.uint16), 1.0)
    assert not P.any() and not G.any() and mm.tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ stage 3
def _hist(G, mn, mx):
    from axtrack_amd import hotpath as hp
    return hp.segment_histogram(_f32(G), mn, mx).cpu().numpy()


def _np_hist(G, mn, mx):
    return np.histogram(np.asarray(G, np.float32).astype(np.float64), 256, range=(float(mn), float(mx)))[0]


def test_histogram_equals_numpy():
    for shape in sr.PINNED_SHAPES:
        _, G, mm = _edges(sr.pinned(shape)[1], 1.0)
        h = _hist(G, mm[0], mm[1])
        assert h.dtype == np.int64 and h.sum() == G.size
        assert np.array_equal(h, _np_hist(G, mm[0], mm[1])) and np.array_equal(h, sr.histogram(G, mm[0], mm[1]))
        assert np.array_equal(h, _hist(G, mm[0], mm[1])), 'two runs differ'


@pytest.mark.parametrize('mn,mx', [(0.0, 256.0), (1.0, 3.0), (0.3721, 1977.337), (1e-3, 1.1e-3)])
def test_histogram_of_values_on_the_bin_edges(mn, mx):
    """Values on the edges, on mn and mx and one f32 step to either side of each: edges that f32 holds exactly (the
    first two ranges) and edges it does not."""
    mn, mx = float(np.float32(mn)), float(np.float32(mx))
    e = sr.bin_edges(mn, mx).astype(np.float32)
    v = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))])
    v = np.tile(v[(v >= mn) & (v <= mx)], 3)
    h = _hist(v, mn, mx)
    assert h.sum() == v.size and np.array_equal(h, _np_hist(v, mn, mx)) and np.array_equal(h, sr.histogram(v, mn, mx))
    assert h[0] >= 3 and h[255] >= 3


def test_histogram_of_a_flat_image_and_the_stages_after_it():
    from axtrack_amd import segment as seg
    h = _hist(np.full((37, 41), 2.5, np.float32), 2.5, 2.5)
    assert h[0] == 37 * 41 and h.sum() == 37 * 41
    st = seg.segment_microchannels(np.full((37, 41), 1234, np.uint16), return_stages=True)
    assert st['hist'][0] == 37 * 41 and st['threshold'] == 0.0 and not st['binary'].any() and not st['initial_mask'].any()
    assert st['initial_mask'].dtype == bool and st['prewitt'].dtype == np.float32 and st['hist'].dtype == np.int64


# ------------------------------------------------------------------------------------------------ stage 4
@pytest.mark.parametrize('k', [2, 3, 4, 7, 32])
def test_closing_equals_scipy(k):
    from axtrack_amd import hotpath as hp
    P, G, mm = _edges(sr.pinned((96, 130))[1], 1.0)
    thr = sr.otsu(sr.histogram(G, mm[0], mm[1]), mm[0], mm[1])
    rng = np.random.default_rng(k)
    cases = {'edges 96 x 130': (P, thr),
             'noise 70 x 130': (rng.random((70, 130), np.float32), 0.5),      # every window position matters
             'noise 50 x 37': (rng.random((50, 37), np.float32), 0.5),        # one word, not full
             'noise 33 x 64': (rng.random((33, 64), np.float32), 0.5),        # one word, full
             'sparse 40 x 200': (rng.random((40, 200), np.float32), 0.97),
             'all False': (rng.random((45, 130), np.float32), 2.0),           # the dilation's 0 outside
             'all True': (rng.random((45, 130), np.float32), -1.0)}           # the erosion's 1 outside
    for name, (img, t) in cases.items():
        got = hp.segment_close(_f32(img), t, k).cpu().numpy()
        B = img.astype(np.float64) > t
        ref = sr.closing(B, k)
        assert got.dtype == np.uint8 and got.max(initial=0) <= 1
        bad = np.argwhere(got.astype(bool) != ref)
        assert len(bad) == 0, f'k = {k}, {name}: {len(bad)} pixels differ, first {bad[0].tolist()}'
        assert {'all False': not ref.any(), 'all True': ref.all()}.get(name, True)


def test_threshold_is_compared_in_f64():
    """A threshold between two neighbouring f32 values separates them."""
    from axtrack_amd import hotpath as hp
    lo = np.float32(1000.0)
    hi = np.nextafter(lo, np.float32(np.inf))
    img = np.full((8, 70), lo, np.float32)
    img[2:6, 10:60] = hi
    thr = (float(lo) + float(hi)) / 2
    assert np.float32(thr) in (lo, hi)                     # in f32 the comparison would lose one side
    got = hp.segment_close(_f32(img), thr, 2).cpu().numpy().astype(bool)
    assert np.array_equal(got, sr.closing(img.astype(np.float64) > thr, 2)) and got.sum() == 4 * 50


# ------------------------------------------------------------------------------------------------ stage 5
def _flood(img, seed, connectivity, rounds=False):
    import torch
    from axtrack_amd import hotpath as hp
    out = hp.segment_flood(torch.from_numpy(np.array(img, bool).view(np.uint8)).cuda(), seed[0], seed[1],
                           conn8=connectivity == 2, return_rounds=True)
    got = out[0].cpu().numpy()
    assert got.dtype == np.uint8 and got.max() == 1
    return (got.astype(bool), out[1]) if rounds else got.astype(bool)


def _anti_diagonal():
    m = np.zeros((200, 200), bool)
    m[np.arange(192), 191 - np.arange(192)] = True         # (63, 128) -> (64, 127): through a tile corner
    return m


def _flood_cases():
    blobs = tr.blob_mask(200, 312, seed=7)
    ys, xs = np.nonzero(blobs)
    yo, xo = np.nonzero(~blobs)
    checker = (np.add.outer(np.arange(70), np.arange(130)) % 2) == 0
    single = np.zeros((130, 140), bool)
    single[70, 64] = True
    spiral = sr.spiral_mask(61)
    assert spiral.sum() > 1900 and sr.flood(spiral, (0, 0), 1).sum() == spiral.sum()
    cells = np.argwhere(spiral)
    inner = tuple(int(v) for v in cells[np.argmin(((cells - 30) ** 2).sum(1))])
    return [('serpentine, many tiles one after the other', tr.serpentine_mask(256, 256, 12, 24), (0, 0)),
            ('serpentine from its far end', tr.serpentine_mask(256, 256, 12, 24), (251, 3)),
            ('blobs', blobs, (int(ys[len(ys) // 2]), int(xs[len(xs) // 2]))),
            ('blobs, seed on a False cell', blobs, (int(yo[len(yo) // 3]), int(xo[len(yo) // 3]))),
            ('one-pixel checkerboard', checker, (0, 0)),
            ('checkerboard, seed on a False cell', checker, (69, 128)),
            ('spiral inside one tile', spiral, (0, 0)),
            ('spiral from its inner end', spiral, inner),
            ('diagonal through tile corners', sr.diagonal_mask(200), (0, 0)),
            ('diagonal from its other end', sr.diagonal_mask(200), (199, 199)),
            ('anti-diagonal through tile corners', _anti_diagonal(), (0, 191)),
            ('anti-diagonal from its other end', _anti_diagonal(), (191, 0)),
            ('isolated pixel', single, (70, 64)),
            ('around an isolated pixel', single, (0, 0)),
            ('uniform image', np.ones((96, 130), bool), (5, 5)),
            ('uniform False image', np.zeros((65, 64), bool), (64, 63))]


@pytest.mark.parametrize('connectivity', [1, 2])
def test_flood_equals_scipy_label(connectivity):
    for name, img, seed in _flood_cases():
        got = _flood(img, seed, connectivity)
        ref = sr.flood(img, seed, connectivity)
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, (f'{name}, connectivity {connectivity}: {len(bad)} cells differ, first {bad[0].tolist()} '
                               f'(got {got.sum()} cells, reference {ref.sum()})')
        assert got[seed]


def test_flood_connectivities_differ_where_they_should():
    checker = (np.add.outer(np.arange(70), np.arange(130)) % 2) == 0
    assert _flood(checker, (0, 0), 1).sum() == 1 and np.array_equal(_flood(checker, (0, 0), 2), checker)
    assert _flood(sr.diagonal_mask(200), (0, 0), 1).sum() == 1 and _flood(sr.diagonal_mask(200), (0, 0), 2).sum() == 200


def test_flood_of_a_large_serpentine_stays_below_the_round_bound():
    from axtrack_amd import hotpath as hp
    img = tr.serpentine_mask(1024, 1024, 12, 24)
    got, rounds = _flood(img, (0, 0), 2, rounds=True)
    assert np.array_equal(got, sr.flood(img, (0, 0), 2)) and np.array_equal(got, img)
    ts = hp.segment_tile_size()
    n_tiles = (1024 // ts) ** 2
    print(f'1024 x 1024 serpentine: {rounds} rounds with work, bound {n_tiles * 4 * ts}')
    assert ts == 64 and 1024 // 24 <= rounds < n_tiles * 4 * ts
    again, rounds2 = _flood(img, (0, 0), 2, rounds=True)
    assert again.tobytes() == got.tobytes() and rounds2 == rounds


def test_flood_is_byte_identical_from_run_to_run():
    blobs = tr.blob_mask(200, 312, seed=7)
    yo, xo = np.nonzero(~blobs)
    seed = (int(yo[len(yo) // 3]), int(xo[len(yo) // 3]))
    a = _flood(blobs, seed, 2)
    for _ in range(3):
        assert _flood(blobs, seed, 2).tobytes() == a.tobytes()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize('shape', sr.PINNED_SHAPES)
def test_segment_mask_recovers_the_planted_mask(shape):
    """The pinned recipe of test_segment_cpu.py. Otsu's two best bins differ by 1e-6 .. 2e-5 of the variance on these
    images, so the f32 pipeline may pick the bin next to the f64 reference's: equality is asserted per stage above, and
    here only what the mask is for."""
    from axtrack_amd import segment as seg
    planted, img, stages, seed, final = sr.pinned(shape)
    got = seg.segment_mask(img, seed)
    assert got.dtype == bool and got.shape == shape
    differ = float((got != final).mean())
    got_iou, ref_iou = sr.iou(got, planted), sr.iou(final, planted)
    print(f'{shape}: IoU {got_iou:.4f} (f64 reference {ref_iou:.4f}), {differ:.2e} of the pixels differ from the reference')
    assert got_iou >= 0.9, f'{shape}: IoU {got_iou:.4f} < 0.9; {differ:.2e} of the pixels differ from the f64 reference ({ref_iou:.4f})'
    # the two steps and the stages agree with the one call
    st = seg.segment_microchannels(img, return_stages=True)
    assert np.array_equal(seg.flood_initial_mask(st['initial_mask'], seed), got)
    assert np.array_equal(st['initial_mask'], seg.segment_microchannels(img[None]))      # [T, H, W] is cut to t = 0
    assert np.array_equal(st['initial_mask'], sr.closing(st['binary'], 4))
    assert st['threshold'] == sr.otsu(st['hist'], st['smoothed'].min(), st['smoothed'].max())


def test_saved_mask_feeds_prepare_input_data_and_the_target_screen(tmp_path):
    import axtrack_amd
    from axtrack_amd import segment as seg
    shape = (96, 130)
    planted, img, _, seed, _ = sr.pinned(shape)
    mask = seg.segment_mask(img, seed)
    assert seg.save_final_mask(mask, str(tmp_path / 'mask.npy')) == str(tmp_path / 'mask.npy')
    loaded = np.load(tmp_path / 'mask.npy')
    assert loaded.dtype == bool and np.array_equal(loaded, mask)
    P = params.load_parameters()
    P['ASTAR_8_CONNECTED'] = True                          # the flood's 8 neighbours
    raw = np.stack([img] * 5)
    tl = axtrack_amd.prepare_input_data(raw, P, str(tmp_path), str(tmp_path), params.DEPLOYED_STND_SCALER, 'mask.npy',
                                        use_cached_datasets=None, input_metadata={'name': 'segmented'})
    assert np.array_equal(tl.mask2d, mask)
    ad = axtrack_amd.AxonDetections(None, tl, P, None)
    cells = np.argwhere(mask)
    ad.set_target(tuple(int(v) for v in cells[len(cells) // 4]))
    off = ad.target_field()[0].cpu().numpy()
    assert (off[mask] == 0).all() and off[seed] == 0       # the flooded region is one component: no off-mask cell on the way
