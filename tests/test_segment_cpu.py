"""Mask preparation without a GPU: the reference (tests/segment_reference.py) is consistent with itself and with numpy,
the host arithmetic of axtrack_amd/segment.py equals it, every bound on the arguments is enforced before any GPU work, in
Python and in the library, and the pinned recipe the GPU test reuses recovers the planted mask."""
import ctypes
import os
import re

import numpy as np
import pytest

import segment_reference as sr
from axtrack_amd import _lib, synth
from axtrack_amd import segment as seg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('axt_segment_edges', 'axt_segment_histogram', 'axt_segment_close', 'axt_segment_flood', 'axt_segment_tile_size')
AXT_EINVAL = -22


# ------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize('k', [2, 3, 4, 5])
def test_window_form_of_the_closing_equals_scipy(k):
    rng = np.random.default_rng(k)
    for B in (rng.random((37, 70)) < 0.5, rng.random((20, 9)) < 0.15, np.zeros((9, 11), bool), np.ones((9, 11), bool)):
        assert np.array_equal(sr.closing(B, k), sr.closing_windows(B, k))
    # the windows in one dimension: a single pixel dilates to [y - a, y + b] ...
    a, b = k // 2, k - 1 - k // 2
    one = np.zeros((1, 41), bool)
    one[0, 20] = True
    from scipy import ndimage as ndi
    d = ndi.binary_dilation(one, np.ones((1, k), bool))
    assert np.flatnonzero(d[0]).tolist() == list(range(20 - a, 20 + b + 1))     # out[x] = OR in[x - b .. x + a]
    hole = ~one
    e = ndi.binary_erosion(hole, np.ones((1, k), bool), border_value=1)
    assert np.flatnonzero(~e[0]).tolist() == list(range(20 - b, 20 + a + 1))    # out[x] = AND in[x - a .. x + b]


def test_histogram_rule_equals_numpy():
    rng = np.random.default_rng(1)
    G = rng.gamma(2.0, 300.0, (64, 97)).astype(np.float32)
    mn, mx = float(G.min()), float(G.max())
    assert np.array_equal(sr.histogram(G, mn, mx), np.histogram(G.astype(np.float64), 256, range=(mn, mx))[0])
    e = sr.bin_edges(mn, mx)
    assert np.array_equal(e, np.linspace(mn, mx, 257))
    on_edges = np.concatenate([e, np.nextafter(e, -np.inf)[1:], np.nextafter(e, np.inf)[:-1]])
    h = sr.histogram(on_edges, mn, mx)
    assert np.array_equal(h, np.histogram(on_edges, 256, range=(mn, mx))[0]) and h.sum() == on_edges.size
    flat = sr.histogram(np.full((5, 7), 3.25, np.float32), 3.25, 3.25)
    assert flat[0] == 35 and flat.sum() == 35


# ------------------------------------------------------------------------------------------ host arithmetic
@pytest.mark.parametrize('shape', sr.PINNED_SHAPES)
def test_otsu_threshold_from_hist_equals_the_reference(shape):
    _, _, stages, _, _ = sr.pinned(shape)
    G = stages['smoothed']
    mn, mx = float(G.min()), float(G.max())
    thr = seg.otsu_threshold_from_hist(stages['hist'], mn, mx)
    assert thr == stages['threshold'] == sr.otsu(stages['hist'], mn, mx)
    assert mn < thr < mx


def test_otsu_threshold_of_degenerate_histograms():
    h = np.zeros(256, np.int64)
    h[0] = 1234                                          # what stage 3 makes of a flat image
    assert seg.otsu_threshold_from_hist(h, 7.5, 7.5) == 7.5 == sr.otsu(h, 7.5, 7.5)
    for i in (0, 17, 255):                               # one non-empty bin on a proper range: no split has two classes
        h = np.zeros(256, np.int64)
        h[i] = 99
        assert seg.otsu_threshold_from_hist(h, 1.0, 3.0) == sr.otsu(h, 1.0, 3.0) == sr.bin_edges(1.0, 3.0)[:2].mean()
    with pytest.raises(ValueError):
        seg.otsu_threshold_from_hist(np.zeros(256), 0.0, 1.0)
    with pytest.raises(ValueError):
        seg.otsu_threshold_from_hist(np.ones(255), 0.0, 1.0)


# ------------------------------------------------------------------------------------------ validation
def _img(H=40, W=50):
    return np.zeros((H, W), np.uint16)


@pytest.mark.parametrize('kwargs', [
    dict(gaussion_sigma=0), dict(gaussion_sigma=-1.0), dict(gaussion_sigma=float('nan')), dict(gaussion_sigma=float('inf')),
    dict(gaussion_sigma=4.2),                            # radius 17
    dict(gaussion_sigma=2.5),                            # radius 10: 40 x 50 >= 22, but ...
    dict(bin_closing_dim=1), dict(bin_closing_dim=33), dict(bin_closing_dim=2.5), dict(bin_closing_dim=True)])
def test_segment_microchannels_rejects_bad_arguments(kwargs):
    img = _img(21, 50) if kwargs.get('gaussion_sigma') == 2.5 else _img()
    with pytest.raises(ValueError):
        seg.segment_microchannels(img, **kwargs)
    with pytest.raises(ValueError):
        seg.segment_mask(img, (3, 3), **kwargs)


def test_segment_microchannels_rejects_bad_images():
    for bad in (np.zeros((40, 50), np.float32), np.zeros((40, 50), np.int16), np.zeros(40, np.uint16),
                np.zeros((2, 3, 40, 50), np.uint16), _img(9, 50), _img(50, 9)):       # sigma 1: 2 radius + 2 = 10
        with pytest.raises(ValueError):
            seg.segment_microchannels(bad)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint16), (65536, 32768), (0, 0))      # 2^31 pixels, no memory
    with pytest.raises(ValueError):
        seg.segment_microchannels(big)
    # the smallest image and the largest radius pass the checks (and then need the GPU, which is another error)
    a, sigma, k = seg._check_image(_img(34, 34), 4.1, 32)
    assert a.shape == (34, 34) and int(4 * sigma + 0.5) == 16 and k == 32
    a, _, _ = seg._check_image(np.zeros((3, 10, 12), np.uint16), 1, 2)
    assert a.shape == (10, 12)


@pytest.mark.parametrize('point', [(-1, 0), (0, -1), (40, 0), (0, 50), (1, 2, 3), 'ab', None])
def test_flood_rejects_a_seed_outside_the_grid(point):
    with pytest.raises(ValueError):
        seg.flood_initial_mask(np.zeros((40, 50), bool), point)
    with pytest.raises(ValueError):
        seg.segment_mask(_img(), point)


def test_flood_rejects_bad_connectivity_and_shapes():
    for c in (0, 3, 8, None):
        with pytest.raises(ValueError):
            seg.flood_initial_mask(np.zeros((40, 50), bool), (1, 1), connectivity=c)
    with pytest.raises(ValueError):
        seg.flood_initial_mask(np.zeros((4, 40, 50), bool), (1, 1))
    with pytest.raises(ValueError):
        seg.save_final_mask(np.zeros((4, 40, 50), bool), 'never_written.npy')
    assert not os.path.exists('never_written.npy')


def test_library_returns_the_invalid_argument_status():
    """Every bound, at the C ABI: the arguments are checked before any pointer is read and before any HIP call."""
    lib = _lib.load()
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    rounds = ctypes.c_int(0)
    edges = lambda H, W, sigma, img=p: lib.axt_segment_edges(img, H, W, sigma, p, p, p, None)
    for H, W, sigma in ((0, 50, 1.0), (50, -1, 1.0), (65536, 32768, 1.0), (50, 50, 0.0), (50, 50, -1.0), (50, 50, float('nan')),
                        (50, 50, 4.2), (50, 50, 1e300), (9, 50, 1.0), (50, 9, 1.0), (33, 40, 4.1)):
        assert edges(H, W, sigma) == AXT_EINVAL, (H, W, sigma)
        assert lib.axt_last_error()
    assert edges(50, 50, 1.0, None) == AXT_EINVAL
    for n, mn, mx in ((0, 0.0, 1.0), (2 ** 31, 0.0, 1.0), (10, 2.0, 1.0), (10, float('nan'), 1.0), (10, 0.0, float('inf'))):
        assert lib.axt_segment_histogram(p, n, mn, mx, p, None) == AXT_EINVAL, (n, mn, mx)
    assert lib.axt_segment_histogram(None, 10, 0.0, 1.0, p, None) == AXT_EINVAL
    for H, W, thr, k in ((0, 5, 1.0, 4), (5, 0, 1.0, 4), (65536, 32768, 1.0, 4), (5, 5, 1.0, 1), (5, 5, 1.0, 33),
                         (5, 5, float('nan'), 4)):
        assert lib.axt_segment_close(p, H, W, thr, k, p, None) == AXT_EINVAL, (H, W, thr, k)
    assert lib.axt_segment_close(p, 5, 5, 1.0, 4, None, None) == AXT_EINVAL
    for H, W, y, x in ((0, 5, 0, 0), (5, 0, 0, 0), (65536, 32768, 0, 0), (5, 6, -1, 0), (5, 6, 0, -1), (5, 6, 5, 0), (5, 6, 0, 6)):
        assert lib.axt_segment_flood(p, H, W, y, x, 1, p, ctypes.byref(rounds), None) == AXT_EINVAL, (H, W, y, x)
    assert lib.axt_segment_flood(None, 5, 6, 0, 0, 1, p, None, None) == AXT_EINVAL
    assert not buf.any()


# ------------------------------------------------------------------------------------------ declarations
def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'axtrack_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = _lib.load()
    for n in SYMBOLS:
        assert re.search(r'\bint\s+' + n + r'\s*\(', code), f'{n} is not declared in include/axtrack_hip.h'
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert '00_segment_bg.ipynb' in text
    assert lib.axt_segment_tile_size() == 64 and lib.axt_abi_version() == 1
    import axtrack_amd
    from axtrack_amd import hotpath as hp
    for n in ('segment_microchannels', 'flood_initial_mask', 'segment_mask', 'save_final_mask', 'otsu_threshold_from_hist'):
        assert n in axtrack_amd.__all__ and getattr(axtrack_amd, n) is getattr(seg, n)
    for n in ('segment_edges', 'segment_histogram', 'segment_close', 'segment_flood'):
        assert callable(getattr(hp, n))
    assert 'segment.hip' in open(os.path.join(ROOT, 'axtrack_amd', 'csrc', 'Makefile')).read()


# ------------------------------------------------------------------------------------------ the pinned recipe
def test_transmission_image_is_what_it_says():
    from scipy.ndimage import gaussian_filter
    mask = synth.corridor_mask(96, 130)
    img = synth.transmission_image(mask, seed=0)
    want = gaussian_filter(20000.0 + 8000.0 * mask, 1.5) + np.random.default_rng(0).normal(0.0, 300.0, mask.shape)
    assert img.dtype == np.uint16 and np.array_equal(img, np.clip(np.rint(want), 0, 65535).astype(np.uint16))
    assert not np.array_equal(img, synth.transmission_image(mask, seed=1))


@pytest.mark.parametrize('shape,measured', list(zip(sr.PINNED_SHAPES, (0.927, 0.939, 0.946))))
def test_reference_pipeline_recovers_the_planted_mask(shape, measured):
    """corridor_mask, image seed 0, sigma 1, k 4, the flood point of seed_of: the f64 reference reaches IoU 0.927, 0.939
    and 0.946 against the planted mask at 512 x 512, 200 x 312 and 96 x 130. It has to stay >= 0.9: the condition the GPU
    test asks of the package."""
    planted, img, stages, seed, final = sr.pinned(shape)
    assert planted[seed] and not stages['initial_mask'][seed], 'the flood point lies in a channel, off the closed edges'
    got = sr.iou(final, planted)
    assert got >= 0.9 and abs(got - measured) < 1e-3, got
