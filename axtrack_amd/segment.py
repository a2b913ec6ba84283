"""Mask preparation: the microchannel mask from a transmission image, on the GPU.

Stands in for the reference's data_prep_nbs/00_segment_bg.ipynb (napari + scikit-image): segment_microchannels,
flood_initial_mask and save_final_mask keep the notebook's names and argument names (`gaussion_sigma` included). Between
the two steps the initial mask is a plain numpy array, so it can be touched up by hand as in the notebook. The stages are
defined in DESIGN.md 6.8d; the kernels are csrc/segment.hip. There is no CPU path: arguments are checked first, then
everything but the 256-number Otsu arithmetic runs on the device."""
import numpy as np

MAX_RADIUS = 16            # of the Gaussian: int(4 sigma + 0.5)
NBINS = 256                # threshold_otsu's default


def _check_image(transm_chnl, gaussion_sigma, bin_closing_dim):
    a = np.asarray(transm_chnl)
    if a.ndim == 3:
        a = a[0]                                        # the notebook segments t = 0
    if a.ndim != 2 or a.dtype != np.uint16:
        raise ValueError(f'the transmission image must be uint16 [H, W] or [T, H, W], not {a.dtype} {list(a.shape)}')
    try:
        sigma = float(gaussion_sigma)
    except (TypeError, ValueError):
        raise ValueError(f'gaussion_sigma must be a number, not {gaussion_sigma!r}') from None
    if not sigma > 0 or not np.isfinite(sigma):
        raise ValueError(f'gaussion_sigma must be > 0, not {gaussion_sigma!r}')
    radius = int(4.0 * sigma + 0.5)
    if radius > MAX_RADIUS:
        raise ValueError(f'gaussion_sigma {sigma} needs a radius of {radius} > {MAX_RADIUS}')
    H, W = a.shape
    if H * W > 2 ** 31 - 1:
        raise ValueError(f'a {H} x {W} image has more than 2^31 - 1 pixels')
    if min(H, W) < 2 * radius + 2:
        raise ValueError(f'a {H} x {W} image is smaller than 2 radius + 2 = {2 * radius + 2}')
    if isinstance(bin_closing_dim, bool) or int(bin_closing_dim) != bin_closing_dim or not 2 <= int(bin_closing_dim) <= 32:
        raise ValueError(f'bin_closing_dim must be an integer in [2, 32], not {bin_closing_dim!r}')
    return np.ascontiguousarray(a), sigma, int(bin_closing_dim)


def _check_seed(shape, floodpoint, connectivity):
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1 or shape[0] * shape[1] > 2 ** 31 - 1:
        raise ValueError(f'the mask must be [H, W] with at most 2^31 - 1 cells, not {list(shape)}')
    try:
        y, x = (int(v) for v in floodpoint)
    except (TypeError, ValueError):
        raise ValueError(f'floodpoint must be (y, x), not {floodpoint!r}') from None
    if not (0 <= y < shape[0] and 0 <= x < shape[1]):
        raise ValueError(f'floodpoint ({y}, {x}) is outside the {shape[0]} x {shape[1]} image')
    if connectivity not in (1, 2):
        raise ValueError(f'connectivity must be 1 (4 neighbours) or 2 (8 neighbours), not {connectivity!r}')
    return y, x


def otsu_threshold_from_hist(hist, mn, mx):
    """Otsu's threshold from the 256 counts of np.histogram(image, 256, range=(mn, mx)), in f64 as threshold_otsu
    computes it: the centre of the bin that maximises the between-class variance, the first such bin. A flat image
    (mn == mx) gives mn."""
    h = np.asarray(hist, np.float64)
    if h.shape != (NBINS,) or (h < 0).any() or not h.sum() > 0:
        raise ValueError('hist must be 256 non-negative counts, not all zero')
    mn, mx = float(mn), float(mx)
    if not mn <= mx:
        raise ValueError(f'bad range [{mn}, {mx}]')
    if mn == mx:
        return mn
    edges = np.arange(NBINS + 1) * ((mx - mn) / NBINS) + mn
    edges[-1] = mx
    c = (edges[:-1] + edges[1:]) / 2
    w1 = np.cumsum(h)
    w2 = np.cumsum(h[::-1])[::-1]
    with np.errstate(divide='ignore', invalid='ignore'):
        m1 = np.cumsum(h * c) / w1
        m2 = (np.cumsum((h * c)[::-1]) / w2[::-1])[::-1]
        var = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    var = np.where(np.isnan(var), 0.0, var)            # (an empty class has weight 0: no variance between classes)
    return float(c[int(np.argmax(var))])


def _to_device_u16(a):
    import torch
    a = a if a.flags.writeable else a.copy()           # (torch refuses to wrap a read-only array quietly)
    return torch.from_numpy(a.view(np.int16)).cuda()


def segment_microchannels(transm_chnl, gaussion_sigma=1, bin_closing_dim=4, return_stages=False):
    """The notebook's segment_microchannels: Prewitt edges, Gaussian smoothing, Otsu's threshold of the smoothed edges
    applied to the unsmoothed ones, binary closing with a bin_closing_dim square. transm_chnl: uint16 [H, W] (a
    [T, H, W] array is cut to t = 0). Returns the initial mask, bool [H, W]; with return_stages a dict of numpy arrays:
    prewitt, smoothed (f32), hist (i64 [256]), threshold (float), binary, initial_mask (bool)."""
    from . import hotpath as hp
    a, sigma, k = _check_image(transm_chnl, gaussion_sigma, bin_closing_dim)
    hp._require_gpu()
    P, G, minmax = hp.segment_edges(_to_device_u16(a), sigma)
    mn, mx = (float(v) for v in minmax.cpu().numpy())
    hist = hp.segment_histogram(G, mn, mx).cpu().numpy()
    thr = otsu_threshold_from_hist(hist, mn, mx)
    initial = hp.segment_close(P, thr, k).cpu().numpy().astype(bool)
    if not return_stages:
        return initial
    prewitt = P.cpu().numpy()
    return {'prewitt': prewitt, 'smoothed': G.cpu().numpy(), 'hist': hist, 'threshold': thr,
            'binary': prewitt.astype(np.float64) > thr, 'initial_mask': initial}


def flood_initial_mask(initial_mask, floodpoint, connectivity=2):
    """The notebook's flood_initial_mask, skimage.segmentation.flood(initial_mask, floodpoint): the cells connected to
    floodpoint = (y, x) through cells of its value. connectivity 2: 8 neighbours, 1: 4 neighbours. Returns bool [H, W]."""
    import torch
    from . import hotpath as hp
    m = np.asarray(initial_mask)
    y, x = _check_seed(m.shape, floodpoint, connectivity)
    hp._require_gpu()
    img = torch.from_numpy(np.ascontiguousarray(m != 0).view(np.uint8)).cuda()
    return hp.segment_flood(img, y, x, conn8=connectivity == 2).cpu().numpy().astype(bool)


def segment_mask(transm_chnl, floodpoint, gaussion_sigma=1, bin_closing_dim=4, connectivity=2):
    """segment_microchannels and flood_initial_mask in one call: the final mask, bool [H, W]. transm_chnl may also be the
    name of a .npy or .tif / .tiff file (the latter through the package's own reader, tiff.py; page 0 is segmented)."""
    if isinstance(transm_chnl, str):
        from . import tiff
        transm_chnl = tiff.read_stack(transm_chnl) if tiff.is_tiff_name(transm_chnl) else np.load(transm_chnl)
    a, _, _ = _check_image(transm_chnl, gaussion_sigma, bin_closing_dim)
    _check_seed(a.shape, floodpoint, connectivity)
    return flood_initial_mask(segment_microchannels(a, gaussion_sigma, bin_closing_dim), floodpoint, connectivity)


def save_final_mask(mask, fname):
    """The notebook's save_final_mask: np.save of the bool mask, the file prepare_input_data(mask_fname=...) loads."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError(f'the mask must be [H, W], not {list(m.shape)}')
    np.save(fname, m.astype(bool))
    return fname
