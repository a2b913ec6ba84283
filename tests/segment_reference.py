"""Reference of the mask preparation (axtrack_amd/csrc/segment.hip, axtrack_amd/segment.py), independent of the package:
the definitions of DESIGN.md 6.8d restated with SciPy and numpy in f64. scikit-image, which the reference project's
notebook (data_prep_nbs/00_segment_bg.ipynb) calls, is not a dependency; SciPy is what it calls underneath."""
import functools

import numpy as np
from scipy import ndimage as ndi

NBINS = 256


# --------------------------------------------------------------------------------------------------- stages 1, 2
def edge_magnitude(img):
    """P = sqrt((gy^2 + gx^2) / 2), gy / gx = scipy's Prewitt along axis 0 / 1 divided by 3, reflect, in f64."""
    a = np.asarray(img).astype(np.float64)
    gy = ndi.prewitt(a, axis=0, mode='reflect') / 3.0
    gx = ndi.prewitt(a, axis=1, mode='reflect') / 3.0
    return np.sqrt((gy * gy + gx * gx) / 2.0)


def radius_of(sigma):
    return int(4.0 * float(sigma) + 0.5)


def smooth(P, sigma):
    return ndi.gaussian_filter(np.asarray(P, np.float64), float(sigma), mode='nearest', truncate=4.0)


# --------------------------------------------------------------------------------------------------- stage 3
def bin_edges(mn, mx):
    e = np.array([float(mn) + i * ((float(mx) - float(mn)) / NBINS) for i in range(NBINS + 1)], np.float64)
    e[NBINS] = float(mx)
    return e


def histogram(G, mn, mx):
    """The rule in words: v falls into the bin i with e_i <= v < e_i+1, the last bin closed on the right; a flat image
    (mn == mx) puts everything into bin 0. i64 [256]."""
    v = np.asarray(G).astype(np.float64).ravel()
    if float(mn) == float(mx):
        h = np.zeros(NBINS, np.int64)
        h[0] = int((v == float(mn)).sum())
        return h
    e = bin_edges(mn, mx)
    v = v[(v >= e[0]) & (v <= e[NBINS])]
    i = np.searchsorted(e, v, side='right') - 1           # the last edge that is <= v
    i[i == NBINS] = NBINS - 1                             # v == mx
    return np.bincount(i, minlength=NBINS).astype(np.int64)


def otsu(hist, mn, mx):
    """Otsu's threshold from the counts: the centre of the first bin i that maximises the between-class variance of
    the split bins [0, i] | [i + 1, 255]; a split with an empty class has variance 0. Plain loop, f64."""
    if float(mn) == float(mx):
        return float(mn)
    h = [float(x) for x in hist]
    e = bin_edges(mn, mx)
    c = [(e[i] + e[i + 1]) / 2 for i in range(NBINS)]
    best, arg = -1.0, 0
    for i in range(NBINS - 1):
        w1, w2 = sum(h[:i + 1]), sum(h[i + 1:])
        var = 0.0
        if w1 > 0 and w2 > 0:
            m1 = sum(h[j] * c[j] for j in range(i + 1)) / w1
            m2 = sum(h[j] * c[j] for j in range(i + 1, NBINS)) / w2
            var = w1 * w2 * (m1 - m2) ** 2
        if var > best:
            best, arg = var, i
    return float(c[arg])


def otsu_variances(hist, mn, mx):
    """The 255 between-class variances, vectorised (for reporting how close the two best bins are)."""
    h = np.asarray(hist, np.float64)
    e = bin_edges(mn, mx)
    c = (e[:-1] + e[1:]) / 2
    w1, w2 = np.cumsum(h), np.cumsum(h[::-1])[::-1]
    with np.errstate(divide='ignore', invalid='ignore'):
        m1 = np.cumsum(h * c) / w1
        m2 = (np.cumsum((h * c)[::-1]) / w2[::-1])[::-1]
        return np.nan_to_num(w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2)


# --------------------------------------------------------------------------------------------------- stage 4
def closing(B, k):
    """scipy.ndimage.binary_erosion(binary_dilation(B, ones((k, k))), ones((k, k)), border_value=1)."""
    s = np.ones((k, k), bool)
    return ndi.binary_erosion(ndi.binary_dilation(np.asarray(B, bool), s), s, border_value=1)


def closing_windows(B, k):
    """The same in window terms, with slices: a = k // 2, b = k - 1 - a; dilation = OR over [y - b, y + a] with 0
    outside, erosion = AND over [y - a, y + b] with 1 outside, per axis."""
    B = np.asarray(B, bool)
    H, W = B.shape
    a, b = k // 2, k - 1 - k // 2

    def window(img, lo, hi, outside, op):
        pad = np.full((H + lo + hi, W + lo + hi), outside, bool)
        pad[lo:lo + H, lo:lo + W] = img
        out = img.copy()
        for dy in range(-lo, hi + 1):
            for dx in range(-lo, hi + 1):
                out = op(out, pad[lo + dy:lo + dy + H, lo + dx:lo + dx + W])
        return out
    d = window(B, b, a, False, np.logical_or)
    return window(d, a, b, True, np.logical_and)


# --------------------------------------------------------------------------------------------------- stage 5
def flood(img, seed, connectivity=2):
    """lab == lab[seed] for lab = scipy.ndimage.label(img == img[seed], structure)."""
    img = np.asarray(img) != 0
    structure = ndi.generate_binary_structure(2, connectivity)
    lab, _ = ndi.label(img == img[tuple(seed)], structure)
    return lab == lab[tuple(seed)]


# --------------------------------------------------------------------------------------------------- the pipeline
def pipeline(img, sigma=1.0, k=4):
    P = edge_magnitude(img)
    G = smooth(P, sigma)
    mn, mx = float(G.min()), float(G.max())
    hist = histogram(G, mn, mx)
    thr = otsu(hist, mn, mx)
    binary = P > thr
    return {'prewitt': P, 'smoothed': G, 'hist': hist, 'threshold': thr, 'binary': binary, 'initial_mask': closing(binary, k)}


def iou(a, b):
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    return float((a & b).sum()) / float((a | b).sum())


def seed_of(planted, initial_mask):
    """The pinned recipe's flood point: the middle element (row-major) of the planted mask's cells that lie outside a
    9 x 9 dilation of the closed edges."""
    far = ~ndi.binary_dilation(np.asarray(initial_mask, bool), np.ones((9, 9), bool))
    cells = np.argwhere(np.asarray(planted, bool) & far)
    return tuple(int(v) for v in cells[len(cells) // 2])


PINNED_SHAPES = ((512, 512), (200, 312), (96, 130))


@functools.lru_cache(maxsize=None)
def pinned(shape):
    """The pinned recipe on synth.corridor_mask(*shape), image seed 0, sigma 1, k 4: (planted mask, image, the f64
    pipeline's stages, flood point, the f64 final mask). Computed once per shape; callers must not write into it."""
    from axtrack_amd import synth
    planted = synth.corridor_mask(*shape)
    img = synth.transmission_image(planted, seed=0)
    stages = pipeline(img, 1.0, 4)
    seed = seed_of(planted, stages['initial_mask'])
    final = flood(stages['initial_mask'], seed, 2)
    for a in (planted, img, final, *[v for v in stages.values() if isinstance(v, np.ndarray)]):
        a.setflags(write=False)
    return planted, img, stages, seed, final


# --------------------------------------------------------------------------------------------------- flood cases
def spiral_mask(n=61):
    """A one-pixel square spiral corridor with one-pixel walls in an n x n image: one long path inside one tile."""
    m = np.zeros((n, n), bool)
    y, x, dy, dx, stuck = 0, 0, 0, 1, 0
    m[0, 0] = True
    while stuck < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
            y, x, stuck = ny, nx, 0
            m[y, x] = True
        else:
            dy, dx, stuck = dx, -dy, stuck + 1             # turn right
    return m


def diagonal_mask(n=200):
    """A one-pixel diagonal line: it crosses the corners of the 64-pixel tiles; connected only with 8 neighbours."""
    return np.eye(n, dtype=bool)
