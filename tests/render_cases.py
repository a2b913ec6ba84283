"""Cases for the render kernel (axtrack_amd/csrc/render.hip, axt_render_frames): the smallest inputs that reach every launch
shape, trail carry, strided loop, store path and rounding edge of the kernel, each with the *route facts* it claims and a
per-pixel reference. Pure numpy, no GPU, no torch: tests/test_render_routes_cpu.py proves that every case reaches the route
its facts name, tests/test_render_routes_gpu.py runs the kernel on them and compares bytes.

A `Case` holds the raw, unbinned inputs of axt_render_frames: the frames, the mask, `ts`, the slice, `grid`, `bg`, the trail
cells and the primitives (both in output coordinates, as the kernel takes them), and the byte offset at which the output is
put behind a 16-byte-aligned address. `facts_of(case)` recomputes, from those inputs and the launch constants below alone,
the facts that really hold; a claimed fact that is not among them is an error of the case, not of the kernel.

`reference(case)` paints every output frame per pixel in int64 on the whole frame and crops the slice. It knows nothing of
tiles, runs, bins or cursors; the drawing rules are those of DESIGN.md 6.8b.

The colour and glyph tables are an input of the kernel, so the cases bring their own (`TABLES`): the palette of DESIGN.md
6.8b, and a synthetic 5 x 7 font whose 665 rows differ from their neighbours, so that a glyph drawn mirrored, transposed or
from the wrong row shows. The pixels of the production font are the affair of tests/test_render.py."""
import colorsys
import functools

import numpy as np

# ---- launch constants the route facts rest on. A change of launch shape in render.hip sends you back to the cases. ---------
RT = 64                     # render.hip `constexpr int RT = 64;` (output tile edge; axt_render_tile_size)
NT = 256                    # render.hip `constexpr int NT = 256;` (threads; the stride of the trail and primitive loops)
HALO = 12                   # render.hip `constexpr int HALO = 12;` (3 box passes of radius 4)
BLUR_R, BLUR_PASSES = 4, 3  # render.hip `for (int d = -4; d <= 4; ++d)`, `for (int pass = 1; pass <= 3; ++pass)`
PX_PER_THREAD = 16          # render.hip resolve: `lx0 = (tid & 3) * 16`, `n = min(16, a.Wo - ox)`, the uint4 stores need n == 16
WG_BUDGET = 512             # render.hip axt_render_frames `runs = std::max(1, std::min(n_out, 512 / ntiles))`
GLYPHS = 95                 # render.hip `constexpr int GLYPHS = 95;` (`if (ch < 0 || ch >= GLYPHS) continue;`)
ALPHA_DIM, DIM_MAX = 26, 30  # render.hip `bufA[k] = (r > 0 && r <= 30) ? 26 : 256;`
ALPHA_GRID = 38             # render.hip `r = blend(38, 255, r)` under `a.grid && (gx % a.grid == 0 || gy % a.grid == 0)`
ALPHA_GT = 154              # render.hip `r = blend(154, 255, r)` under `gt[...]`
GREY = 107                  # render.hip `if (ok >> 24 == 3u) r = g = b = 107;`
TARGET_PATH, TARGET_CELL = 217, 255      # render.hip `r = g = b = (tg == TGT_CELL) ? 255 : 217;`
TRAIL_R = 2                 # render.hip `for (int dy = -2; dy <= 2; ++dy)` (5 x 5 squares)
P_DASHED, P_SOLID, P_GLYPH, P_RECT, P_TARGET = 0, 1, 2, 3, 4     # render.hip `enum { P_DASHED = 0, ... }`
TGT_PATH, TGT_CELL = 1, 2                                        # render.hip `enum { TGT_PATH = 1, TGT_CELL = 2 };`
LAYER_BOX, LAYER_LABEL, LAYER_HEADER = 1, 2, 3                   # key = layer << 24 | (n + 1); layer 3 is drawn grey

PALETTE = np.array([[int(round(c * 255)) for c in colorsys.hsv_to_rgb(k / 20, 1.0, 1.0)] for k in range(20)], np.uint8)
FONT = np.array([[((c * 7 + r) * 37 + 11) % 31 + 1 for r in range(7)] for c in range(GLYPHS)], np.uint8)   # bit 4 = leftmost
TABLES = np.concatenate([PALETTE.ravel(), FONT.ravel()])         # u8: palette [20, 3], then glyph rows [95, 7]


def cdiv(a, b):
    return -(-a // b)


class Case:
    def __init__(self, name, facts, frames, mask, ts, slice_, grid, bg, trail, trail_col, prims, out_offset=0):
        self.name, self.facts = name, tuple(facts)
        self.frames = np.ascontiguousarray(frames, np.float32)             # [T, H, W]
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)       # None, [H, W] or [T, H, W]
        self.ts = np.asarray(ts, np.int32)
        self.slice = tuple(int(v) for v in slice_)                        # (ymin, xmin, Ho, Wo)
        self.grid, self.bg = int(grid), bool(bg)
        self.trail = np.asarray(trail, np.int64).reshape(-1, 4)            # (frame, key, x, y), output coordinates
        self.trail_col = np.asarray(trail_col, np.uint8)                  # [keys + 1] palette index of each key
        self.prims = np.asarray(prims, np.int64).reshape(-1, 7)            # (i, x0, y0, kind, a, b, key), output coordinates
        self.out_offset = int(out_offset)                                 # bytes behind a 16-byte-aligned address
        T, H, W = self.frames.shape
        ymin, xmin, Ho, Wo = self.slice
        assert 0 <= ymin and 0 <= xmin and Ho > 0 and Wo > 0 and ymin + Ho <= H and xmin + Wo <= W
        assert len(self.ts) and (np.diff(self.ts) > 0).all() and 0 <= self.ts[0] and self.ts[-1] < T
        assert self.mask is None or self.mask.shape in ((H, W), (T, H, W))
        assert not len(self.trail) or (0 < self.trail[:, 1].min() and self.trail[:, 1].max() < len(self.trail_col))
        assert self.trail_col.max(initial=0) < 20
        assert not len(self.prims) or (0 <= self.prims[:, 0].min() and self.prims[:, 0].max() < len(self.ts))

    def __repr__(self):
        return self.name

    @property
    def mask_stride(self):
        return 0 if self.mask is None or self.mask.ndim == 2 else self.frames.shape[1] * self.frames.shape[2]

    @property
    def route(self):
        return f'render/{self.name} [{"; ".join(self.facts)}]'


def launch(case, n_out=None):
    """(ntx, nty, ntiles, chunk, number of runs) of axt_render_frames."""
    _, _, Ho, Wo = case.slice
    n_out = len(case.ts) if n_out is None else n_out
    ntx, nty = cdiv(Wo, RT), cdiv(Ho, RT)
    ntiles = ntx * nty
    runs = max(1, min(n_out, WG_BUDGET // ntiles))
    chunk = cdiv(n_out, runs)
    return ntx, nty, ntiles, chunk, cdiv(n_out, chunk)


def prim_extent(prims):
    """(w, h) of the box a primitive can touch from (x0, y0): what the binning of axtrack_amd/render.py goes by."""
    kind, a, b = prims[:, 3], prims[:, 4], prims[:, 5]
    w = np.where(kind == P_GLYPH, 5 * b, a)
    h = np.where(kind == P_GLYPH, 7 * b, np.where((kind == P_RECT) | (kind == P_TARGET), b, a))
    return w, h


def binned(case, bin_fn, csr_fn, ts=None, prims=None):
    """The lists of axt_render_frames as axtrack_amd.render.render_frames builds them, with the binning functions handed in
    (render._bin, render._csr): (trail_ptr i32 [ntiles + 1], trail i32 [n, 4], prim_ptr i32 [n_out * ntiles + 1], prims i32
    [m, 8])."""
    _, _, Ho, Wo = case.slice
    n_out = len(case.ts) if ts is None else len(ts)
    pr = case.prims if prims is None else prims
    ntiles = launch(case)[2]
    w, h = prim_extent(pr)
    idx, bins = bin_fn(pr[:, 0], pr[:, 1], pr[:, 2], w, h, Ho, Wo, RT, n_out)
    out = np.zeros((len(idx), 8), np.int32)
    out[:, :6] = pr[idx, 1:7]
    prim_ptr = csr_fn(bins, n_out * ntiles)
    tf, tk, tx, ty = case.trail.T
    five = np.full(len(tf), 2 * TRAIL_R + 1)
    cidx, cbin = bin_fn(np.zeros(len(tf), np.int64), tx - TRAIL_R, ty - TRAIL_R, five, five, Ho, Wo, RT, 1)
    order = np.lexsort((tf[cidx], cbin))                              # per tile, by frame
    cidx, cbin = cidx[order], cbin[order]
    trail = np.stack([tf[cidx], tk[cidx], tx[cidx], ty[cidx]], 1).astype(np.int32).reshape(-1, 4)
    return csr_fn(cbin, ntiles), trail, prim_ptr, out


def tail_inputs(case, k):
    """(ts, prims) of the render of ts[k:]: the primitives of the dropped frames go, the others are renumbered."""
    pr = case.prims[case.prims[:, 0] >= k].copy()
    pr[:, 0] -= k
    return case.ts[k:], pr


# =============================================================================================== the reference painter
def r8(v):
    """u8 value of a pixel, for every float: NaN and negatives 0, > 1 and +inf 255, else the f32 product v * 255 rounded half
    to even."""
    v = np.asarray(v, np.float32)
    out = np.zeros(v.shape, np.int64)
    with np.errstate(invalid='ignore'):
        out[v > 1] = 255
        mid = (v >= 0) & (v <= 1)
    p = (v[mid] * np.float32(255)).astype(np.float32).astype(np.float64)
    fl = np.floor(p)
    d = p - fl
    out[mid] = (fl + ((d > 0.5) | ((d == 0.5) & (fl % 2 == 1)))).astype(np.int64)
    return out


def blend(a, C, c):
    return (a * C + (256 - a) * c + 128) >> 8


def _box9(a, axis):
    n = a.shape[axis]
    idx = np.arange(n)
    s = np.zeros_like(a)
    for d in range(-BLUR_R, BLUR_R + 1):
        s = s + np.take(a, np.clip(idx + d, 0, n - 1), axis=axis)
    return (s + 4) // 9


def weight_map(R):
    """The blurred weight of the brightened background over the whole frame (clamped at the frame edges)."""
    w = np.where((R > 0) & (R <= DIM_MAX), ALPHA_DIM, 256).astype(np.int64)
    for axis in (1, 0):
        for _ in range(BLUR_PASSES):
            w = _box9(w, axis)
    return w


def _border(b):
    """(u, v) of the border pixels of a b x b square."""
    if b <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    e, m = np.arange(b), np.arange(1, max(b - 1, 1))
    z = lambda n, v: np.full(n, v, np.int64)
    return (np.concatenate([e, e, z(len(m), 0), z(len(m), b - 1)]), np.concatenate([z(b, 0), z(b, b - 1), m, m]))


def prim_pixels(p, lo=-(1 << 20), hi=1 << 20):
    """(x, y) arrays, output coordinates, of the pixels one primitive row (i, x0, y0, kind, a, b, key) paints; rectangles
    are cut to [lo, hi) on both axes (they may be larger than any frame)."""
    _, x0, y0, kind, a, b, _ = (int(v) for v in p)
    if kind in (P_DASHED, P_SOLID):
        u, v = _border(a)
        if kind == P_DASHED:
            keep = ((u + v) // 4) % 2 == 0
            u, v = u[keep], v[keep]
        return x0 + u, y0 + v
    if kind == P_GLYPH:
        if not 0 <= a < GLYPHS or b <= 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        bits = (FONT[a][:, None] >> (4 - np.arange(5))[None]) & 1                 # [7 rows, 5 columns]
        gy, gx = np.nonzero(np.kron(bits, np.ones((b, b), np.int64)))
        return x0 + gx, y0 + gy
    xa, xb, ya, yb = max(x0, lo), min(x0 + a, hi), max(y0, lo), min(y0 + b, hi)
    if xa >= xb or ya >= yb:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    xx, yy = np.meshgrid(np.arange(xa, xb), np.arange(ya, yb))
    return xx.ravel(), yy.ravel()


def _raise_to(plane, x, y, value):
    """plane[y, x] = max(plane[y, x], value) where (x, y) lies inside the plane."""
    ok = (x >= 0) & (x < plane.shape[1]) & (y >= 0) & (y < plane.shape[0])
    x, y = x[ok], y[ok]
    plane[y, x] = np.maximum(plane[y, x], value)


def planes(case, i):
    """The drawn layers of output frame i over the whole frame (frame coordinates), int64 [H, W] each: target (0, 1 path,
    2 cell), trail (max key of the cells of frames <= ts[i]), ground truth (0 / 1), overlay (max key)."""
    _, H, W = case.frames.shape
    ymin, xmin, _, _ = case.slice
    tgt, trail, gt, over = (np.zeros((H, W), np.int64) for _ in range(4))
    sq = np.arange(-TRAIL_R, TRAIL_R + 1)
    dx, dy = (v.ravel() for v in np.meshgrid(sq, sq))
    for f, key, x, y in case.trail[case.trail[:, 0] <= case.ts[i]]:
        _raise_to(trail, x + dx + xmin, y + dy + ymin, key)
    mine = case.prims[case.prims[:, 0] == i]
    span = max(H, W) + 1
    for want in (TGT_PATH, TGT_CELL):                                 # the cells go over the paths
        for p in mine[(mine[:, 3] == P_TARGET) & (mine[:, 6] == want)]:
            x, y = prim_pixels(p, -span, span)
            _raise_to(tgt, x + xmin, y + ymin, want)
    for p in mine[mine[:, 3] != P_TARGET]:
        x, y = prim_pixels(p, -span, span)
        _raise_to(gt if p[3] == P_SOLID else over, x + xmin, y + ymin, 1 if p[3] == P_SOLID else p[6])
    return tgt, trail, gt, over


def reference(case):
    """u8 [n_out, Ho, Wo, 3]: every output frame painted per pixel on the whole frame, then cropped."""
    _, H, W = case.frames.shape
    ymin, xmin, Ho, Wo = case.slice
    out = np.zeros((len(case.ts), Ho, Wo, 3), np.uint8)
    gy, gx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    for i, f in enumerate(case.ts):
        R = r8(case.frames[f])
        rgb = np.stack([R, np.zeros_like(R), np.zeros_like(R)], -1)
        if case.bg:
            wt = weight_map(R)[..., None]
            m = np.ones((H, W), bool) if case.mask is None else (case.mask if case.mask.ndim == 2 else case.mask[f]) != 0
            rgb = blend(wt, rgb, np.where(m, 255, 0)[..., None])
        if case.grid:
            line = (gx % case.grid == 0) | (gy % case.grid == 0)
            rgb[line] = blend(ALPHA_GRID, 255, rgb[line])
        tgt, trail, gt, over = planes(case, i)
        rgb[tgt == TGT_PATH] = TARGET_PATH
        rgb[tgt == TGT_CELL] = TARGET_CELL
        rgb[trail > 0] = PALETTE[case.trail_col[trail[trail > 0]]]
        rgb[gt > 0] = blend(ALPHA_GT, 255, rgb[gt > 0])
        rgb[over > 0] = PALETTE[((over[over > 0] & 0xFFFFFF) - 1) % 20]
        rgb[over >> 24 == LAYER_HEADER] = GREY
        assert rgb.min() >= 0 and rgb.max() <= 255
        out[i] = rgb[ymin:ymin + Ho, xmin:xmin + Wo]
    return out


# =============================================================================================== route facts
FACTS = (
    # launch shape
    'chunk == 1', 'chunk > 1, last run shorter than chunk', 'ntiles > 512, one run', 'n_out == 1',
    # trail carry
    'ts with gaps', 'cell frame strictly between two ts', 'cell later than ts[-1]',
    'cell of an earlier run visible in the first frame of a later run', 'more than 256 cells enter one tile at one frame step',
    'cell square reaches into four tiles at their shared corner', 'cell centre outside the output, square reaches in',
    'two keys on one pixel', 'trail key >= 256',
    # primitives
    'more than 256 primitives in one (frame, tile) bin', 'dashed box across a vertical and a horizontal tile border, odd b',
    'dashed box across a vertical and a horizontal tile border, even b', 'box edge 1', 'box edge 2',
    'box partly left of and above the output', 'solid box under a dashed one', 'glyphs of scale 1, 2 and 3 straddle a tile border',
    'glyph code -1', 'glyph code 95', 'rectangle clipped on all four sides', 'header over label over box on one pixel',
    'two boxes of one layer on one pixel', 'n >= 20', 'target cell over target path over grid line', 'trail over a target',
    # background
    'bg, no mask', 'bg, mask [H, W]', 'bg, mask [T, H, W]', 'mask byte 2', 'mask byte 255', 'r8 of 0, 1, 30 and 31',
    'products 0.5, 1.5, 30.5 and 254.5', 'NaN, -1, 2 and +inf pixels', 'halo reads real pixels outside the slice on all four sides',
    'slice at the top frame edge', 'slice at the left frame edge', 'slice at the bottom frame edge', 'slice at the right frame edge',
    'H < 12', 'W < 12',
    # grid
    'grid == 0', 'grid == 1', 'grid divides neither xmin nor ymin',
    # stores
    'Wo == 64', 'Wo == 80', 'Wo * 3 % 16 == 8', 'Wo % 16 == 1', 'Wo < 16', 'Wo == 1', 'Ho % 64 != 0',
    'output base at byte offset 1', 'output base at byte offset 4', 'output base at byte offset 8',
)


def _clipped(x0, y0, w, h, Ho, Wo):
    """The box cut to the output: (xa, xb, ya, yb) inclusive, and whether anything is left."""
    xa, xb, ya, yb = np.maximum(x0, 0), np.minimum(x0 + w, Wo) - 1, np.maximum(y0, 0), np.minimum(y0 + h, Ho) - 1
    return xa, xb, ya, yb, (xa <= xb) & (ya <= yb)


def tiles_touched(x0, y0, w, h, Ho, Wo):
    """The tiles the box [x0, x0 + w) x [y0, y0 + h) touches, by testing every tile of the output."""
    ntx, nty = cdiv(Wo, RT), cdiv(Ho, RT)
    ty, tx = np.divmod(np.arange(ntx * nty), ntx)
    hit = ((w > 0) & (h > 0) & (x0 < np.minimum((tx + 1) * RT, Wo)) & (x0 + w > tx * RT) & (y0 < np.minimum((ty + 1) * RT, Ho)) & (y0 + h > ty * RT))
    return np.nonzero(hit)[0]


def _count(case, i, select):
    """How many of the primitives of output frame i that `select` accepts paint each pixel of the slice: int64 [Ho, Wo]."""
    _, _, Ho, Wo = case.slice
    n = np.zeros((Ho, Wo), np.int64)
    for p in case.prims[case.prims[:, 0] == i]:
        if select(p):
            one = np.zeros((Ho, Wo), np.int64)
            _raise_to(one, *prim_pixels(p, -1, max(Ho, Wo) + 1), 1)
            n += one
    return n


def _crop(case, plane):
    ymin, xmin, Ho, Wo = case.slice
    return plane[ymin:ymin + Ho, xmin:xmin + Wo]


def facts_of(case):
    """The route facts that hold for the case's inputs (a superset of what it claims, if the case is right)."""
    T, H, W = case.frames.shape
    ymin, xmin, Ho, Wo = case.slice
    ts, n_out = case.ts, len(case.ts)
    ntx, nty, ntiles, chunk, n_runs = launch(case)
    tr, pr = case.trail, case.prims
    layer, n1 = pr[:, 6] >> 24, pr[:, 6] & 0xFFFFFF
    is_box = (pr[:, 3] == P_DASHED) | (pr[:, 3] == P_SOLID)
    dashed = pr[:, 3] == P_DASHED
    glyph = pr[:, 3] == P_GLYPH
    cache = {}

    def pl(i):
        if i not in cache:
            cache[i] = tuple(_crop(case, p) for p in planes(case, i))
        return cache[i]

    # ---- trail cells
    tf, tk, tx, ty = tr.T
    _, _, _, _, touches = _clipped(tx - TRAIL_R, ty - TRAIL_R, 5, 5, Ho, Wo)
    drawn = touches & (tf <= ts[-1])
    between = np.zeros(len(tr), bool)
    for k in range(n_out - 1):
        between |= (tf > ts[k]) & (tf < ts[k + 1])
    four = (touches & ((tx - 2) // RT != (tx + 2) // RT) & ((ty - 2) // RT != (ty + 2) // RT) & (tx - 2 >= 0) & (ty - 2 >= 0)
            & (tx + 2 < Wo) & (ty + 2 < Ho))
    outside = touches & ((tx < 0) | (tx >= Wo) | (ty < 0) | (ty >= Ho))

    def history_visible():
        for run in range(1, n_runs):
            i0 = run * chunk
            _, trail_p, _, over_p = pl(i0)
            for f, key, x, y in tr[drawn & (tf <= ts[i0 - 1])]:
                ya, yb, xa, xb = max(y - 2, 0), min(y + 3, Ho), max(x - 2, 0), min(x + 3, Wo)
                if ((trail_p[ya:yb, xa:xb] == key) & (over_p[ya:yb, xa:xb] == 0)).any():
                    return True
        return False

    def many_cells_enter():
        per_tile = {}
        for k in np.nonzero(drawn)[0]:
            for t in tiles_touched(tx[k] - 2, ty[k] - 2, 5, 5, Ho, Wo):
                per_tile.setdefault(int(t), []).append(tf[k])
        for fr in per_tile.values():
            fr = np.array(fr)
            for i in range(n_out):
                lower = -1 if i % chunk == 0 else ts[i - 1]          # the first frame of a run takes the whole history
                if ((fr > lower) & (fr <= ts[i])).sum() > NT:
                    return True
        return False

    def two_keys():
        for i in range(n_out):
            first = np.zeros((Ho, Wo), np.int64)
            for f, key, x, y in tr[tf <= ts[i]]:
                ya, yb, xa, xb = max(y - 2, 0), min(y + 3, Ho), max(x - 2, 0), min(x + 3, Wo)
                if ya < yb and xa < xb:
                    if ((first[ya:yb, xa:xb] != 0) & (first[ya:yb, xa:xb] != key)).any():
                        return True
                    first[ya:yb, xa:xb] = key
        return False

    # ---- primitives
    def crowded_bin():
        w, h = prim_extent(pr)
        n = {}
        for k in range(len(pr)):
            for t in tiles_touched(pr[k, 1], pr[k, 2], w[k], h[k], Ho, Wo):
                n[(int(pr[k, 0]), int(t))] = n.get((int(pr[k, 0]), int(t)), 0) + 1
        return max(n.values(), default=0) > NT

    x0, y0, a, b = pr[:, 1], pr[:, 2], pr[:, 4], pr[:, 5]
    crosses = (dashed & (a >= 8) & (x0 >= 0) & (y0 >= 0) & (x0 + a <= Wo) & (y0 + a <= Ho) & (x0 // RT != (x0 + a - 1) // RT)
               & (y0 // RT != (y0 + a - 1) // RT) & ((x0 + y0) % 8 != 0))
    inside = (x0 >= 0) & (y0 >= 0) & (x0 + a <= Wo) & (y0 + a <= Ho)

    def solid_under_dashed():
        s = {tuple(p[[0, 1, 2, 4]]) for p in pr[(pr[:, 3] == P_SOLID) & (a >= 8) & inside]}
        return any(tuple(p[[0, 1, 2, 4]]) in s for p in pr[dashed])

    def glyph_scales():
        ok = set()
        for p in pr[glyph & (a >= 0) & (a < GLYPHS)]:
            s = p[5]
            gx0, gy0, gx1, gy1 = p[1], p[2], p[1] + 5 * s - 1, p[2] + 7 * s - 1
            if 0 <= gx0 and 0 <= gy0 and gx1 < Wo and gy1 < Ho and (gx0 // RT != gx1 // RT or gy0 // RT != gy1 // RT):
                ok.add(int(s))
        return {1, 2, 3} <= ok

    def stacked_layers():
        for i in range(n_out):
            c = [_count(case, i, lambda p, L=L: p[3] != P_SOLID and p[3] != P_TARGET and p[6] >> 24 == L) for L in (1, 2, 3)]
            if ((c[0] > 0) & (c[1] > 0) & (c[2] > 0)).any():
                return True
        return False

    def two_boxes():
        for i in range(n_out):
            mine = pr[(pr[:, 0] == i) & dashed & (layer == LAYER_BOX)]
            if len(mine) == len(set(mine[:, 6].tolist())) and (_count(case, i, lambda p: p[3] == P_DASHED and p[6] >> 24 == LAYER_BOX) > 1).any():
                return True
        return False

    def grid_lines():
        gy, gx = np.meshgrid(np.arange(ymin, ymin + Ho), np.arange(xmin, xmin + Wo), indexing='ij')
        return (gx % case.grid == 0) | (gy % case.grid == 0) if case.grid else np.zeros((Ho, Wo), bool)

    def target_stack():
        for i in range(n_out):
            path = _count(case, i, lambda p: p[3] == P_TARGET and p[6] == TGT_PATH) > 0
            cell = _count(case, i, lambda p: p[3] == P_TARGET and p[6] == TGT_CELL) > 0
            if (path & cell & grid_lines()).any():
                return True
        return False

    # ---- background
    sl = case.frames[ts][:, ymin:ymin + Ho, xmin:xmin + Wo]
    R = r8(sl)
    prod = (np.nan_to_num(sl, nan=-1.0, posinf=-1.0, neginf=-1.0) * np.float32(255)).astype(np.float32)
    if case.mask is None:
        msl = np.ones((1, 1, 1), np.uint8)
    else:
        msl = (case.mask[None] if case.mask.ndim == 2 else case.mask[ts])[:, ymin:ymin + Ho, xmin:xmin + Wo]

    def halo_all_round():
        if not (case.bg and ymin >= HALO and xmin >= HALO and ymin + Ho + HALO <= H and xmin + Wo + HALO <= W):
            return False
        dim = (r8(case.frames[ts[0]]) > 0) & (r8(case.frames[ts[0]]) <= DIM_MAX)
        bands = (dim[ymin - HALO:ymin, xmin:xmin + Wo], dim[ymin + Ho:ymin + Ho + HALO, xmin:xmin + Wo],
                 dim[ymin:ymin + Ho, xmin - HALO:xmin], dim[ymin:ymin + Ho, xmin + Wo:xmin + Wo + HALO])
        return all(band.any() and not band.all() for band in bands)

    have = {
        'chunk == 1': chunk == 1,
        'chunk > 1, last run shorter than chunk': chunk > 1 and n_runs > 1 and n_out % chunk != 0,
        'ntiles > 512, one run': ntiles > WG_BUDGET and n_runs == 1 and n_out > 1,
        'n_out == 1': n_out == 1,
        'ts with gaps': bool((np.diff(ts) > 1).any()),
        'cell frame strictly between two ts': bool((touches & between).any()),
        'cell later than ts[-1]': bool((touches & (tf > ts[-1])).any()),
        'cell of an earlier run visible in the first frame of a later run': history_visible(),
        'more than 256 cells enter one tile at one frame step': many_cells_enter(),
        'cell square reaches into four tiles at their shared corner': bool((drawn & four).any()),
        'cell centre outside the output, square reaches in': bool((drawn & outside).any()),
        'two keys on one pixel': two_keys(),
        'trail key >= 256': bool((drawn & (tk >= 256)).any()),
        'more than 256 primitives in one (frame, tile) bin': crowded_bin(),
        'dashed box across a vertical and a horizontal tile border, odd b': bool((crosses & (a % 2 == 1)).any()),
        'dashed box across a vertical and a horizontal tile border, even b': bool((crosses & (a % 2 == 0)).any()),
        'box edge 1': bool((dashed & inside & (a == 1)).any()),
        'box edge 2': bool((dashed & inside & (a == 2)).any()),
        'box partly left of and above the output': bool((is_box & (x0 < 0) & (y0 < 0) & (x0 + a > 0) & (y0 + a > 0)).any()),
        'solid box under a dashed one': solid_under_dashed(),
        'glyphs of scale 1, 2 and 3 straddle a tile border': glyph_scales(),
        'glyph code -1': bool((glyph & (a == -1) & (b > 0)).any()),
        'glyph code 95': bool((glyph & (a == GLYPHS) & (b > 0)).any()),
        'rectangle clipped on all four sides': bool(((pr[:, 3] == P_RECT) & (x0 < 0) & (y0 < 0) & (x0 + a > Wo) & (y0 + b > Ho)).any()),
        'header over label over box on one pixel': stacked_layers(),
        'two boxes of one layer on one pixel': two_boxes(),
        'n >= 20': bool(((pr[:, 3] != P_SOLID) & (pr[:, 3] != P_TARGET) & ((layer == 1) | (layer == 2)) & (n1 - 1 >= 20)).any()),
        'target cell over target path over grid line': target_stack(),
        'trail over a target': any(((pl(i)[0] > 0) & (pl(i)[1] > 0)).any() for i in range(n_out)),
        'bg, no mask': case.bg and case.mask is None,
        'bg, mask [H, W]': case.bg and case.mask is not None and case.mask.ndim == 2,
        'bg, mask [T, H, W]': case.bg and case.mask is not None and case.mask.ndim == 3,
        'mask byte 2': case.bg and bool((msl == 2).any() and (msl == 0).any() and (msl == 1).any()),
        'mask byte 255': case.bg and bool((msl == 255).any() and (msl == 0).any() and (msl == 1).any()),
        'r8 of 0, 1, 30 and 31': case.bg and all((R == v).any() for v in (0, 1, 30, 31)),
        'products 0.5, 1.5, 30.5 and 254.5': case.bg and all((prod == np.float32(v)).any() for v in (0.5, 1.5, 30.5, 254.5)),
        'NaN, -1, 2 and +inf pixels': bool(np.isnan(sl).any() and (sl == -1).any() and (sl == 2).any() and np.isposinf(sl).any()),
        'halo reads real pixels outside the slice on all four sides': halo_all_round(),
        'slice at the top frame edge': case.bg and ymin == 0,
        'slice at the left frame edge': case.bg and xmin == 0,
        'slice at the bottom frame edge': case.bg and ymin + Ho == H,
        'slice at the right frame edge': case.bg and xmin + Wo == W,
        'H < 12': case.bg and H < HALO,
        'W < 12': case.bg and W < HALO,
        'grid == 0': case.grid == 0,
        'grid == 1': case.grid == 1,
        'grid divides neither xmin nor ymin': case.grid > 1 and xmin % case.grid != 0 and ymin % case.grid != 0 and bool(grid_lines().any()),
        'Wo == 64': Wo == 64,
        'Wo == 80': Wo == 80,
        'Wo * 3 % 16 == 8': Wo * 3 % 16 == 8 and Wo >= PX_PER_THREAD and Ho > 1,
        'Wo % 16 == 1': Wo % PX_PER_THREAD == 1 and Wo > PX_PER_THREAD,
        'Wo < 16': Wo < PX_PER_THREAD,
        'Wo == 1': Wo == 1,
        'Ho % 64 != 0': Ho % RT != 0,
        'output base at byte offset 1': case.out_offset == 1,
        'output base at byte offset 4': case.out_offset == 4,
        'output base at byte offset 8': case.out_offset == 8,
    }
    assert set(have) == set(FACTS)
    return {name for name, ok in have.items() if ok}


# =============================================================================================== the cases
def _key(layer, n):
    return (layer << 24) | (n + 1)


def _frames(rng, T, H, W):
    """Pixels with many dim ones (0 < r8 <= 30), exact zeros and bright ones."""
    fr = rng.random((T, H, W), dtype=np.float32) * np.float32(0.25)
    fr[rng.random((T, H, W)) < 0.1] = 0
    bright = rng.random((T, H, W)) < 0.1
    fr[bright] = rng.random(int(bright.sum()), dtype=np.float32)
    return fr


def _mask(rng, shape, values=(0, 1)):
    """Blocks of 8 x 8 pixels, so that the mask has regions as a corridor mask has."""
    *lead, H, W = shape
    small = rng.integers(0, len(values), size=(*lead, cdiv(H, 8), cdiv(W, 8)))
    return np.asarray(values, np.uint8)[np.kron(small, np.ones((8, 8), np.int64))[..., :H, :W]]


def _scatter(rng, ts, Ho, Wo, boxes=3, cells=30, first_key=1):
    """Ordinary content for every output frame: dashed boxes with a label of three glyphs, a solid box, a header of four
    glyphs and a bar at the top right, a target path with a target cell; and trail cells over the frames up to ts[-1] + 1.
    Returns (primitive rows, trail rows)."""
    prims, trail = [], []
    for i in range(len(ts)):
        for _ in range(boxes):
            b = int(rng.integers(3, 40))
            x0, y0 = int(rng.integers(-b // 2, Wo)), int(rng.integers(-b // 2, Ho))
            n, s = int(rng.integers(0, 60)), int(rng.integers(1, 3))
            prims.append((i, x0, y0, P_DASHED, b, 0, _key(LAYER_BOX, n)))
            prims += [(i, x0 + 6 * s * k, y0 - 8 * s, P_GLYPH, int(rng.integers(0, GLYPHS)), s, _key(LAYER_LABEL, n)) for k in range(3)]
        prims.append((i, x0 + 2, y0 - 1, P_SOLID, b, 0, 0))
        prims += [(i, Wo - 4 - 23 + 6 * k, 4, P_GLYPH, int(rng.integers(0, GLYPHS)), 1, LAYER_HEADER << 24) for k in range(4)]
        prims.append((i, Wo - 4 - 30, 14, P_RECT, 30, 2, LAYER_HEADER << 24))
        px, py = int(rng.integers(-4, Wo)), int(rng.integers(-4, Ho))
        prims.append((i, px, py, P_TARGET, int(rng.integers(5, 40)), 5, TGT_PATH))
        prims.append((i, px + 3, py, P_TARGET, 5, int(rng.integers(5, 12)), TGT_PATH))
        prims.append((i, px + int(rng.integers(0, 8)), py + int(rng.integers(-3, 4)), P_TARGET, 5, 5, TGT_CELL))
    fr = np.sort(rng.integers(0, int(ts[-1]) + 2, size=cells))
    x, y = int(rng.integers(0, Wo)), int(rng.integers(0, Ho))
    for k in range(cells):
        x, y = int(np.clip(x + rng.integers(-3, 4), -2, Wo + 1)), int(np.clip(y + rng.integers(-3, 4), -2, Ho + 1))
        trail.append((int(fr[k]), first_key + k // 4, x, y))
    return prims, trail


def _trail_col(trail):
    top = max((t[1] for t in trail), default=0)
    return (np.arange(top + 1) * 7 % 20).astype(np.uint8)


def _with_product(p):
    """An f32 v in [0, 1] whose f32 product v * 255 is exactly p."""
    v = np.float32(p) / np.float32(255)
    down, up = [v], [v]
    for _ in range(4):
        down.append(np.nextafter(down[-1], np.float32(0)))
        up.append(np.nextafter(up[-1], np.float32(1)))
    for c in down + up:
        if np.float32(np.float32(c) * np.float32(255)) == np.float32(p):
            return np.float32(c)
    raise AssertionError(p)


def _glyph_with(gy, gx):
    """A glyph code whose font row gy has column gx set."""
    return int(np.nonzero((FONT[:, gy] >> (4 - gx)) & 1)[0][0])


def _case_prims():
    rng = np.random.default_rng(101)
    H, W, sl, ts, grid = 150, 170, (13, 17, 100, 130), [0, 1], 40
    Ho, Wo = sl[2:]
    prims, trail = _scatter(rng, ts, Ho, Wo, boxes=2, cells=12, first_key=10)
    code = _glyph_with(3, 2)
    prims += [
        (0, 53, 58, P_DASHED, 21, 0, _key(LAYER_BOX, 4)),            # odd b over the corner (64, 64); x0 + y0 = 111
        (0, 53, 58, P_SOLID, 21, 0, 0),                               # the solid box under it
        (0, 40, 45, P_DASHED, 30, 0, _key(LAYER_BOX, 47)),           # even b over the corner, crosses the first; n >= 20
        (0, 51, 55, P_GLYPH, code, 1, _key(LAYER_LABEL, 4)),         # label and header glyph over the box corner (53, 58)
        (0, 51, 55, P_GLYPH, code, 1, LAYER_HEADER << 24),
        (0, 49, 50, P_GLYPH, _glyph_with(0, 0), 1, _key(LAYER_LABEL, 30)),
        (0, 5, 90, P_DASHED, 1, 0, _key(LAYER_BOX, 1)), (0, 9, 90, P_DASHED, 2, 0, _key(LAYER_BOX, 2)),
        (0, 13, 90, P_SOLID, 1, 0, 0), (0, 17, 90, P_SOLID, 2, 0, 0), (0, 21, 90, P_DASHED, 0, 0, _key(LAYER_BOX, 3)),
        (0, -7, -9, P_DASHED, 25, 0, _key(LAYER_BOX, 8)), (0, -4, -3, P_SOLID, 11, 0, 0),
        (0, 62, 20, P_GLYPH, 10, 1, _key(LAYER_LABEL, 5)),           # scale 1 over x = 64
        (0, 120, 30, P_GLYPH, 33, 2, _key(LAYER_LABEL, 6)),          # scale 2 over x = 128
        (0, 90, 50, P_GLYPH, 64, 3, _key(LAYER_LABEL, 7)),           # scale 3 over y = 64
        (0, 123, 70, P_GLYPH, 94, 3, _key(LAYER_LABEL, 9)),          # scale 3 over x = 128 and the right output edge
        (0, 80, 5, P_GLYPH, -1, 1, _key(LAYER_LABEL, 5)), (0, 86, 5, P_GLYPH, GLYPHS, 2, _key(LAYER_LABEL, 5)),
        (0, 10, 25, P_TARGET, 34, 5, TGT_PATH),                       # over the grid line y = 40 - 13 = 27
        (0, 20, 25, P_TARGET, 5, 5, TGT_CELL), (0, 41, 23, P_TARGET, 5, 5, TGT_CELL),
        (0, 20, 25, P_TARGET, 9, 5, TGT_PATH),                        # a path listed AFTER the cell it lies under
    ]
    trail += [(0, 3, 12, 27), (0, 3, 13, 28), (1, 4, 22, 27)]         # over the target path and the target cell
    prims += [(1, 3 * (k % 20), 3 * (k // 20), P_RECT, 2, 2, _key(LAYER_BOX, k)) for k in range(300)]     # one bin of frame 1
    facts = ['chunk == 1', 'more than 256 primitives in one (frame, tile) bin', 'dashed box across a vertical and a horizontal tile border, odd b',
             'dashed box across a vertical and a horizontal tile border, even b', 'box edge 1', 'box edge 2', 'box partly left of and above the output',
             'solid box under a dashed one', 'glyphs of scale 1, 2 and 3 straddle a tile border', 'glyph code -1', 'glyph code 95',
             'header over label over box on one pixel', 'two boxes of one layer on one pixel', 'n >= 20', 'target cell over target path over grid line',
             'trail over a target', 'bg, mask [H, W]', 'mask byte 2', 'mask byte 255', 'halo reads real pixels outside the slice on all four sides',
             'grid divides neither xmin nor ymin', 'Ho % 64 != 0']
    return Case('prims', facts, _frames(rng, 2, H, W), _mask(rng, (H, W), (0, 1, 2, 255)), ts, sl, grid, True, trail, _trail_col(trail), prims)


def _case_trails():
    rng = np.random.default_rng(102)
    H, W, sl, ts = 120, 110, (11, 4, 100, 100), [1, 3, 4, 7]
    prims, trail = _scatter(rng, ts, 100, 100, boxes=1, cells=20, first_key=400)
    trail += [
        (0, 1, 10, 10), (1, 2, 14, 10), (2, 3, 18, 10), (3, 4, 22, 10), (4, 6, 26, 10), (5, 7, 30, 10), (6, 8, 34, 10), (7, 11, 38, 10),
        (8, 12, 42, 10), (9, 13, 46, 10),                             # one cell per frame 0..9: frames 2, 5, 6 between, 8, 9 never
        (1, 5, 30, 30), (3, 9, 31, 31), (4, 10, 29, 32),              # two and three keys on a pixel, the later frame above
        (3, 300, 63, 63), (1, 2, 64, 64), (4, 70000, 65, 62),         # the corner of four tiles; keys >= 256
        (1, 14, -1, 30), (3, 15, 101, 50), (4, 16, 50, -2), (2, 17, 50, 101), (1, 18, -2, -2), (3, 19, 101, 101),
        (1, 20, -3, 40), (1, 21, 40, 102),                            # squares that end one pixel outside: nothing drawn
    ]
    facts = ['chunk == 1', 'ts with gaps', 'cell frame strictly between two ts', 'cell later than ts[-1]',
             'cell square reaches into four tiles at their shared corner', 'cell centre outside the output, square reaches in',
             'two keys on one pixel', 'trail key >= 256', 'grid == 0', 'Ho % 64 != 0']
    return Case('trails', facts, _frames(rng, 8, H, W), None, ts, sl, 0, False, trail, _trail_col(trail), prims)


def _case_single_frame():
    rng = np.random.default_rng(103)
    ts = [2]
    prims, trail = _scatter(rng, ts, 64, 64, boxes=2, cells=16)
    facts = ['n_out == 1', 'chunk == 1', 'Wo == 64', 'grid == 1', 'bg, no mask', 'slice at the top frame edge', 'slice at the left frame edge',
             'slice at the bottom frame edge', 'slice at the right frame edge']
    return Case('single_frame_64', facts, _frames(rng, 3, 64, 64), None, ts, (0, 0, 64, 64), 1, True, trail, _trail_col(trail), prims)


def _case_runs():
    """640 x 704 output: 110 tiles, 5 frames -> 4 runs, chunk 2, runs [0, 1], [2, 3], [4]."""
    rng = np.random.default_rng(104)
    H, W, sl, ts = 660, 717, (10, 13, 640, 704), [0, 2, 3, 5, 6]
    prims, trail = _scatter(rng, ts, 640, 704, boxes=6, cells=200, first_key=2000)
    trail += [(0, 1, 100, 100), (1, 2, 300, 200), (2, 3, 500, 300), (3, 4, 200, 400), (4, 5, 400, 500), (5, 6, 600, 600), (6, 7, 650, 50),
              (7, 8, 50, 600)]                                        # one lone cell per frame 0..7, each in a tile of its own
    # 300 cells of frame 4 in tile (3, 5): they enter at output frame 3 (ts 5), the second frame of run 1; stride 3, keys rising
    trail += [(4, 100 + k, 5 * RT + 3 * (k % 20) + 2, 3 * RT + 3 * (k // 20) + 2) for k in range(300)]
    # 280 cells of frames 0..6 in tile (7, 2): the whole history enters at the first frame of every run
    trail += [(k % 7, 500 + k, 2 * RT + 3 * (k % 20) + 2, 7 * RT + 3 * (k // 20) + 2) for k in range(280)]
    facts = ['chunk > 1, last run shorter than chunk', 'ts with gaps', 'cell frame strictly between two ts', 'cell later than ts[-1]',
             'cell of an earlier run visible in the first frame of a later run', 'more than 256 cells enter one tile at one frame step',
             'bg, mask [T, H, W]', 'slice at the right frame edge']
    return Case('runs_110_tiles', facts, _frames(rng, 7, H, W), _mask(rng, (7, H, W)), ts, sl, 50, True, trail, _trail_col(trail), prims)


def _case_strip():
    """16 x 32 769 output: 513 tiles (the last one pixel wide), one run of 3 frames."""
    rng = np.random.default_rng(105)
    Wo = 512 * RT + 1
    H, W, sl, ts = 20, Wo + 5, (2, 3, 16, Wo), [1, 4, 5]
    prims, trail = _scatter(rng, ts, 16, Wo, boxes=40, cells=100, first_key=1000)
    trail += [(f, 1 + f, 4000 * f + 70, 8) for f in range(8)]          # one lone cell per frame 0..7
    trail += [(f, 20 + f, Wo - 1 - f, 3 + f) for f in range(8)]        # and around the one-pixel tile at the right end
    # 300 cells of frames 2..4 in tile 300: they enter at output frame 1 (ts 4), inside the run
    trail += [(2 + k % 3, 100 + k, 300 * RT + 3 * (k % 20) + 2, (k // 20) + 1) for k in range(300)]
    prims += [(1, 511 * RT + 50, -3, P_DASHED, 22, 0, _key(LAYER_BOX, 12)), (2, Wo - 9, 2, P_GLYPH, 40, 2, _key(LAYER_LABEL, 12))]
    facts = ['ntiles > 512, one run', 'ts with gaps', 'cell frame strictly between two ts', 'cell later than ts[-1]',
             'more than 256 cells enter one tile at one frame step', 'Wo % 16 == 1', 'Ho % 64 != 0']
    return Case('strip_513_tiles', facts, _frames(rng, 6, H, W), None, ts, sl, 100, False, trail, _trail_col(trail), prims)


def _case_bg_values():
    rng = np.random.default_rng(106)
    H, W, ts = 40, 48, [0, 1]
    fr = _frames(rng, 2, H, W)
    special = [0.0, 0.0019, 1 / 255, 30 / 255, 31 / 255, _with_product(0.5), _with_product(1.5), _with_product(30.5), _with_product(254.5),
               _with_product(2.5), _with_product(29.5), np.nan, -1.0, 2.0, np.inf, -np.inf, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)),
               1e-45, -1e-45]
    for t in range(2):
        for k, v in enumerate(special * 3):                           # three of each per frame, in dim and in bright surroundings
            fr[t, 2 + 3 * (k // 12), 1 + 4 * (k % 12) + t] = v
    prims, trail = _scatter(rng, ts, H, W, boxes=1, cells=8)
    facts = ['chunk == 1', 'bg, mask [T, H, W]', 'r8 of 0, 1, 30 and 31', 'products 0.5, 1.5, 30.5 and 254.5', 'NaN, -1, 2 and +inf pixels',
             'grid == 0', 'output base at byte offset 1', 'Ho % 64 != 0']
    return Case('bg_values', facts, fr, _mask(rng, (2, H, W)), ts, (0, 0, H, W), 0, True, trail, _trail_col(trail), prims, out_offset=1)


def _small(name, seed, H, W, sl, facts, mask=None, ts=(0, 1), grid=7, bg=True, out_offset=0, boxes=2):
    rng = np.random.default_rng(seed)
    prims, trail = _scatter(rng, list(ts), sl[2], sl[3], boxes=boxes, cells=10)
    T = ts[-1] + 1
    m = None if mask is None else _mask(rng, (H, W) if mask == 2 else (T, H, W))
    return Case(name, facts, _frames(rng, T, H, W), m, list(ts), sl, grid, bg, trail, _trail_col(trail), prims, out_offset)


def _case_rect():
    c = _small('rect_over_all', 113, 30, 40, (5, 6, 20, 24), ['rectangle clipped on all four sides', 'chunk == 1'], bg=False)
    c.prims = np.concatenate([c.prims, [[0, -3, -2, P_RECT, 40, 30, _key(LAYER_BOX, 3)], [1, -1, -1, P_RECT, 26, 22, LAYER_HEADER << 24]]])
    return c


@functools.lru_cache(maxsize=None)
def all_cases():
    edges = ['slice at the top frame edge', 'slice at the left frame edge', 'slice at the bottom frame edge', 'slice at the right frame edge']
    return (
        _case_prims(), _case_trails(), _case_single_frame(), _case_runs(), _case_strip(), _case_bg_values(), _case_rect(),
        _small('low_frame_wo80', 107, 9, 80, (0, 0, 9, 80), ['H < 12', 'Wo == 80', 'bg, no mask', 'output base at byte offset 4'] + edges, out_offset=4),
        _small('narrow_frame_wo7', 108, 70, 7, (0, 0, 70, 7), ['W < 12', 'Wo < 16', 'bg, mask [H, W]', 'Ho % 64 != 0'] + edges, mask=2),
        _small('top_left_wo72', 109, 100, 100, (0, 0, 40, 72), ['Wo * 3 % 16 == 8', 'bg, mask [H, W]'] + edges[:2], mask=2),
        _small('bottom_right_wo72', 110, 100, 100, (60, 28, 40, 72), ['Wo * 3 % 16 == 8', 'output base at byte offset 8', 'bg, no mask'] + edges[2:],
               out_offset=8),
        _small('one_column', 111, 30, 30, (3, 29, 20, 1), ['Wo == 1', 'Wo < 16', 'bg, no mask', 'slice at the right frame edge'], boxes=6),
        _small('wo17', 112, 20, 40, (4, 6, 9, 17), ['Wo % 16 == 1', 'bg, mask [T, H, W]'], mask=3),
        _small('wo80_two_columns', 114, 90, 100, (6, 9, 70, 80), ['Wo == 80', 'Ho % 64 != 0', 'grid divides neither xmin nor ymin'], bg=False, grid=16),
    )
