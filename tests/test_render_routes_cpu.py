"""The cases of tests/render_cases.py, checked on the CPU: every case reaches the route its facts name, every fact of the list
is claimed, the production binning (render._bin, render._csr) equals a brute-force loop over (element, tile) intersections on
every case's lists, and a tile-wise numpy model of render.hip -- the same runs, tiles, cursor, LDS planes and store groups,
working from the binned lists -- paints what the per-pixel reference paints. The last block breaks one route at a time in
that model and shows that a named case then differs from its reference: the cases are sharp enough to see those bugs."""
import numpy as np
import pytest

import render_cases as rc
from axtrack_amd import render
from render_cases import RT, NT, HALO, P_DASHED, P_SOLID, P_GLYPH, P_RECT, P_TARGET, TGT_PATH, TGT_CELL

CASES = rc.all_cases()
BY_NAME = {c.name: c for c in CASES}
BW = RT + 2 * HALO
_CACHE = {}


def lists_of(case):
    if ('lists', case.name) not in _CACHE:
        _CACHE['lists', case.name] = rc.binned(case, render._bin, render._csr)
    return _CACHE['lists', case.name]


def reference_of(case):
    if ('ref', case.name) not in _CACHE:
        _CACHE['ref', case.name] = rc.reference(case)
    return _CACHE['ref', case.name]


# ------------------------------------------------------------------------------------------------- the cases themselves
def test_case_names_are_unique():
    assert len(BY_NAME) == len(CASES)


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_route_facts_hold(case):
    have = rc.facts_of(case)
    assert case.facts and not set(case.facts) - have, f'{case.route}: claimed but not true: {sorted(set(case.facts) - have)}'
    assert not set(case.facts) - set(rc.FACTS), f'{case.route}: not in the list of facts: {sorted(set(case.facts) - set(rc.FACTS))}'


def test_every_fact_is_claimed():
    claimed = {f for c in CASES for f in c.facts}
    assert not set(rc.FACTS) - claimed, f'no case claims {sorted(set(rc.FACTS) - claimed)}'


def test_constants_and_tables_match_the_python_side():
    assert np.array_equal(rc.PALETTE, render.PALETTE)
    assert rc.FONT.shape == render.GLYPH_ROWS.shape == (rc.GLYPHS, 7) and rc.FONT.max() < 32 and rc.FONT.min() > 0
    assert len(rc.TABLES) == render.PALETTE.size + render.GLYPH_ROWS.size == 60 + 7 * rc.GLYPHS
    assert (rc.ALPHA_GRID, rc.ALPHA_GT, rc.ALPHA_DIM) == (render.WHITE_ALPHA_GRID, render.WHITE_ALPHA_GT, render.BG_ALPHA_DIM)
    assert (rc.GREY,) * 3 == render.HEADER_RGB and (rc.TARGET_PATH,) * 3 == render.TARGET_PATH_RGB and (rc.TARGET_CELL,) * 3 == render.TARGET_RGB
    assert (P_DASHED, P_SOLID, P_GLYPH, P_RECT, P_TARGET) == (render.P_DASHED, render.P_SOLID, render.P_GLYPH, render.P_RECT, render.P_TARGET)
    assert (TGT_PATH, TGT_CELL) == (render.TGT_PATH, render.TGT_CELL)
    assert (rc.LAYER_BOX, rc.LAYER_LABEL, rc.LAYER_HEADER) == (render.LAYER_BOX, render.LAYER_LABEL, render.LAYER_HEADER)
    # neighbouring font rows differ, and no glyph is its own mirror image in every row
    assert (rc.FONT[:, 1:] != rc.FONT[:, :-1]).all()
    mirror = sum(((rc.FONT >> k) & 1) << (4 - k) for k in range(5))
    assert (mirror != rc.FONT).any(axis=1).all()


def test_r8_is_defined_for_every_float():
    f = np.float32
    assert rc.r8(np.array([np.nan, -1, -0.0, 0, 1e-45, 1, 2, np.inf, -np.inf], f)).tolist() == [0, 0, 0, 0, 0, 255, 255, 255, 0]
    for p, want in ((0.5, 0), (1.5, 2), (2.5, 2), (29.5, 30), (30.5, 30), (254.5, 254)):
        v = rc._with_product(p)
        assert f(v * f(255)) == f(p) and rc.r8(v) == want, (p, v)
    assert rc.r8(np.array([1 / 255, 30 / 255, 31 / 255, 0.0019], f)).tolist() == [1, 30, 31, 0]


# ------------------------------------------------------------------------------------------------- binning
def brute_bins(i, x0, y0, w, h, Ho, Wo, ntiles):
    """(element, bin) of every (primitive, tile) whose rectangles intersect, bins ascending, elements ascending within a bin."""
    pairs = sorted((int(i[k]) * ntiles + int(t), k) for k in range(len(i)) for t in rc.tiles_touched(x0[k], y0[k], w[k], h[k], Ho, Wo))
    return np.array([k for _, k in pairs], np.int64), np.array([b for b, _ in pairs], np.int64)


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_bin_and_csr_equal_the_brute_force(case):
    _, _, Ho, Wo = case.slice
    ntiles, n_out = rc.launch(case)[2], len(case.ts)
    pr = case.prims
    w, h = rc.prim_extent(pr)
    idx, bins = render._bin(pr[:, 0], pr[:, 1], pr[:, 2], w, h, Ho, Wo, RT, n_out)
    b_idx, b_bins = brute_bins(pr[:, 0], pr[:, 1], pr[:, 2], w, h, Ho, Wo, ntiles)
    assert np.array_equal(bins, b_bins) and np.array_equal(idx, b_idx), f'{case.route}: primitives'
    assert (np.diff(bins) >= 0).all()
    ptr = render._csr(bins, n_out * ntiles)
    assert ptr.dtype == np.int32 and len(ptr) == n_out * ntiles + 1 and ptr[0] == 0 and ptr[-1] == len(idx)
    for b in np.unique(b_bins):
        assert np.array_equal(idx[ptr[b]:ptr[b + 1]], b_idx[b_bins == b]), f'{case.route}: bin {b}'
    assert (np.diff(ptr)[np.setdiff1d(np.arange(n_out * ntiles), b_bins)] == 0).all()
    # the trail lists as render_frames builds them: per tile, sorted by frame, equal frames in their original order
    trail_ptr, trail, _, _ = lists_of(case)
    tf, tk, tx, ty = case.trail.T
    five = np.full(len(tf), 5)
    c_idx, c_bins = brute_bins(np.zeros(len(tf), np.int64), tx - 2, ty - 2, five, five, Ho, Wo, ntiles)
    assert len(trail_ptr) == ntiles + 1 and trail_ptr[-1] == len(c_idx) == len(trail)
    for t in range(ntiles):
        mine = c_idx[c_bins == t]
        mine = mine[np.argsort(tf[mine], kind='stable')]
        got = trail[trail_ptr[t]:trail_ptr[t + 1]]
        assert np.array_equal(got, case.trail[mine]), f'{case.route}: trail cells of tile {t}'
        assert (np.diff(got[:, 0]) >= 0).all()


def test_bin_drops_what_lies_outside_and_keeps_empty_input():
    z = np.zeros(0, np.int64)
    idx, bins = render._bin(z, z, z, z, z, 100, 100, RT, 2)
    assert len(idx) == len(bins) == 0 and np.array_equal(render._csr(bins, 8), np.zeros(9, np.int32))
    a = lambda *v: np.array(v, np.int64)
    idx, bins = render._bin(a(0, 1, 1, 0), a(-5, 100, 63, 10), a(-5, 0, 63, 10), a(5, 9, 2, 0), a(5, 9, 2, 3), 100, 100, RT, 2)
    assert idx.tolist() == [2, 2, 2, 2] and bins.tolist() == [4, 5, 6, 7]


# ------------------------------------------------------------------------------------------------- the tile-wise model
DEFECTS = ('no_resplat', 'cursor_not_carried', 'search_lt', 'dash_from_tile', 'blur_clamped_at_slice', 'round_half_away',
           'row_tail_ignores_n', 'path_over_cell', 'overlay_without_layer', 'stride_stops_at_256', 'grid_from_output')


def model_r8(v, defect=None):
    v = np.asarray(v, np.float32)
    p = np.clip(np.where(np.isnan(v), np.float32(0), v), np.float32(0), np.float32(1)) * np.float32(255)       # fmaxf(NaN, 0) = 0
    assert p.dtype == np.float32
    return (np.floor(p.astype(np.float64) + 0.5) if defect == 'round_half_away' else np.rint(p)).astype(np.int64)


def tile_weights(R, fy0, fx0, clamp):
    """The weight of the tile's pixels as render_tiles computes it in LDS: an 88 x 88 window, ping-pong buffers, three
    horizontal passes over every row and three vertical ones over the tile's columns, entries outside [ylo, yhi) x [xlo, xhi)
    (the frame) never written and never read."""
    ylo, yhi, xlo, xhi = clamp
    wy0, wx0 = fy0 - HALO, fx0 - HALO
    gy, gx = wy0 + np.arange(BW), wx0 + np.arange(BW)
    iny, inx = (gy >= ylo) & (gy < yhi), (gx >= xlo) & (gx < xhi)
    A, B = np.full((BW, BW), -10 ** 9, np.int64), np.full((BW, BW), -10 ** 9, np.int64)       # poison: a stale read shows
    r = R[np.ix_(gy[iny], gx[inx])]
    A[np.ix_(iny, inx)] = np.where((r > 0) & (r <= rc.DIM_MAX), rc.ALPHA_DIM, 256)
    rows = np.nonzero(iny)[0]
    for ps in (1, 2, 3):
        src, dst = (A, B) if ps & 1 else (B, A)
        cols = np.arange(4 * ps, BW - 4 * ps)
        cols = cols[inx[cols]]
        s = sum(src[np.ix_(rows, np.clip(gx[cols] + d, xlo, xhi - 1) - wx0)] for d in range(-4, 5))
        dst[np.ix_(rows, cols)] = (s + 4) // 9
    cols = HALO + np.arange(RT)
    cols = cols[inx[cols]]
    for ps in (1, 2, 3):
        src, dst = (B, A) if ps & 1 else (A, B)
        rws = np.arange(4 * ps, BW - 4 * ps)
        rws = rws[iny[rws]]
        s = sum(src[np.ix_(np.clip(gy[rws] + d, ylo, yhi - 1) - wy0, cols)] for d in range(-4, 5))
        dst[np.ix_(rws, cols)] = (s + 4) // 9
    return A[HALO:HALO + RT, HALO:HALO + RT]


def model(case, lists, defect=None, tiles=None):
    """render_tiles and its launch in numpy. Returns (u8 [n_out, Ho, Wo, 3], bool [Ho, Wo] of the pixels of the computed
    tiles). tiles: the tiles to compute (default all)."""
    assert defect is None or defect in DEFECTS
    trail_ptr, trail, prim_ptr, prims = lists
    _, H, W = case.frames.shape
    ymin, xmin, Ho, Wo = case.slice
    ts, n_out = case.ts, len(case.ts)
    ntx, nty, ntiles, chunk, n_runs = rc.launch(case)
    tiles = range(ntiles) if tiles is None else tiles
    flat = np.zeros(n_out * Ho * Wo * 3 + 48, np.uint8)
    spills = []
    done = np.zeros((Ho, Wo), bool)
    R_of = {}
    stop = NT if defect == 'stride_stops_at_256' else 1 << 30
    clamp = (ymin, ymin + Ho, xmin, xmin + Wo) if defect == 'blur_clamped_at_slice' else (0, H, 0, W)
    rank = (lambda k: ((k & 0xFFFFFF) << 8) | (k >> 24)) if defect == 'overlay_without_layer' else (lambda k: k)
    for run in range(n_runs):
        i0, i1 = run * chunk, min(run * chunk + chunk, n_out)
        for tile in tiles:
            oy0, ox0 = (tile // ntx) * RT, (tile % ntx) * RT
            fy0, fx0 = oy0 + ymin, ox0 + xmin
            done[oy0:oy0 + RT, ox0:ox0 + RT] = True
            canvas = np.zeros((RT, RT), np.int64)
            first, pend = int(trail_ptr[tile]), int(trail_ptr[tile + 1])
            p = first
            if defect == 'no_resplat' and run > 0:                    # as if the cursor came over from the previous run
                p = first + int(np.searchsorted(trail[first:pend, 0], ts[i0 - 1], 'right'))
            for i in range(i0, i1):
                f = int(ts[i])
                lo, hi = p, pend
                while lo < hi:
                    mid = (lo + hi) >> 1
                    if (trail[mid, 0] < f) if defect == 'search_lt' else (trail[mid, 0] <= f):
                        lo = mid + 1
                    else:
                        hi = mid
                start = p
                if defect == 'cursor_not_carried' and i > i0:         # the cells of frame f alone: right for contiguous ts only
                    start = first + int(np.searchsorted(trail[first:pend, 0], f, 'left'))
                for _, key, x, y in trail[start:lo][:stop]:
                    lx, ly = x - ox0, y - oy0
                    ya, yb, xa, xb = max(ly - 2, 0), min(ly + 3, RT), max(lx - 2, 0), min(lx + 3, RT)
                    if ya < yb and xa < xb:
                        canvas[ya:yb, xa:xb] = np.maximum(canvas[ya:yb, xa:xb], key)
                p = lo
                over, gt, tgt = np.zeros((RT, RT), np.int64), np.zeros((RT, RT), bool), np.zeros((RT, RT), np.int64)
                q0, q1 = int(prim_ptr[i * ntiles + tile]), int(prim_ptr[i * ntiles + tile + 1])
                mine = prims[q0:q1][:stop].astype(np.int64)

                def raise_over(yy, xx, key):
                    old = over[yy, xx]
                    over[yy, xx] = np.where(rank(np.int64(key)) > rank(old), key, old)

                for x0, y0, kind, a, b, key, _, _ in mine:
                    x0, y0 = x0 - ox0, y0 - oy0
                    if kind in (P_DASHED, P_SOLID):
                        for e in range(4):
                            row, fixed = e < 2, (a - 1 if e & 1 else 0)
                            frm, to = (0, a) if row else (1, a - 1)
                            base = x0 if row else y0
                            c = (y0 if row else x0) + fixed
                            if c < 0 or c >= RT:
                                continue
                            s = np.arange(max(frm, -base), min(to, RT - base))
                            xx, yy = (x0 + s, np.full(len(s), c)) if row else (np.full(len(s), c), y0 + s)
                            if kind == P_DASHED:
                                keep = (((xx + yy) if defect == 'dash_from_tile' else (s + fixed)) >> 2) & 1 == 0
                                raise_over(yy[keep], xx[keep], key)
                            else:
                                gt[yy, xx] = True
                    elif kind == P_GLYPH:
                        if a < 0 or a >= rc.GLYPHS:
                            continue
                        for g_y in range(7):
                            for g_x in range(5):
                                if (rc.TABLES[60 + a * 7 + g_y] >> (4 - g_x)) & 1:
                                    ya, yb = max(y0 + g_y * b, 0), min(y0 + g_y * b + b, RT)
                                    xa, xb = max(x0 + g_x * b, 0), min(x0 + g_x * b + b, RT)
                                    if ya < yb and xa < xb:
                                        yy, xx = np.meshgrid(np.arange(ya, yb), np.arange(xa, xb), indexing='ij')
                                        raise_over(yy.ravel(), xx.ravel(), key)
                    elif kind == P_RECT:
                        ya, yb, xa, xb = max(y0, 0), min(y0 + b, RT), max(x0, 0), min(x0 + a, RT)
                        if ya < yb and xa < xb:
                            yy, xx = np.meshgrid(np.arange(ya, yb), np.arange(xa, xb), indexing='ij')
                            raise_over(yy.ravel(), xx.ravel(), key)
                order = (TGT_CELL, TGT_PATH) if defect == 'path_over_cell' else (TGT_PATH, TGT_CELL)
                for want in order:                                    # two passes with a barrier between them
                    for x0, y0, kind, a, b, key, _, _ in mine:
                        if kind == P_TARGET and key == want:
                            x0, y0 = x0 - ox0, y0 - oy0
                            tgt[max(y0, 0):max(min(y0 + b, RT), 0), max(x0, 0):max(min(x0 + a, RT), 0)] = want
                # resolve: the tile's pixels inside the output
                h, w = min(RT, Ho - oy0), min(RT, Wo - ox0)
                if f not in R_of:
                    R_of[f] = model_r8(case.frames[f], defect)
                R = R_of[f][fy0:fy0 + h, fx0:fx0 + w]
                rgb = np.stack([R, np.zeros_like(R), np.zeros_like(R)], -1)
                if case.bg:
                    wt = tile_weights(R_of[f], fy0, fx0, clamp)[:h, :w, None]
                    assert wt.min() >= rc.ALPHA_DIM and wt.max() <= 256, 'the blur read an entry it never wrote'
                    if case.mask is None:
                        m = np.full((h, w), 255)
                    else:
                        flat_mask = case.mask.reshape(-1)
                        gy, gx = np.meshgrid(np.arange(fy0, fy0 + h), np.arange(fx0, fx0 + w), indexing='ij')
                        m = np.where(flat_mask[f * case.mask_stride + gy * W + gx] != 0, 255, 0)
                    rgb = rc.blend(wt, rgb, m[..., None])
                if case.grid:
                    cy, cx = (oy0, ox0) if defect == 'grid_from_output' else (fy0, fx0)
                    line = ((cx + np.arange(w))[None] % case.grid == 0) | ((cy + np.arange(h))[:, None] % case.grid == 0)
                    rgb[line] = rc.blend(rc.ALPHA_GRID, 255, rgb[line])
                tg, tk, g, ok = tgt[:h, :w], canvas[:h, :w], gt[:h, :w], over[:h, :w]
                rgb[tg == TGT_PATH] = rc.TARGET_PATH
                rgb[tg == TGT_CELL] = rc.TARGET_CELL
                rgb[tk > 0] = rc.TABLES[:60].reshape(20, 3)[case.trail_col[tk[tk > 0]]]
                rgb[g] = rc.blend(rc.ALPHA_GT, 255, rgb[g])
                rgb[ok > 0] = rc.TABLES[:60].reshape(20, 3)[((ok[ok > 0] & 0xFFFFFF) - 1) % 20]
                rgb[ok >> 24 == 3] = rc.GREY
                # stores: one thread per 16 pixels of a row
                for ly in range(h):
                    for lx0 in range(0, w, rc.PX_PER_THREAD):
                        n = min(rc.PX_PER_THREAD, Wo - (ox0 + lx0))
                        dst = ((i * Ho + oy0 + ly) * Wo + ox0 + lx0) * 3
                        flat[dst:dst + 3 * n] = rgb[ly, lx0:lx0 + n].reshape(-1)
                        if defect == 'row_tail_ignores_n' and n < rc.PX_PER_THREAD:
                            spills.append((dst + 3 * n, dst + 3 * rc.PX_PER_THREAD))
    for a, b in spills:                                               # (the zero bytes of the unused pixels land last)
        flat[a:b] = 0
    return flat[:n_out * Ho * Wo * 3].reshape(n_out, Ho, Wo, 3), done


def first_diff(got, want, case):
    d = np.argwhere((got != want).any(-1))
    i, y, x = (int(v) for v in d[0])
    ntx, _, _, chunk, _ = rc.launch(case)
    return (f'{len(d)} pixels differ, first at (frame {i}, y {y}, x {x}), tile {(y // RT) * ntx + x // RT}, run {i // chunk}: '
            f'{got[i, y, x].tolist()}, reference {want[i, y, x].tolist()}')


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_tile_model_equals_the_reference(case):
    got, done = model(case, lists_of(case))
    want = reference_of(case)
    assert done.all()
    assert np.array_equal(got, want), f'{case.route}: {first_diff(got, want, case)}'


def busy_tiles(case):
    """The tiles that hold a trail cell."""
    return [int(t) for t in np.nonzero(np.diff(lists_of(case)[0]))[0]]


CAUGHT_BY = [                                                         # (defect, case, whole output or the tiles with trail cells)
    ('no_resplat', 'runs_110_tiles', False),
    ('cursor_not_carried', 'runs_110_tiles', False),
    ('cursor_not_carried', 'strip_513_tiles', False),
    ('search_lt', 'trails', True),
    ('search_lt', 'runs_110_tiles', False),
    ('dash_from_tile', 'prims', True),
    ('blur_clamped_at_slice', 'prims', True),
    ('blur_clamped_at_slice', 'wo17', True),
    ('round_half_away', 'bg_values', True),
    ('row_tail_ignores_n', 'wo17', True),
    ('row_tail_ignores_n', 'one_column', True),
    ('path_over_cell', 'prims', True),
    ('overlay_without_layer', 'prims', True),
    ('stride_stops_at_256', 'prims', True),
    ('stride_stops_at_256', 'runs_110_tiles', False),
    ('stride_stops_at_256', 'strip_513_tiles', False),
    ('grid_from_output', 'prims', True),
    ('grid_from_output', 'wo80_two_columns', True),
]


def test_every_defect_has_a_case():
    assert {d for d, _, _ in CAUGHT_BY} == set(DEFECTS)


@pytest.mark.parametrize('defect,name,whole', CAUGHT_BY, ids=[f'{d}-{n}' for d, n, _ in CAUGHT_BY])
def test_a_broken_route_is_seen(defect, name, whole):
    case = BY_NAME[name]
    tiles = None if whole else busy_tiles(case)
    want = reference_of(case)
    sound, done = model(case, lists_of(case), None, tiles)
    assert np.array_equal(sound[:, done], want[:, done])
    broken, _ = model(case, lists_of(case), defect, tiles)
    assert not np.array_equal(broken[:, done], want[:, done]), f'{case.route}: the defect {defect} changes no pixel: a case is missing'


def test_the_no_resplat_defect_shows_in_the_first_frame_of_a_later_run():
    case = BY_NAME['runs_110_tiles']
    chunk = rc.launch(case)[3]
    broken, done = model(case, lists_of(case), 'no_resplat', busy_tiles(case))
    differs = [(broken[i][done] != reference_of(case)[i][done]).any() for i in range(len(case.ts))]
    assert chunk == 2 and differs == [False, False, True, True, True]


def test_the_glyph_codes_outside_the_font_draw_nothing():
    case = BY_NAME['prims']
    keep = ~((case.prims[:, 3] == P_GLYPH) & ((case.prims[:, 4] < 0) | (case.prims[:, 4] >= rc.GLYPHS)))
    assert (~keep).sum() == 2
    without = rc.Case('x', case.facts, case.frames, case.mask, case.ts, case.slice, case.grid, case.bg, case.trail, case.trail_col, case.prims[keep])
    assert np.array_equal(rc.reference(without), reference_of(case))
