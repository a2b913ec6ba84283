"""Cases for the kernels between the CNN and the solver and behind the solver (detect.hip, the open-grid and table routes of
assoc.hip, ided.hip, metrics.hip, appearance.hip, preproc.hip): the smallest inputs that reach every launch shape, chunk
carry and branch of those kernels, each with the *route facts* it claims and a reference from the project's own oracle
(oracle/oracle.py). Pure numpy, no GPU: tests/test_stagekernels_cpu.py proves that every case reaches the route its facts
name, tests/test_stagekernels_gpu.py runs the kernels on them.

A case is a `Case`: family, name, the facts it claims, and its inputs as attributes. `facts_of(case)` recomputes, from the
inputs and the launch constants below alone, the facts that really hold; a claimed fact that is not among them is an error
of the case, not of the kernel."""
import numpy as np

from oracle import oracle as orc

# ---- launch constants the route facts rest on. A change of launch shape in the source sends you back to the cases. --------
FRAME_CHUNK = 1024          # assoc.hip frame_offsets_kernel (`base += 1024`), ided.hip ided_slot_kernel (`f0 += 1024`)
DET_CHUNK = 1024            # assoc.hip row_ptr_kernel (`base += 1024` over detections)
TARGET_STEP = 64            # assoc.hip arcs_open_kernel (`j0 += 64`: one wave scans 64 targets per step)
ARC_WAVES_PER_FRAME = 8 * 4  # assoc.hip axt_build_arcs `grid_dim(n_frames, 8)` x 256 threads = 4 waves
MAX_GAP_LIMIT = 8           # assoc.hip axt_build_arcs (`max_gap <= 8`, VisParams::mp[8])
OBS_THREADS = 64            # assoc.hip axt_obs_costs launches conf_max_kernel / obs_cost_kernel with 64 threads
PREP_BLOCK_CAP, PREP_THREADS, PREP_VEC = 2048, 256, 8       # preproc.hip axt_preprocess_u16 (`blocks > 256 * 8`), 8 px per lane
PREP_GRID_PIXELS = PREP_BLOCK_CAP * PREP_THREADS * PREP_VEC  # 4 194 304: more pixels than this need the grid-stride loop
LDS_TILES = 28              # detect.hip axt_decode_stitch_nms (`n_tiles > 28` -> decode_stitch_nms_big_kernel)
NMS_THREADS = 256           # detect.hip: 256 threads per frame, survivors compacted 256 at a time
OCC_ROWS, OCC_THREADS, OCC_HEAD = 64, 256, 4                # detect.hip tile_occupancy_kernel / axt_tile_occupancy (`t_head`)
METRICS_CAP, METRICS_MIN_DIST = 2048, 1024                   # metrics.hip axt_detection_confusion (key = d2 << 11 | j)
TILE, S, CELLS = 512, 12, 144


class Case:
    def __init__(self, family, name, facts, **inputs):
        self.family, self.name, self.facts = family, name, tuple(facts)
        self.__dict__.update(inputs)

    def __repr__(self):
        return self.name

    @property
    def route(self):
        return f'{self.family}/{self.name} [{"; ".join(self.facts)}]'


def facts_of(case):
    """The route facts that hold for the case's inputs (a superset of what it claims, if the case is right)."""
    return {name for name, ok in _FACTS[case.family](case).items() if ok}


# =============================================================================================== tile occupancy
OCC_SHAPE = (577, 1030)       # 2 x 3 tiles; last row group is one row; the right-hand tile is 6 px wide


def _occ_frames(case):
    H, W = OCC_SHAPE
    fr = np.full((case.T, H, W), case.fill, np.float32)
    if case.fill_pattern:
        fr.reshape(-1)[1::3] = np.float32(-0.0)
        fr.reshape(-1)[2::3] = np.float32(np.nan)
    for t, yy, xx, v in case.pixels:
        fr[t, yy, xx] = v
    return fr


def _occ_facts(c):
    H, W = OCC_SHAPE
    fr = c.frames()
    pos = fr > 0
    first = [int(np.nonzero(pos[:, yy, xx])[0][0]) for _, yy, xx, _ in c.pixels if pos[:, yy, xx].any()]
    return {
        'H % 64 != 0': H % OCC_ROWS != 0,
        'right tile narrower than the 256 threads': 0 < W % TILE < OCC_THREADS,
        'one launch (T <= 4)': c.T <= OCC_HEAD,
        'second launch runs (T > 4)': c.T > OCC_HEAD,
        'pixel first appears in frame >= 4': bool(first) and min(first) >= OCC_HEAD,
        'pixel in the last row group and the narrow tile': any(yy // OCC_ROWS == (H - 1) // OCC_ROWS and xx // TILE == (W - 1) // TILE
                                                                 for _, yy, xx, _ in c.pixels),
        'pixel on a tile corner': any((yy % TILE, xx % TILE) in ((511, 511), (0, 0)) for _, yy, xx, _ in c.pixels),
        'no positive pixel': not pos.any(),
        'negatives, -0.0 and NaN present': bool((fr < 0).any() and np.isnan(fr).any() and (np.signbit(fr) & (fr == 0)).any()),
        'positive denormal': bool(((fr > 0) & (fr < np.finfo(np.float32).tiny)).any()),
    }


def occupancy_cases():
    H, W = OCC_SHAPE
    base = ['H % 64 != 0', 'right tile narrower than the 256 threads']

    def case(name, T, pixels, facts, fill=0.0, fill_pattern=False):
        c = Case('occupancy', name, base + facts, T=T, pixels=pixels, fill=np.float32(fill), fill_pattern=fill_pattern)
        c.frames = lambda c=c: _occ_frames(c)
        return c

    out = []
    for T in (1, 4, 5):
        out.append(case(f'last_pixel_frame0_T{T}', T, [(0, H - 1, W - 1, 1.0)],
                        ['pixel in the last row group and the narrow tile', 'one launch (T <= 4)' if T <= 4 else 'second launch runs (T > 4)']))
    out.append(case('last_pixel_frame5_T6', 6, [(5, H - 1, W - 1, 1.0)],
                    ['pixel in the last row group and the narrow tile', 'second launch runs (T > 4)', 'pixel first appears in frame >= 4']))
    out.append(case('px_511_511_T4', 4, [(3, 511, 511, 0.25)], ['pixel on a tile corner', 'one launch (T <= 4)']))
    out.append(case('px_512_512_T5', 5, [(4, 512, 512, 0.25)], ['pixel on a tile corner', 'pixel first appears in frame >= 4']))
    out.append(case('non_positive_T5', 5, [], ['no positive pixel', 'negatives, -0.0 and NaN present', 'second launch runs (T > 4)'],
                    fill=-1.5, fill_pattern=True))
    out.append(case('denormal_T5', 5, [(4, 300, 700, np.float32(1e-45))], ['positive denormal', 'pixel first appears in frame >= 4']))
    return out


def occupancy_reference(case):
    """u8 [tile_rows * tile_cols] from orc.kept_tiles."""
    H, W = OCC_SHAPE
    nty, ntx = orc.tile_grid(H, W)
    occ = np.zeros((nty, ntx), np.uint8)
    for iy, ix in orc.kept_tiles(case.frames()):
        occ[iy, ix] = 1
    return occ.reshape(-1)


# =============================================================================================== decode + stitch + NMS
F32_FLOOR = np.float32(0.55)
BELOW_FLOOR = np.nextafter(F32_FLOOR, np.float32(0))


def decode_keep(n_tiles):
    """Kept tiles, row-major on a 16 x 4 tile grid: the first n-1 and the last one, (15, 3)."""
    grid = [(r, c) for r in range(16) for c in range(4)]
    return grid[:n_tiles - 1] + [(15, 3)]


class _Grid:
    """YOLO grids under construction: put(frame, tile, cell, conf, absolute x, absolute y) with offsets that decode exactly."""

    def __init__(self, n_frames, keep):
        self.keep = keep
        self.yolo = np.zeros((n_frames, len(keep), S, S, 3), np.float32)
        self.used = set()
        self.want = {}                      # (frame, tile, cell) -> intended (x, y)

    def raw(self, f, k, cell, conf, x_in, y_in, want):
        assert (f, k, cell) not in self.used, (f, k, cell)
        self.used.add((f, k, cell))
        self.yolo[f, k, cell // S, cell % S] = (conf, x_in, y_in)
        self.want[(f, k, cell)] = want

    def put(self, f, k, cell, conf, ax, ay):
        i, j = cell // S, cell % S
        rx, ry = ax - self.keep[k][1] * TILE, ay - self.keep[k][0] * TILE
        # rel * 3 / 128 - i is exact in f32, and ((x_in + i) * 512) / 12 = rel exactly
        self.raw(f, k, cell, conf, np.float32(rx * 3 / 128 - i), np.float32(ry * 3 / 128 - j), (ax, ay))

    def free_cell(self, f, k, start=0):
        for cell in range(start, CELLS):
            if (f, k, cell) not in self.used:
                return cell
        raise AssertionError('tile full')


NMS_PAIRS = ((23, 0), (21, 9), (13, 19))          # d^2 = 529 (kept), 522 (dropped), 530 (kept)


def _decode_case(n_tiles):
    keep = decode_keep(n_tiles)
    g = _Grid(3, keep)
    A = 0
    B = 1 if n_tiles > 1 else 0
    oy, ox = keep[A][0] * TILE, keep[A][1] * TILE
    facts = ['frame 0 empty', 'conf == thr kept, one ulp below dropped', 'NaN dropped', '+inf ranked first', 'negative coordinates',
             'half-to-even decode', 'equal confidences within 23 px', 'd2 = 529, 522, 530 pairs', 'frames 1 and 2 differ',
             'tile origin (15, 3)']
    # ---- frame 1 -------------------------------------------------------------------------------------------------------
    # half-to-even: (k/4096 + i) * 512 / 12 lands exactly on .5 for i in {0, 3}
    g.raw(1, A, 0 * S + 0, 0.80, 48 / 4096, 144 / 4096, (ox + 0, oy + 2))          # 0.5 -> 0, 1.5 -> 2
    g.raw(1, A, 3 * S + 0, 0.81, 144 / 4096, 48 / 4096, (ox + 130, oy + 0))        # 129.5 -> 130, 0.5 -> 0
    g.raw(1, A, 3 * S + 3, 0.82, 48 / 4096, 144 / 4096, (ox + 128, oy + 130))      # 128.5 -> 128, 129.5 -> 130
    g.raw(1, A, 0 * S + 3, 0.83, 240 / 4096, 48 / 4096, (ox + 2, oy + 128))        # 2.5 -> 2, 128.5 -> 128
    # the threshold and the non-finite confidences
    g.put(1, A, 0 * S + 1, F32_FLOOR, ox + 40, oy + 40)
    g.put(1, A, 0 * S + 2, BELOW_FLOOR, ox + 80, oy + 40)
    g.put(1, A, 1 * S + 1, np.float32(np.nan), ox + 120, oy + 40)
    g.put(1, A, 1 * S + 2, np.float32(np.inf), ox + 160, oy + 40)
    # in-cell offsets below 0 and above 1 (tile-relative coordinates negative; absolute ones too when the tile is (0, 0))
    g.raw(1, A, 1 * S + 0, 0.90, -1.75, -0.5, (ox - 32, oy - 21))                   # (-0.75 * 512/12, -0.5 * 512/12)
    g.raw(1, A, 2 * S + 0, 0.91, 3.25, -1.0, (ox + 224, oy - 43))
    # equal confidences within 23 px: the first in (tile, cell) order survives. The other tile's cell index is LOWER, so a
    # ranking by cell alone keeps the wrong one.
    g.put(1, A, 4 * S + 4, 0.77, ox + 300, oy + 300)
    g.put(1, A, 5 * S + 5, 0.77, ox + 310, oy + 300)
    g.put(1, B, 2 * S + (2 if B != A else 6), 0.77, ox + 300, oy + 312)
    if B != A:
        facts.append('tie across tiles, later tile has the lower cell')
        g.put(1, A, 8 * S + 8, 0.66, ox + 400, oy + 300)             # and a tie whose first member sits in the LATER cell
        g.put(1, B, 1 * S + 1, 0.66, ox + 410, oy + 300)
    # NMS distance boundary: stronger detection at p, weaker at p + d
    for n, (dx, dy) in enumerate(NMS_PAIRS):
        px, py = ox + 100 + 100 * n, oy + 200
        g.put(1, A, 6 * S + 2 * n, 0.95, px, py)
        g.put(1, B, 7 * S + 2 * n, 0.60, px + dx, py + dy)
    # the last kept tile is (15, 3): its origin is the largest the stitch sees
    last = n_tiles - 1
    g.put(1, last, g.free_cell(1, last, 130), 0.88, 3 * TILE + 500, 15 * TILE + 500)
    if n_tiles > 1:
        g.put(1, n_tiles - 2, 143, 0.87, keep[-2][1] * TILE + 17, keep[-2][0] * TILE + 490)
    # ---- frame 2 -------------------------------------------------------------------------------------------------------
    g.put(2, last, 11 * S + 11, 0.93, 3 * TILE + 7, 15 * TILE + 7)
    if n_tiles >= 6:
        facts += ['chain of 432 links over three tiles', 'dependency depth > 256', 'more than 256 survivors']
        # a straight chain, 15 px apart, descending confidence, hosted by ALL cells of tiles 1, 2, 3: link e kills link e + 1
        # (15 < 23) and not link e + 2 (30 >= 23), so 216 survive and link e is decided only after link e - 1. A 15 px chain
        # over 432 cells cannot leave more than 216 survivors: the 144 isolated detections of tile 4 (cell centres, 42.7 px
        # apart) lift the frame past 256, so that the compaction carries a base across its first 256 survivors.
        for e in range(3 * CELLS):
            g.put(2, 1 + e // CELLS, e % CELLS, np.float32(0.99 - 0.001 * e), 20 + 15 * e, 2000)
        for cell in range(CELLS):
            g.raw(2, 4, cell, 0.70, 0.5, 0.5, None)
    else:
        for cell in range(0, CELLS - 1, 2):          # a different frame: every other cell, at its centre
            g.raw(2, 0, cell, np.float32(0.9 - 0.001 * cell), 0.5, 0.5, None)
    facts.append({1: 'n_tiles == 1', LDS_TILES: 'n_tiles == 28 (LDS limit)', LDS_TILES + 1: 'n_tiles == 29 (first HBM size)'}[n_tiles])
    return Case('decode', f'tiles{n_tiles}', facts, yolo=g.yolo, keep=keep, conf_thr=F32_FLOOR, min_dist=23, cap=n_tiles * CELLS + 5,
                want=g.want)


def _decode_zero_case():
    keep = [(0, 1), (2, 3)]
    g = _Grid(3, keep)
    g.raw(1, 0, 5 * S + 5, 0.5, 0.5, 0.5, None)                       # an ordinary detection
    g.raw(1, 1, 0, 0.0, 0.75, 0.0, (3 * TILE + 32, 2 * TILE))         # conf 0 but not all-zero: decodes at its cell (0.75 * 512/12 = 32)
    g.raw(1, 1, 7 * S + 1, -0.0, -0.0, -0.0, None)                    # -0.0 == 0: an all-zero cell
    g.raw(1, 1, 9 * S + 9, -0.25, 0.5, 0.5, None)                     # below a threshold of 0: dropped
    g.raw(2, 0, 11 * S + 11, 0.0, 0.0, 0.5, None)                     # frame 2: one cell of tile 0 not all-zero
    return Case('decode', 'zero_cells_thr0', ['conf_thr == 0: all-zero cells pass', 'all-zero cells decode to the tile origin',
                                              '-0.0 counts as zero', 'frames 1 and 2 differ'],
                yolo=g.yolo, keep=keep, conf_thr=np.float32(0.0), min_dist=23, cap=2 * CELLS + 5, want=g.want)


def decode_cases():
    return [_decode_case(1), _decode_case(LDS_TILES), _decode_case(LDS_TILES + 1), _decode_zero_case()]


# Tiles so far apart that the square of their distance does not fit 32 bits: 128 tiles = 65536 px, whose square is 2^32 (wraps
# to 0); 91 tiles = 46592 px, whose square 2170814464 wraps to a negative number. Either way a 32-bit dx * dx + dy * dy lies
# below 23^2 and the less confident twin dies. (Not part of decode_cases(): tests/test_contract_gpu.py runs them.)
DISTANT_TILES = (128, 91)


def distant_tiles_case(apart, along, n_tiles):
    """Two kept tiles `apart` tile columns (along = 'cols') or rows ('rows') from each other, the other n_tiles - 2 tiles
    empty; in both frames the two tiles hold the same cell with the same in-cell offsets at confidences 0.9 / 0.8 (twins:
    both survive), and tile 0 a pair 21 x 9 px apart that must still lose its weaker member."""
    far = (0, apart) if along == 'cols' else (apart, 0)
    keep = [(0, 0), far] + [(1 + k // 16, 1 + k % 16) for k in range(n_tiles - 2)]
    g = _Grid(2, keep)
    for f in range(2):
        cell = (5 + f) * S + 7
        g.raw(f, 0, cell, 0.9, 0.25, 0.75, None)
        g.raw(f, 1, cell, 0.8, 0.25, 0.75, None)
        g.put(f, 0, 2 * S + 2, 0.95, 100, 100 + f)                      # the genuinely close pair: d^2 = 522 < 529
        g.put(f, 0, 2 * S + 3, 0.60, 121, 109 + f)
    return Case('decode', f'twins_{apart}_{along}_tiles{n_tiles}',
                [f'twins {apart} tile {along} apart', 'close pair inside a tile', f'n_tiles == {n_tiles}'],
                yolo=g.yolo, keep=keep, conf_thr=F32_FLOOR, min_dist=23, cap=n_tiles * CELLS, want=g.want)


def distant_tiles_cases():
    return [distant_tiles_case(apart, along, n) for apart in DISTANT_TILES for along in ('cols', 'rows') for n in (2, LDS_TILES + 1)]


def decode_256_tiles_case():
    """n_tiles == 256 with cap == 256 * 144 exactly: tile indices spread up to (15, 15), the last tile at the largest accepted
    index (32767, 32767), about 300 cells above the threshold per frame (the rank is quadratic in those only)."""
    rng = np.random.default_rng(256)
    keep = [(r, c) for r in range(16) for c in range(16)][:255] + [(32767, 32767)]
    yolo = np.zeros((2, 256, S, S, 3), np.float32)
    for f in range(2):
        for _ in range(300):
            k, i, j = int(rng.integers(0, 256)), int(rng.integers(0, S)), int(rng.integers(0, S))
            yolo[f, k, i, j] = (rng.uniform(0.56, 0.99), rng.uniform(0, 1), rng.uniform(0, 1))
        yolo[f, 255, 11, 11] = (0.93, 0.5, 0.5)
        yolo[f, 255, 11, 10] = (0.71, 0.5, 1.1)                          # 17 px above it: dies
    return Case('decode', 'tiles256', ['n_tiles == 256', 'cap == n_tiles * 144', 'tile index 32767'], yolo=yolo, keep=keep,
                conf_thr=F32_FLOOR, min_dist=23, cap=256 * CELLS, want={})


def decode_reference(case):
    """Per frame (conf f32, x i64, y i64) from the oracle's decode_filter -> stitch -> nms."""
    return [orc.nms(*orc.stitch(orc.decode_filter(y, TILE, S, case.conf_thr), case.keep, TILE), case.min_dist) for y in case.yolo]


def decode_candidates(case, f):
    """Frame f's candidates that pass the threshold, in (tile, cell) order: (conf, x, y, tile, cell) arrays."""
    per = orc.decode_filter(case.yolo[f], TILE, S, case.conf_thr)
    rows = [(c, x + ix * TILE, y + iy * TILE, np.full(len(c), k), cell) for k, ((c, x, y, cell), (iy, ix)) in enumerate(zip(per, case.keep))]
    return tuple(np.concatenate([r[n] for r in rows]) for n in range(5))


def nms_depth(conf, x, y, min_dist=23):
    """Rounds the parallel NMS needs: 1 + the longest chain of undecided earlier neighbours, over the ranked candidates."""
    order = np.argsort(-conf.astype(np.float64), kind='stable')
    x, y = x[order], y[order]
    depth = np.zeros(len(x), np.int64)
    for i in range(len(x)):
        near = (x[:i] - x[i]) ** 2 + (y[:i] - y[i]) ** 2 < min_dist * min_dist
        depth[i] = 1 + (depth[:i][near].max() if near.any() else 0)
    return int(depth.max()) if len(depth) else 0


def _decode_facts(c):
    ref = decode_reference(c)
    y = c.yolo
    cand1 = decode_candidates(c, 1)
    conf1 = y[1, ..., 0]
    surv = {f: set(zip(r[1].tolist(), r[2].tolist())) for f, r in enumerate(ref)}
    out = {
        'frame 0 empty': len(ref[0][0]) == 0,
        'frames 1 and 2 differ': not np.array_equal(y[1].view(np.uint32), y[2].view(np.uint32)) and len(ref[1][0]) != len(ref[2][0]),
        'conf == thr kept, one ulp below dropped': bool((conf1 == c.conf_thr).any() and (conf1 == np.nextafter(c.conf_thr, np.float32(0))).any()
                                                        and (ref[1][0] == c.conf_thr).any()),
        'NaN dropped': bool(np.isnan(conf1).any() and not np.isnan(ref[1][0]).any()),
        '+inf ranked first': len(ref[1][0]) > 0 and np.isposinf(ref[1][0][0]),
        'negative coordinates': bool((cand1[1] - np.array([c.keep[k][1] for k in cand1[3]]) * TILE < 0).any()),
        'tile origin (15, 3)': (15, 3) in c.keep and bool((ref[1][1] >= 3 * TILE).any() and (ref[1][2] >= 15 * TILE).any()),
        'n_tiles == 1': len(c.keep) == 1,
        'n_tiles == 28 (LDS limit)': len(c.keep) == LDS_TILES,
        'n_tiles == 29 (first HBM size)': len(c.keep) == LDS_TILES + 1,
    }
    # half-to-even: a raw value exactly on .5 in f32
    v = ((y[1, ..., 1] + np.arange(S, dtype=np.float32).reshape(1, S, 1)) * np.float32(TILE)) / np.float32(S)
    w = ((y[1, ..., 2] + np.arange(S, dtype=np.float32).reshape(1, 1, S)) * np.float32(TILE)) / np.float32(S)
    half = lambda a: (np.abs(a - np.floor(a)) == 0.5) & (conf1 >= c.conf_thr)
    out['half-to-even decode'] = bool(half(v).any() and half(w).any() and (np.floor(v[half(v)]) % 2 == 0).any()
                                      and (np.floor(v[half(v)]) % 2 == 1).any())
    # ties
    cf, cx, cy, ck, cc = cand1
    tie = tie_cross = False
    for a in range(len(cf)):
        for b in range(a + 1, len(cf)):
            if cf[a] == cf[b] and (cx[a] - cx[b]) ** 2 + (cy[a] - cy[b]) ** 2 < 529:
                tie = True
                tie_cross |= bool(ck[a] != ck[b] and cc[b] < cc[a])
    out['equal confidences within 23 px'] = tie
    out['tie across tiles, later tile has the lower cell'] = tie_cross
    d2 = {int((cx[a] - cx[b]) ** 2 + (cy[a] - cy[b]) ** 2) for a in range(len(cf)) for b in range(len(cf)) if cf[a] > cf[b]}
    out['d2 = 529, 522, 530 pairs'] = {529, 522, 530} <= d2
    f2 = decode_candidates(c, 2)
    chain = f2[2] == 2000
    out['chain of 432 links over three tiles'] = int(chain.sum()) == 3 * CELLS and len(set(f2[3][chain].tolist())) == 3
    out['dependency depth > 256'] = nms_depth(f2[0], f2[1], f2[2]) > NMS_THREADS
    out['more than 256 survivors'] = len(ref[2][0]) > NMS_THREADS
    zero = (y == 0).all(-1)
    out['conf_thr == 0: all-zero cells pass'] = bool(c.conf_thr == 0 and zero[1].any())
    origins = {(ix * TILE, iy * TILE) for iy, ix in c.keep}
    out['all-zero cells decode to the tile origin'] = bool(c.conf_thr == 0) and all(
        origins <= surv[f] and len(r[0]) < CELLS for f, r in enumerate(ref))
    out['-0.0 counts as zero'] = bool((np.signbit(y) & zero[..., None]).any())
    return out


# =============================================================================================== observation costs
def obs_case():
    rng = np.random.default_rng(11)
    F, cap = 4, 200
    count = np.array([0, 1, 130, 200], np.int32)
    conf = np.full((F, cap), 1e9, np.float32)                       # slots beyond count: garbage that would win the maximum
    for t in range(F):
        conf[t, :count[t]] = rng.uniform(0.56, 0.999, count[t]).astype(np.float32)
    conf[1, 0] = F32_FLOOR
    conf[2, 5] = 1.0
    conf[3, 150] = 60.0                                              # the maximum: index >= 64 of the last frame
    return Case('obs', 'counts_0_1_130_200', ['count 0', 'count 1', 'count > 64', 'garbage beyond count', 'maximum at index >= 64 of the last frame',
                                              'upper clamp reached (scale_to_max)', 'lower clamp reached'],
                conf=conf, count=count, max_conf_cost=4.6)


def obs_reference(case, method):
    """f64 [F, cap]: cap_conf + observation_cost over the valid detections of all frames, zero beyond each count."""
    flat = np.concatenate([case.conf[t, :n] for t, n in enumerate(case.count)]).astype(np.float64)
    cost = orc.observation_cost(orc.cap_conf(flat, method), case.max_conf_cost)
    out = np.zeros(case.conf.shape, np.float64)
    o = 0
    for t, n in enumerate(case.count):
        out[t, :n] = cost[o:o + n]
        o += n
    return out


def _obs_facts(c):
    valid = np.arange(c.conf.shape[1])[None] < c.count[:, None]
    mx = np.where(valid, c.conf, -np.inf)
    f, i = np.unravel_index(np.argmax(mx), mx.shape)
    stm, ceil = obs_reference(c, 'scale_to_max'), obs_reference(c, 'ceil')
    return {
        'count 0': bool((c.count == 0).any()), 'count 1': bool((c.count == 1).any()), 'count > 64': bool((c.count > OBS_THREADS).any()),
        'garbage beyond count': bool((c.conf[~valid] > mx.max()).all()),
        'maximum at index >= 64 of the last frame': f == len(c.count) - 1 and i >= OBS_THREADS,
        'upper clamp reached (scale_to_max)': bool((stm[valid] == c.max_conf_cost).any()),
        'lower clamp reached': bool((stm[valid] == -c.max_conf_cost).any() and (ceil[valid] == -c.max_conf_cost).any()),
    }


# =============================================================================================== open-grid arcs
def arc_cost_int_vec(units, kind, a, b):
    """orc.arc_cost_int for integer cost units, vectorised: units << 16 | splitmix64(kind << 60 ^ a << 30 ^ b) & 0xffff."""
    u64 = np.uint64
    with np.errstate(over='ignore'):
        x = (u64(kind) << u64(60)) ^ (np.asarray(a).astype(u64) << u64(30)) ^ np.asarray(b).astype(u64)
        x = x + u64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> u64(27))) * u64(0x94D049BB133111EB)
        x = x ^ (x >> u64(31))
    return np.asarray(units, np.int64) * 65536 + (x & u64(0xFFFF)).astype(np.int64)


class Csr:
    def __init__(self, row_ptr, tail, col, length, gap, cost, offs):
        self.row_ptr, self.tail, self.col, self.length, self.gap, self.cost, self.offs = row_ptr, tail, col, length, gap, cost, offs


def open_grid_csr(x, y, count, H, W, dmax, conn8=False, max_dist=orc.MAX_PX_ASSOC_DIST, units=None, src_count=None,
                  length_table=None):
    """The arcs axt_build_arcs admits on an all-ones mask (or from a table of path lengths), CSR by tail detection in global
    numbering, rows sorted by (gap, head): helpers.open_grid_network for any dmax, conn8, max_dist, units table [max_gap,
    max_dist + 1], src_count (rows only for the first src_count[t] detections of frame t) and length table i16 [F, cap,
    max_gap, cap] (entries <= 0: no path; the in-bounds and euclidean gates belong to whoever filled the table).
    Path lengths as orc.path_matrix (mask=None) gives them, vectorised per frame pair."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    F, cap = x.shape
    cnt = np.minimum(np.asarray(count, np.int64), cap)
    src = cnt if src_count is None else np.minimum(np.asarray(src_count, np.int64), cap)
    offs = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    tails, heads, gaps, lens = [], [], [], []
    for t in range(F):
        na = int(src[t])
        if na == 0:
            continue
        for g in range(1, len(dmax) + 1):
            tb = t + g
            if tb >= F or cnt[tb] == 0:
                continue
            nb, lim = int(cnt[tb]), int(dmax[g - 1])
            if length_table is not None:
                L = np.asarray(length_table[t, :na, g - 1, :nb], np.int64)
                L = np.where(L <= 0, lim + 1, L)
            else:
                xa, ya, xb, yb = x[t, :na, None], y[t, :na, None], x[tb, None, :nb], y[tb, None, :nb]
                dx, dy = np.abs(xa - xb), np.abs(ya - yb)
                L = (np.maximum(dx, dy) if conn8 else dx + dy) + 1
                inb = (xa >= 0) & (xa < W) & (ya >= 0) & (ya < H) & (xb >= 0) & (xb < W) & (yb >= 0) & (yb < H)
                L = np.where((dx * dx + dy * dy < max_dist * max_dist) & (L <= max_dist) & inb, L, max_dist)
            i, j = np.nonzero(L <= lim)
            tails.append(offs[t] + i); heads.append(offs[tb] + j); gaps.append(np.full(len(i), g, np.int64)); lens.append(L[i, j])
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    a, b, g, L = cat(tails), cat(heads), cat(gaps), cat(lens)
    order = np.lexsort((b, g, a))
    a, b, g, L = a[order], b[order], g[order], L[order]
    n = int(offs[-1])
    row_ptr = np.zeros(n + 1, np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(a, minlength=n))
    cost = arc_cost_int_vec(np.asarray(units, np.int64)[g - 1, L], 3, a, b) if units is not None else None
    return Csr(row_ptr, a, b.astype(np.int32), L.astype(np.int16), g.astype(np.uint8), cost, offs)


def transition_units(max_gap, max_dist, miss_rate=0.6):
    """round(orc.transition_cost * 1e6) for D = 0..max_dist and every gap (0 where the cost is infinite): i64 [max_gap, max_dist+1]."""
    D = np.arange(max_dist + 1)
    t = np.stack([orc.transition_cost(D, g, miss_rate, max_px=max_dist) for g in range(1, max_gap + 1)])
    return np.where(np.isfinite(t), np.rint(t * orc.COST_SCALE), 0).astype(np.int64)


def _scatter(rng, F, cap, counts, H, W, outside=0):
    x = rng.integers(0, W, (F, cap)).astype(np.int32)               # slots beyond count: garbage that would make plausible arcs
    y = rng.integers(0, H, (F, cap)).astype(np.int32)
    for t, n in enumerate(counts):
        x[t, :n] = rng.integers(0, W, n)
        y[t, :n] = rng.integers(0, H, n)
    for _ in range(outside):                                          # anchors outside the image: decode does not clamp
        t = int(rng.choice(np.nonzero(np.asarray(counts) > 0)[0]))
        i = int(rng.integers(0, counts[t]))
        x[t, i], y[t, i] = ((-2, 5), (W, 5), (5, -1), (5, H))[int(rng.integers(0, 4))]
    return x, y


def _arc_case(name, facts, **kw):
    kw.setdefault('conn8', False); kw.setdefault('src_count', None); kw.setdefault('length_table', None); kw.setdefault('vis', None)
    return Case('arcs', name, facts, **kw)


def many_frames_case():
    rng = np.random.default_rng(21)
    F, cap, H, W = 1100, 4, 64, 64
    count = rng.integers(0, cap + 1, F).astype(np.int32)
    count[1019:1029] = 0                                              # an empty run across frames 1023 / 1024
    count[500:503] = 0
    count[1029] = 4; count[1018] = 4; count[1099] = 3; count[1097] = 2
    x, y = _scatter(rng, F, cap, count, H, W, outside=12)
    max_dist = 100
    units = 1000 + np.arange(3 * (max_dist + 1), dtype=np.int64).reshape(3, max_dist + 1) * 7      # distinct integers
    return _arc_case('many_frames', ['n_frames > 1024', 'empty frames 1023 and 1024', 'detections after frame 1024', 'n_det > 1024',
                                     'max_gap > 2', 'counts 0..cap', 'detection outside the image', 'units table of distinct integers',
                                     't + g >= n_frames for more than the last two frames'],
                     x=x, y=y, count=count, shape=(H, W), dmax=np.array([40, 30, 20], np.int32), max_dist=max_dist, units=units)


def many_detections_case(conn8=False):
    rng = np.random.default_rng(22)
    F, cap, H, W = 8, 192, 256, 256
    count = np.array([192, 191, 192, 190, 129, 128, 65, 100], np.int32)
    x, y = _scatter(rng, F, cap, count, H, W, outside=6)
    max_dist = 500
    units = (np.arange(1, 3)[:, None] * 100000 + np.arange(max_dist + 1)[None]).astype(np.int64)
    return _arc_case('many_detections' + ('_conn8' if conn8 else ''),
                     ['n_det > 1024', 'several 64-target steps with a partial last one', 'more waves of work than a frame gets',
                      'rows of more than 64 arcs in one gap', 'detection outside the image', 'units table of distinct integers']
                     + (['conn8'] if conn8 else []),
                     x=x, y=y, count=count, shape=(H, W), dmax=np.array([120, 60], np.int32), max_dist=max_dist, units=units, conn8=conn8)


def deep_gaps_case():
    rng = np.random.default_rng(23)
    F, cap, H, W = 6, 6, 64, 64
    count = np.array([6, 3, 0, 5, 1, 6], np.int32)
    x, y = _scatter(rng, F, cap, count, H, W, outside=2)
    max_dist = 120
    return _arc_case('deep_gaps', ['max_gap == 8', 'max_gap > n_frames', 't + g >= n_frames for more than the last two frames',
                                   'detection outside the image', 'small'],
                     x=x, y=y, count=count, shape=(H, W), dmax=np.array([60, 55, 50, 45, 40, 35, 30, 25], np.int32), max_dist=max_dist,
                     units=transition_units(8, max_dist))


def row_subset_cases():
    base = many_detections_case()
    out = []
    for name, lo, hi in (('rows_frames_0_2', 0, 3), ('rows_frames_3_7', 3, 8)):
        src = np.where((np.arange(len(base.count)) >= lo) & (np.arange(len(base.count)) < hi), base.count, 0).astype(np.int32)
        out.append(_arc_case(name, ['src_count: own frames, zeros elsewhere'] + (['n_det > 1024'] if hi == 8 else []), x=base.x, y=base.y, count=base.count,
                             shape=base.shape, dmax=base.dmax, max_dist=base.max_dist, units=base.units, src_count=src))
    src = base.count.copy()
    src[2] = 70; src[7] = 1; src[0] = 0
    out.append(_arc_case('rows_partial_frame', ['src_count below the count of a frame', 'n_det > 1024'], x=base.x, y=base.y,
                         count=base.count, shape=base.shape, dmax=base.dmax, max_dist=base.max_dist, units=base.units, src_count=src))
    return out


def _table_from_open_grid(c, rng, n_edit):
    """A length table as a path cache holds it: the open-grid lengths (0 where there is no path), then n_edit entries of
    every edge value: <= 0, == dmax[g-1], == dmax[g-1] + 1."""
    F, cap = c.x.shape
    G = len(c.dmax)
    H, W = c.shape
    tab = rng.integers(-3, 3 * int(max(c.dmax)), (F, cap, G, cap)).astype(np.int16)        # garbage beyond the counts
    for t in range(F):
        for g in range(1, G + 1):
            if t + g >= F:
                continue
            na, nb = int(c.count[t]), int(c.count[t + g])
            D = orc.path_matrix((None, c.x[t, :na].astype(np.int64), c.y[t, :na].astype(np.int64)),
                                (None, c.x[t + g, :nb].astype(np.int64), c.y[t + g, :nb].astype(np.int64)), H, W, None, c.max_dist, c.conn8)
            if na and nb:
                tab[t, :na, g - 1, :nb] = np.where(D >= c.max_dist, 0, D)
    edits = []
    for t in range(F):
        for g in range(1, G + 1):
            if t + g >= F or not c.count[t] or not c.count[t + g]:
                continue
            for v in (0, -1, int(c.dmax[g - 1]), int(c.dmax[g - 1]) + 1):
                for _ in range(n_edit):
                    i, j = int(rng.integers(0, c.count[t])), int(rng.integers(0, c.count[t + g]))
                    tab[t, i, g - 1, j] = v
                    edits.append((t, i, g, j, v))
    return tab, edits


def length_table_case():
    base = many_detections_case()
    rng = np.random.default_rng(24)
    # the limit of gap 1 EQUALS max_dist: an entry <= 0 must become lim + 1, not max_dist (which that limit would admit)
    max_dist = 120
    c = _arc_case('length_table', ['length table', 'table entries <= 0', 'table entry == dmax', 'table entry == dmax + 1',
                                   'max_dist not above a limit', 'detection outside the image', 'n_det > 1024'],
                  x=base.x.copy(), y=base.y.copy(), count=base.count, shape=base.shape, dmax=np.array([max_dist, 60], np.int32),
                  max_dist=max_dist, units=(np.arange(1, 3)[:, None] * 100000 + np.arange(max_dist + 1)[None]).astype(np.int64))
    c.x[3, 7], c.y[3, 7] = 300, -20                                   # outside the image: the table route has no in-bounds gate
    tab, edits = _table_from_open_grid(c, rng, 3)
    tab[3, 7, :, :5] = 9                                              # ... so these arcs exist
    tab[2, :5, 0, 7] = 11
    c.length_table, c.edits = tab, edits
    return c


def vis_dmax(w, miss_rate, thr, max_gap, max_dist):
    """Largest D per gap whose transition cost with similarity 1 is below thr: the candidate bound of the appearance term."""
    D = np.arange(max_dist + 1)
    out = np.zeros(max_gap, np.int32)
    for g in range(1, max_gap + 1):
        c = orc.transition_cost(D, g, miss_rate, max_px=max_dist, vis_w=w, vis_sim=np.ones(len(D)))
        ok = np.nonzero(c[1:] < thr)[0]
        out[g - 1] = ok.max() + 1 if len(ok) else 0
    return out


VIS = dict(weight=0.3, miss_rate=0.6, thr=0.7)


def _vis_base(name, facts, seed, table):
    rng = np.random.default_rng(seed)
    F, cap, H, W = 5, 80, 256, 256
    count = np.array([70, 80, 66, 0, 75], np.int32)
    x, y = _scatter(rng, F, cap, count, H, W)
    x[0, 0], y[0, 0], x[1, 0], y[1, 0] = 100, 100, 102, 100          # the pair that gets two identical histograms, 2 px apart
    images = (rng.random((F, H, W)) * 0.9).astype(np.float32)
    for t in range(F):                                                # smooth blobs so that nearby crops resemble each other
        yy, xx = np.mgrid[0:H, 0:W]
        images[t] = (0.45 + 0.4 * np.sin(xx / (17.0 + t)) * np.cos(yy / 23.0)).astype(np.float32) * (rng.random((H, W)) < 0.7)
    max_dist = orc.MAX_PX_ASSOC_DIST
    c = _arc_case(name, facts, x=x, y=y, count=count, shape=(H, W), dmax=vis_dmax(VIS['weight'], VIS['miss_rate'], VIS['thr'], 3, max_dist),
                  max_dist=max_dist, units=None, images=images)
    if table:
        c.x[1, 3], c.y[1, 3] = W + 100, H + 100                       # far outside: an empty crop, histogram and sum 0
        tab, edits = _table_from_open_grid(c, rng, 2)
        tab[0, :20, 0, 3] = rng.integers(1, 60, 20)                   # the table admits the detection outside the image
        tab[1, 3, 0, :30] = rng.integers(1, 60, 30)
        c.length_table, c.edits = tab, edits
    hist = np.zeros((F, cap, 180), np.float32)
    for t in range(F):
        n = int(count[t])
        hist[t, :n] = orc.box_histograms(images[t], c.x[t, :n], c.y[t, :n])
    hist[1, 0] = hist[0, 0]                                            # two identical histograms in consecutive frames
    if table:
        c.length_table[0, 0, 0, 0] = 3
    hsum = np.array([[sum(float(v) for v in hist[t, i]) for i in range(cap)] for t in range(F)], np.float64)   # f64, in bin order
    c.vis = dict(VIS, hist=hist, hsum=hsum)
    return c


def vis_cases():
    facts = ['appearance term', 'max_gap > 2', 'nb > 64', 'two identical histograms']
    out = []
    for rows in (False, True):
        c = _vis_base('vis_open' + ('_rows' if rows else ''), facts + (['src_count given'] if rows else ['appearance term, all rows, computed lengths']),
                      31, False)
        if rows:
            c.src_count = c.count.copy()
        out.append(c)
    for rows in (False, True):
        c = _vis_base('vis_table' + ('_rows' if rows else ''), facts + ['length table', 'empty crop: histogram and sum 0', 'table entries <= 0',
                                                                       'appearance term with a length table or src_count']
                      + (['src_count below the count of a frame'] if rows else []), 32, True)
        if rows:
            c.src_count = c.count.copy()
            c.src_count[0] = 40
        out.append(c)
    return out


def vis_csr(case):
    """The arcs with the appearance term: the candidates of open_grid_csr (dmax bounds them), each priced by
    orc.transition_cost with 1 - orc.bhattacharyya of the two histograms and admitted below the threshold. Returns (Csr,
    f64 cost per arc, smallest |cost - thr| over the candidates)."""
    v = case.vis
    H, W = case.shape
    cand = open_grid_csr(case.x, case.y, case.count, H, W, case.dmax, case.conn8, case.max_dist, None, case.src_count, case.length_table)
    offs = cand.offs
    frame_of = lambda k: np.searchsorted(offs, k, 'right') - 1
    ta, tb = frame_of(cand.tail), frame_of(cand.col.astype(np.int64))
    cost = np.zeros(len(cand.col))
    for t in np.unique(ta):
        for u in np.unique(tb[ta == t]):
            m = (ta == t) & (tb == u)
            vs = 1 - orc.bhattacharyya(v['hist'][t, :case.count[t]], v['hist'][u, :case.count[u]])
            i, j = cand.tail[m] - offs[t], cand.col[m] - offs[u]
            cost[m] = orc.transition_cost(cand.length[m].astype(np.int64), int(u - t), v['miss_rate'], max_px=case.max_dist,
                                          vis_w=v['weight'], vis_sim=vs[i, j])
    keep = cost < v['thr']
    margin = float(np.abs(cost - v['thr']).min()) if len(cost) else np.inf
    a, b = cand.tail[keep], cand.col[keep]
    n = int(offs[-1])
    row_ptr = np.zeros(n + 1, np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(a, minlength=n))
    units = np.rint(cost[keep] * orc.COST_SCALE).astype(np.int64)
    return Csr(row_ptr, a, b, cand.length[keep], cand.gap[keep], arc_cost_int_vec(units, 3, a, b), offs), cost[keep], margin


def arc_cases():
    return ([many_frames_case(), many_detections_case(False), many_detections_case(True), deep_gaps_case()] + row_subset_cases()
            + [length_table_case()])


def arcs_reference(case):
    H, W = case.shape
    return open_grid_csr(case.x, case.y, case.count, H, W, case.dmax, case.conn8, case.max_dist, case.units, case.src_count, case.length_table)


def _arc_facts(c):
    F, cap = c.x.shape
    cnt = np.minimum(c.count, cap).astype(np.int64)
    G = len(c.dmax)
    H, W = c.shape
    valid = np.arange(cap)[None] < cnt[:, None]
    ref = vis_csr(c)[0] if c.vis is not None else arcs_reference(c)
    per_gap = np.zeros((int(ref.offs[-1]), G), np.int64)
    np.add.at(per_gap, (ref.tail, ref.gap.astype(np.int64) - 1), 1)
    out = {
        'n_frames > 1024': F > FRAME_CHUNK,
        'empty frames 1023 and 1024': F > FRAME_CHUNK and cnt[FRAME_CHUNK - 1] == 0 and cnt[FRAME_CHUNK] == 0 and cnt[FRAME_CHUNK - 2] == 0,
        'detections after frame 1024': bool(cnt[FRAME_CHUNK:].sum() > 0) and bool((np.diff(ref.row_ptr)[ref.offs[min(FRAME_CHUNK, F)]:] > 0).any()),
        'n_det > 1024': cnt.sum() > DET_CHUNK and bool((np.diff(ref.row_ptr)[DET_CHUNK:] > 0).any()),
        'max_gap > 2': G > 2 and bool((ref.gap > 2).any()),
        'max_gap == 8': G == MAX_GAP_LIMIT and bool((ref.gap >= 5).any()),
        'max_gap > n_frames': G > F,
        'counts 0..cap': set(cnt.tolist()) == set(range(cap + 1)),
        'small': cnt.sum() <= 32,
        'detection outside the image': bool((valid & ((c.x < 0) | (c.x >= W) | (c.y < 0) | (c.y >= H))).any()),
        'units table of distinct integers': c.units is not None and len(np.unique(c.units)) == c.units.size,
        't + g >= n_frames for more than the last two frames': bool((cnt[:max(F - 2, 0)] > 0)[max(F - G, 0):].any()) and G > 2,
        'several 64-target steps with a partial last one': bool(((cnt > 2 * TARGET_STEP) & (cnt % TARGET_STEP != 0)).any()),
        'more waves of work than a frame gets': bool((cnt * G > ARC_WAVES_PER_FRAME).any()),
        'rows of more than 64 arcs in one gap': bool((per_gap > TARGET_STEP).any()),
        'conn8': bool(c.conn8),
        'src_count: own frames, zeros elsewhere': c.src_count is not None and bool(((c.src_count == 0) | (c.src_count == c.count)).all()
                                                                                     and (c.src_count == 0).any() and (c.src_count > 0).any()),
        'src_count below the count of a frame': c.src_count is not None and bool(((c.src_count > 0) & (c.src_count < c.count)).any()),
        'src_count given': c.src_count is not None,
        'length table': c.length_table is not None,
        'max_dist not above a limit': bool((c.max_dist <= np.asarray(c.dmax)).any()),
        'appearance term': c.vis is not None,
        'appearance term, all rows, computed lengths': c.vis is not None and c.src_count is None and c.length_table is None,
        'appearance term with a length table or src_count': c.src_count is not None or (c.vis is not None and c.length_table is not None),
        'nb > 64': bool((cnt[1:] > TARGET_STEP).any()),
    }
    if c.length_table is not None:
        vals = {(g, v) for _, _, g, _, v in c.edits}
        out['table entries <= 0'] = all((g, 0) in vals and (g, -1) in vals for g in range(1, G + 1) if any(e[2] == g for e in c.edits))
        out['table entry == dmax'] = any(v == c.dmax[g - 1] for g, v in vals)
        out['table entry == dmax + 1'] = any(v == c.dmax[g - 1] + 1 for g, v in vals)
    if c.vis is not None:
        h, s = c.vis['hist'], c.vis['hsum']
        out['two identical histograms'] = any(np.array_equal(h[t, i], h[t + 1, j]) and h[t, i].any()
                                              for t in range(F - 1) for i in range(min(cnt[t], 2)) for j in range(min(cnt[t + 1], 2)))
        empty = valid & (s == 0) & ~h.any(-1)
        cand = open_grid_csr(c.x, c.y, c.count, H, W, c.dmax, c.conn8, c.max_dist, None, c.src_count, c.length_table)
        cand_ends = set(cand.tail.tolist()) | set(cand.col.tolist())
        out['empty crop: histogram and sum 0'] = bool(empty.any()) and any(int(ref.offs[t] + i) in cand_ends for t, i in zip(*np.nonzero(empty)))
    return out


# =============================================================================================== identity table
def ided_case(with_map):
    rng = np.random.default_rng(41)
    F, cap = 1100, 3
    n_ids = 40
    count = rng.integers(0, cap + 1, F).astype(np.int32)
    count[1019:1029] = 0                                              # a run of frames without detections across 1023 / 1024
    count[1029] = 3; count[1018] = 3
    count[200:204] = 0
    track = np.full((F, cap), -1, np.int32)
    for t in range(F):
        n = int(count[t])
        ids = rng.choice(n_ids, n, replace=False)
        track[t, :n] = np.where(rng.random(n) < 0.75, ids, -1)
        track[t, n:] = rng.integers(0, n_ids, cap - n)                # valid ids in slots beyond count: must be ignored
    for t in (10, 11, 700, 1030):                                     # detections, but none with an id
        count[t] = max(int(count[t]), 2)
        track[t, :count[t]] = -1
    for t in (20, 900, 1040):                                         # an id >= n_ids next to a valid one
        count[t] = 3
        track[t] = (5, n_ids + 3, 17)
    conf = rng.uniform(0.55, 1, (F, cap)).astype(np.float32)
    x = rng.integers(-50, 5000, (F, cap)).astype(np.int32)
    y = rng.integers(-50, 5000, (F, cap)).astype(np.int32)
    facts = ['n_frames > 1024', 'frames 1023 and 1024 without an id, in a run', 'frame with detections but no id', 'valid ids beyond count',
             'ids >= n_ids']
    id_row = n_rows = None
    if with_map:
        # rows only for the ids of the cache: every third id has none (-1), the others are numbered without gaps
        id_row = np.full(n_ids, -1, np.int32)
        kept = [i for i in range(n_ids) if i % 3 != 1]
        id_row[kept] = np.arange(len(kept))
        n_rows = len(kept)
        # a frame whose ONLY ids are filtered out counts as a frame with ids in the kernel's quirk labels: not built here
        for t in range(F):
            ids = track[t, :count[t]]
            if (ids >= 0).any() and not ((ids >= 0) & (ids < n_ids) & (id_row[np.clip(ids, 0, n_ids - 1)] >= 0)).any():
                track[t, :count[t]] = -1
        facts.append('id_row map with gaps and -1 entries')
    else:
        for t in range(F):                                            # likewise for a frame whose only id is >= n_ids
            ids = track[t, :count[t]]
            assert not ((ids >= n_ids).any() and not ((ids >= 0) & (ids < n_ids)).any())
    return Case('ided', 'map' if with_map else 'identity', facts, track=track, conf=conf, x=x, y=y, count=count, n_ids=n_ids,
                id_row=id_row, n_rows=n_rows)


def ided_cases():
    return [ided_case(False), ided_case(True)]


def ided_tables_of(case):
    """Per frame the sorted rows (row id, conf, x, y) that orc.ided_dets_all takes."""
    tables = []
    for t in range(len(case.count)):
        rows = []
        for k in range(int(case.count[t])):
            i = int(case.track[t, k])
            if i < 0 or i >= case.n_ids:
                continue
            r = i if case.id_row is None else int(case.id_row[i])
            if r >= 0:
                rows.append((r, float(case.conf[t, k]), int(case.x[t, k]), int(case.y[t, k])))
        tables.append(sorted(rows))
    return tables


def ided_reference(case, quirk):
    """f64 [n_rows, 3F] with numpy's NaN: orc.ided_dets_all. Every row id 0..n_rows-1 occurs, so its rows are the kernel's."""
    ids, _, _, vals = orc.ided_dets_all(ided_tables_of(case), quirk)
    n_rows = case.n_ids if case.n_rows is None else case.n_rows
    assert ids == list(range(n_rows))
    return vals


def _ided_facts(c):
    F = len(c.count)
    tabs = ided_tables_of(c)
    has = np.array([len(p) > 0 for p in tabs])
    valid = np.arange(c.track.shape[1])[None] < c.count[:, None]
    return {
        'n_frames > 1024': F > FRAME_CHUNK and bool(has[FRAME_CHUNK:].any()) and bool((~has[:FRAME_CHUNK]).any()),
        'frames 1023 and 1024 without an id, in a run': not has[FRAME_CHUNK - 3:FRAME_CHUNK + 3].any(),
        'frame with detections but no id': bool(((c.count > 0) & ~has).any()),
        'valid ids beyond count': bool((~valid & (c.track >= 0) & (c.track < c.n_ids)).any()),
        'ids >= n_ids': bool((valid & (c.track >= c.n_ids)).any()),
        'id_row map with gaps and -1 entries': c.id_row is not None and bool((c.id_row < 0).any())
                                               and bool((valid & (c.track >= 0) & (c.track < c.n_ids) & (c.id_row[np.clip(c.track, 0, c.n_ids - 1)] < 0)).any()),
    }


# =============================================================================================== detection metrics
F32_VS_F64 = (0.59, 0.63, 0.7, 0.67, 0.55)


def metrics_cases():
    thrs = orc.all_conf_thrs()
    F, cap, gcap = 3, METRICS_CAP, 50
    rng = np.random.default_rng(51)

    def blank():
        return (rng.uniform(0.9, 1.0, (F, cap)).astype(np.float32), rng.integers(-9999, 9999, (F, cap)).astype(np.int32),
                rng.integers(-9999, 9999, (F, cap)).astype(np.int32), np.zeros(F, np.int32),
                rng.integers(-9999, 9999, (F, gcap)).astype(np.int32), rng.integers(-9999, 9999, (F, gcap)).astype(np.int32), np.zeros(F, np.int32))

    # ---- min_dist = 23
    conf, x, y, count, gx, gy, gcount = blank()
    # frame 0: 2048 detections on a 30 px lattice, descending confidence; index 2047 is the only match of label 0
    k = np.arange(cap)
    count[0] = cap
    x[0], y[0] = 30 * (k % 64), 30 * (k // 64)
    conf[0] = np.linspace(0.99, 0.56, cap).astype(np.float32)
    conf[0, 2047] = 0.8
    lab = [(x[0, 2047] + 9, y[0, 2047] + 12)]                          # 15 px from detection 2047, > 23 px from every other one
    lab += [(x[0, j] + 3, y[0, j] - 4) for j in (0, 63, 64, 1000, 2046)]
    lab += [(15, 15), (5000, 5000)]                                   # 21.2 px from four lattice points (ties in d2); no match at all
    gcount[0] = len(lab)
    gx[0, :len(lab)], gy[0, :len(lab)] = zip(*lab)
    # frame 1: crafted ties and thresholds
    count[1] = 100
    x[1, :100], y[1, :100] = 3000 + 40 * np.arange(100), 3000                         # far from everything
    conf[1, :100] = 0.9
    x[1, 3], y[1, 3], x[1, 70], y[1, 70] = 110, 100, 100, 110                         # equal d2 = 100 at j = 3 and j = 70 (lanes 3 and 6)
    conf[1, 70] = 0.95                                                                # the later one is the more confident: still j = 3
    x[1, 10], y[1, 10] = 500, 500                                                     # two labels share this closest detection
    x[1, 11], y[1, 11] = 512, 500                                                     # ... the second one's second choice
    # f32 confidence against the f64 threshold of the same decimal: f32(0.59), f32(0.63) and f32(0.7) lie BELOW theirs (not above
    # it), f32(0.67) and f32(0.55) above
    for n, c32 in enumerate(F32_VS_F64):
        x[1, 20 + n], y[1, 20 + n], conf[1, 20 + n] = 1000 + 100 * n, 1000, np.float32(c32)
    lab = [(100, 100), (498, 500), (503, 500)] + [(1000 + 100 * n, 1001) for n in range(len(F32_VS_F64))]
    gcount[1] = len(lab)
    gx[1, :len(lab)], gy[1, :len(lab)] = zip(*lab)
    # frame 2: no detections, labels (one at the phantom detection's origin)
    gcount[2] = 3
    gx[2, :3], gy[2, :3] = (0, 10, 900), (0, 10, 900)
    a = Case('metrics', 'min_dist_23', ['count == cap == 2048', 'index 2047 is a label\'s only match', 'equal d2 at j = 3 and j = 70',
                                        'ties in d2 across lanes', 'two labels share their closest detection', 'detections empty',
                                        'f32 confidences below (0.59, 0.63, 0.7) and above (0.67, 0.55) their f64 thresholds'],
             conf=conf, x=x, y=y, count=count, gx=gx, gy=gy, gcount=gcount, thrs=thrs, min_dist=23)
    # ---- min_dist = 1024
    conf, x, y, count, gx, gy, gcount = blank()
    count[0] = 70
    x[0, :70], y[0, :70] = 20000 + 3000 * np.arange(70), 20000
    x[0, 69], y[0, 69] = 1023 + 100, 45 + 100                         # d2 = 1 048 554 from label 0, at j = 69
    x[0, 5], y[0, 5] = 1024 + 100, 100 + 3000                         # d2 = 1 048 576 from label 1: not a candidate
    lab = [(100, 100), (100, 3100)]
    gcount[0] = 2
    gx[0, :2], gy[0, :2] = zip(*lab)
    count[1] = 5                                                      # frame 1: detections, no labels (a phantom label at the origin)
    x[1, :5], y[1, :5] = (700, 30, 5000, 1, 900), (700, 40, 5000, 1, 200)
    b = Case('metrics', 'min_dist_1024', ['min_dist == 1024', 'd2 = 1 048 554 at j > 63', 'd2 == min_dist^2 excluded', 'labels empty', 'both sides empty'],
             conf=conf, x=x, y=y, count=count, gx=gx, gy=gy, gcount=gcount, thrs=thrs, min_dist=METRICS_MIN_DIST)
    return [a, b]


def metrics_frame(case, t):
    n, m = int(case.count[t]), int(case.gcount[t])
    return (case.conf[t, :n], case.x[t, :n], case.y[t, :n]), case.gx[t, :m], case.gy[t, :m]


def metrics_reference(case, k_mask):
    """(confusion i64 [F, 3, n_thr], fp mask u8 [F, cap], fn mask u8 [F, gcap]) from orc.detection_confusion, zero beyond the counts."""
    F, cap = case.x.shape
    cm = np.zeros((F, 3, len(case.thrs)), np.int64)
    fp, fn = np.zeros((F, cap), np.uint8), np.zeros((F, case.gx.shape[1]), np.uint8)
    for t in range(F):
        det, gx, gy = metrics_frame(case, t)
        cm[t] = orc.detection_confusion(det, gx, gy, case.thrs, case.min_dist)
        if k_mask >= 0:
            a, b = orc.detection_confusion(det, gx, gy, case.thrs, case.min_dist, return_masks_at=k_mask)
            fp[t, :len(det[0])] = a[:len(det[0])]                     # (the phantom row of an empty side has no slot)
            fn[t, :len(gx)] = b[:len(gx)]
    return cm, fp, fn


def _metrics_facts(c):
    F, cap = c.x.shape
    out = {'count == cap == 2048': cap == METRICS_CAP and bool((c.count == cap).any()), 'min_dist == 1024': c.min_dist == METRICS_MIN_DIST,
           'detections empty': bool(((c.count == 0) & (c.gcount > 0)).any()), 'labels empty': bool(((c.count > 0) & (c.gcount == 0)).any()),
           'both sides empty': bool(((c.count == 0) & (c.gcount == 0)).any())}
    only_last = tie_3_70 = tie_lanes = shared = big = excluded = False
    m2 = c.min_dist ** 2
    for t in range(F):
        (cf, x, y), gx, gy = metrics_frame(c, t)
        if not len(cf) or not len(gx):
            continue
        d2 = (gx[:, None].astype(np.int64) - x[None]) ** 2 + (gy[:, None].astype(np.int64) - y[None]) ** 2
        best = []
        for i in range(len(gx)):
            cand = np.nonzero(d2[i] < m2)[0]
            if len(cand) == 1 and cand[0] == METRICS_CAP - 1:
                only_last = True
            if len(cand):
                mn = d2[i][cand].min()
                at = cand[d2[i][cand] == mn]
                tie_3_70 |= at.tolist() == [3, 70]
                tie_lanes |= len(at) > 1 and len(set((at % 64).tolist())) > 1
                best.append(int(at[0]))
                big |= bool(mn == 1048554 and at[0] > 63)
            excluded |= bool((d2[i] == m2).any())
        shared |= len(best) != len(set(best))
    out.update({"index 2047 is a label's only match": only_last, 'equal d2 at j = 3 and j = 70': tie_3_70, 'ties in d2 across lanes': tie_lanes,
                'two labels share their closest detection': shared, 'd2 = 1 048 554 at j > 63': big, 'd2 == min_dist^2 excluded': excluded})
    f = lambda v: float(np.float32(v))
    have = set(np.concatenate([c.conf[t, :c.count[t]] for t in range(F)]).tolist()) if c.count.sum() else set()
    out['f32 confidences below (0.59, 0.63, 0.7) and above (0.67, 0.55) their f64 thresholds'] = (
        f(0.59) < 0.59 and f(0.63) < 0.63 and f(0.7) < 0.7 and f(0.67) > 0.67 and f(0.55) > 0.55 and {f(v) for v in F32_VS_F64} <= have
        and set(F32_VS_F64) <= set(c.thrs.tolist()))
    return out


# =============================================================================================== box histograms
HIST_SHAPE = (200, 260)


def hist_cases():
    H, W = HIST_SHAPE
    out = []
    for box in (1, 7, 70, 301):
        rng = np.random.default_rng(60 + box)
        F, cap = 2, 12
        frames = (rng.random((F + 1, H, W)) * 1.3).astype(np.float32)            # detection frame f is shown frame f + 1
        frames[rng.random(frames.shape) < 0.5] = 0
        frames[:, 60:70, 50:60] = (np.arange(10) / 180).astype(np.float32)[None, None, :]     # bin boundaries
        x = rng.integers(-40, W + 40, (F, cap)).astype(np.int32)
        y = rng.integers(-40, H + 40, (F, cap)).astype(np.int32)
        x[0, :5], y[0, :5] = (0, W - 1, 0, W - 1, W + 400), (0, 0, H - 1, H - 1, H + 400)      # corners; far outside (empty crop)
        count = np.array([cap, 7], np.int32)
        facts = [f'box == {box}', 'empty crop', 'crop clipped at every edge']
        if box == 70:
            # every pixel of the crop outside [0, 1): all bins 0, mn == mx == 0
            frames[1, 100:170, 100:170] = np.where(rng.random((70, 70)) < 0.5, 1.0, -0.25).astype(np.float32)
            x[0, 5], y[0, 5] = 135, 135
            # a 3 x 60 crop at the bottom-right corner with one pixel in every bin: mn == mx == 1
            frames[1, H - 3:, W - 60:] = ((np.arange(180) + 0.5) / 180).astype(np.float32).reshape(3, 60)
            x[0, 6], y[0, 6] = W - 60 + 35, H - 3 + 35
            facts += ['mn == mx == 0', 'mn == mx > 0']
        out.append(Case('hist', f'box{box}', facts, frames=frames, x=x, y=y, count=count, box=box, t_offset=1))
    return out


def hist_reference(case):
    """(hist f32 [F, cap, 180], bin sums f64 [F, cap]) from orc.box_histograms, zero beyond the counts."""
    F, cap = case.x.shape
    hist, hsum = np.zeros((F, cap, 180), np.float32), np.zeros((F, cap), np.float64)
    for f in range(F):
        n = int(case.count[f])
        hist[f, :n] = orc.box_histograms(case.frames[f + case.t_offset], case.x[f, :n], case.y[f, :n], case.box)
        hsum[f, :n] = [sum(float(v) for v in r) for r in hist[f, :n]]             # f64, in bin order
    return hist, hsum


def hist_crops(case):
    """Per valid detection (f, i): the crop feature_model takes."""
    H, W = HIST_SHAPE
    for f in range(len(case.count)):
        for i in range(int(case.count[f])):
            r0, c0 = max(int(case.y[f, i]) - case.box // 2, 0), max(int(case.x[f, i]) - case.box // 2, 0)
            yield f, i, case.frames[f + case.t_offset][r0:min(r0 + case.box, H), c0:min(c0 + case.box, W)]


def _hist_facts(c):
    H, W = HIST_SHAPE
    out = {f'box == {c.box}': True, 'empty crop': False, 'mn == mx == 0': False, 'mn == mx > 0': False}
    clipped = set()
    for f, i, crop in hist_crops(c):
        out['empty crop'] |= crop.size == 0
        idx = np.floor(crop.astype(np.float64) * 180.0)
        bins = np.bincount(idx[(idx >= 0) & (idx < 180)].astype(np.int64), minlength=180)
        out['mn == mx == 0'] |= crop.size > 0 and bins.max() == 0
        out['mn == mx > 0'] |= bins.min() == bins.max() > 0 and crop.size == 180
        clipped |= {n for n, hit in enumerate((c.y[f, i] - c.box // 2 < 0, c.x[f, i] - c.box // 2 < 0,
                                               0 < H - (c.y[f, i] - c.box // 2) < c.box, 0 < W - (c.x[f, i] - c.box // 2) < c.box)) if hit}
    out['crop clipped at every edge'] = clipped == {0, 1, 2, 3} or c.box == 1 and {0, 1} <= clipped
    return out


# =============================================================================================== preprocess
PREP_INV = np.float32(1. / 65535)
PREP_RAW_OFFSET, PREP_RAW_CLIP = 121, 176
PREP_OFFSET = float(np.float32(PREP_RAW_OFFSET) * PREP_INV)                       # the float of raw 121: x - offset == 0 exactly
PREP_CLIP = float(np.float32(np.float32(PREP_RAW_CLIP) * PREP_INV) - np.float32(PREP_OFFSET))    # raw 176 lands exactly on clip
PREP_SCALE = 0.015176106


def _prep_raw(shape, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 5000, shape).astype(np.uint16)
    raw[rng.random(shape) < 0.7] = 0
    special = np.array([0, 1, 65535, PREP_RAW_OFFSET, PREP_RAW_CLIP, PREP_RAW_OFFSET + 1, PREP_RAW_CLIP - 1, PREP_RAW_CLIP + 1], np.uint16)
    flat = raw.reshape(-1)
    n = len(flat)
    reps = np.resize(special, min(n, 24))
    flat[:len(reps)] = reps                                           # the first lanes ...
    flat[n - len(reps):] = reps[::-1]                                 # ... and the tail
    return raw


def prep_cases():
    out = []
    for shape, masked, log, facts in (
            ((3, 37, 45), True, True, ['frame_px % 8 != 0', 'n_px % 8 != 0: a tail shorter than 8', 'mask', 'out= slice of a larger buffer']),
            ((1, 1, 5), False, True, ['frame_px % 8 != 0', 'n_px < 8']),
            ((17, 512, 512), False, False, ['frame_px % 8 == 0', 'grid-stride loop (n_px > 2048 * 256 * 8)']),
            ((17, 511, 513), True, True, ['frame_px % 8 != 0', 'n_px % 8 != 0: a tail shorter than 8', 'mask',
                                          'grid-stride loop (n_px > 2048 * 256 * 8)'])):
        raw = _prep_raw(shape, 70 + shape[1])
        mask = None
        if masked:
            yy, xx = np.mgrid[0:shape[1], 0:shape[2]]
            mask = ((yy // 3 + xx // 5) % 4 != 0)
            mask.reshape(-1)[:24] = True                               # the special values stay visible ...
            mask.reshape(-1)[-24:] = True
            mask.reshape(-1)[5] = False                                # ... but one
        name = 'x'.join(map(str, shape))
        for lg in ((log, not log) if shape[0] * shape[1] * shape[2] < 100000 else (log,)):
            out.append(Case('prep', f'{name}_{"log" if lg else "nolog"}', facts + (['log'] if lg else ['no log']), raw=raw, mask=mask, log=lg,
                            offset=PREP_OFFSET, clip=PREP_CLIP, scale=PREP_SCALE, out_slice='out= slice of a larger buffer' in facts))
    return out


def prep_reference(case):
    return orc.preprocess(case.raw, case.mask, case.offset, case.clip, case.log, case.scale)


def prep_prelog(case):
    """The f32 value the clip comparison sees, per pixel (orc.preprocess up to the clip)."""
    x = np.multiply(case.raw, 1. / 65535, dtype=np.float32)
    if case.mask is not None:
        x[:, ~case.mask] = 0
    x -= np.float32(case.offset)
    x[x < 0] = 0
    return x


def _prep_facts(c):
    T, H, W = c.raw.shape
    n, fp = T * H * W, H * W
    vals = set(np.unique(c.raw).tolist())
    return {
        'frame_px % 8 != 0': fp % PREP_VEC != 0, 'frame_px % 8 == 0': fp % PREP_VEC == 0,
        'n_px % 8 != 0: a tail shorter than 8': n % PREP_VEC != 0 and n > PREP_VEC, 'n_px < 8': n < PREP_VEC,
        'grid-stride loop (n_px > 2048 * 256 * 8)': n > PREP_GRID_PIXELS,
        'mask': c.mask is not None and bool((~c.mask).any() and c.mask.any()),
        'log': bool(c.log), 'no log': not c.log, 'out= slice of a larger buffer': bool(c.out_slice),
        'special raw values': {0, 1, 65535, PREP_RAW_OFFSET, PREP_RAW_CLIP} <= vals,
    }


_FACTS = {'occupancy': _occ_facts, 'decode': _decode_facts, 'obs': _obs_facts, 'arcs': _arc_facts, 'ided': _ided_facts,
          'metrics': _metrics_facts, 'hist': _hist_facts, 'prep': _prep_facts}


def all_cases():
    return (occupancy_cases() + decode_cases() + [obs_case()] + arc_cases() + vis_cases() + ided_cases() + metrics_cases() + hist_cases()
            + prep_cases())
