"""CPU reference, dispatch model and case battery for the masked-grid path-length searches
(axtrack_amd/csrc/path_bfs.hip). No GPU and no product code except transition_cost_table / params (for dmax).

Reference (the definition in the header of path_bfs.hip): on the whole grid, 4- or 8-connected, a move into a cell costs
1 on the mask (mask == 1) and 65536 off it; the optimum is the minimum-cost path and its length its number of cells.
Solved with scipy.sparse.csgraph.dijkstra in f64 from every distinct in-grid source (costs stay far below 2^53: exact):
off = cost // 65536, length = cost % 65536 + off + 1. A pair becomes an arc iff both ends are in the grid,
dx^2 + dy^2 < max_dist^2 and length <= dmax[gap - 1].

Dispatch model: which of the routes of path_bfs.hip decides a pair, restated from its comments and rules (labels in
raster order of the first cell, off-cell fields saturated at 255, best component with a strict <, kv, the ambiguity rule,
the level-0 rule). It only proves what the battery covers (tests/test_pathsearch_cpu.py) and predicts how many sources
the kernels flag (tests/test_pathsearch_gpu.py); it is never the source of an expected value."""
import dataclasses
import functools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components, dijkstra

OFF = 65536
BFS_R, BFS_WW = 250, 18                     # path_bfs.hip: moves of the window, words per window row
LDS_LIMIT = 159 * 1024
MAX_COMP = 64                               # kMaxComp in axt_grid_create
ROUTES = ('tight', 'front_off', 'front_mask', 'plain', 'windowed', 'general')


def lds4(max_gap, cap):
    """`lds4` of axt_masked_distance_table: four window bitmaps and three per-target arrays."""
    return 4 * (2 * BFS_R + 1) * BFS_WW * 4 + max_gap * cap * 8 + 16


def lds3(max_gap, cap):
    return 3 * (2 * BFS_R + 1) * BFS_WW * 4 + max_gap * cap * 6 + 16


@dataclasses.dataclass(eq=False)
class Case:
    """mask u8 [H, W]; frames: per frame a list of (x, y); cap slots per frame (fill: every free slot holds an
    out-of-grid anchor (-1, 0) and count == cap); misses = MCF_MAX_NUM_MISSES (max_gap - 1); env: overrides for the run;
    src_count: rows built per frame (d_src_count of axt_build_arcs) or None; routes: the deciding routes the case is there for;
    named: {name: (tail (t, i), head (t, j), reference length or None for no arc)}."""
    name: str
    mask: np.ndarray
    conn8: bool
    frames: list
    cap: int
    misses: int = 1
    max_dist: int = 500
    env: dict = dataclasses.field(default_factory=dict)
    src_count: list = None
    fill: bool = False
    routes: tuple = ()
    named: dict = dataclasses.field(default_factory=dict)
    source_route: dict = dataclasses.field(default_factory=dict)      # {(t, i): route of the source} claimed by the case

    def __repr__(self):
        return self.name

    @property
    def group(self):
        return self.name[0]

    @property
    def max_gap(self):
        return self.misses + 1

    @property
    def shape(self):
        return self.mask.shape

    @functools.cached_property
    def dmax(self):
        from axtrack_amd import params
        from axtrack_amd.detections import transition_cost_table
        return [int(d) for d in transition_cost_table(dict(params.DEPLOYED, MCF_MAX_NUM_MISSES=self.misses))[1]]

    def arrays(self):
        """(x i32 [F, cap], y i32 [F, cap], count i32 [F]) as the entry points take them."""
        F = len(self.frames)
        x = np.full((F, self.cap), -1 if self.fill else 0, np.int32)
        y = np.zeros((F, self.cap), np.int32)
        cnt = np.zeros(F, np.int32)
        for t, fr in enumerate(self.frames):
            slots = self.slots(t)
            for (px, py), s in zip(fr, slots):
                x[t, s], y[t, s] = px, py
            cnt[t] = self.cap if self.fill else len(fr)
        return x, y, cnt

    def slots(self, t):
        """Slot of every anchor of frame t: in order; with fill, slot 0 and then the LAST slots."""
        n = len(self.frames[t])
        if not self.fill:
            return list(range(n))
        return [0] + list(range(self.cap - n + 1, self.cap)) if n else []

    def offsets(self):
        cnt = self.arrays()[2]
        return np.concatenate([[0], np.cumsum(np.minimum(cnt, self.cap))]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ reference
# (dy, dx): up, down, left, right, then the diagonals; the first 4 are the 4-connected grid (csrc/grid.h states the same)
STEPS8 = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)]


def _edges(H, W, conn8):
    idx = np.arange(H * W).reshape(H, W)
    steps = STEPS8[:8 if conn8 else 4]
    src, dst = [], []
    for dy, dx in steps:
        ys, xs = np.mgrid[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)]
        src.append(idx[ys, xs].ravel())
        dst.append(idx[ys + dy, xs + dx].ravel())
    return np.concatenate(src), np.concatenate(dst)


_GRAPHS, _DIJKSTRA = {}, {}


def _key(mask, conn8):
    return (mask.shape, bool(conn8), mask.tobytes())


def graph(mask, conn8):
    """The grid as a graph: an edge into cell c costs 1 if mask[c] == 1, else 65536."""
    k = _key(mask, conn8)
    if k not in _GRAPHS:
        H, W = mask.shape
        src, dst = _edges(H, W, conn8)
        w = np.where(mask.ravel() == 1, 1.0, float(OFF))
        _GRAPHS[k] = coo_matrix((w[dst], (src, dst)), (H * W, H * W)).tocsr()
    return _GRAPHS[k]


def costs_from(mask, conn8, sx, sy):
    """i64 [H, W]: cost of the minimum-cost path from (sx, sy) to every cell (one Dijkstra per mask and source, cached)."""
    k = _key(mask, conn8) + (int(sx), int(sy))
    if k not in _DIJKSTRA:
        H, W = mask.shape
        cost = dijkstra(graph(mask, conn8), indices=int(sy) * W + int(sx))
        assert np.isfinite(cost).all() and cost.max() < 2.0 ** 52
        cost = cost.astype(np.int64).reshape(H, W)
        cost.setflags(write=False)
        _DIJKSTRA[k] = cost
    return _DIJKSTRA[k]


def lengths_from(mask, conn8, sx, sy):
    """i64 [H, W]: cells of the minimum-cost path from (sx, sy) to every cell."""
    cost = costs_from(mask, conn8, sx, sy)
    return cost % OFF + cost // OFF + 1


def path_length(mask, conn8, sx, sy, tx, ty, max_dist):
    """One pair as hp.path_cost reports it: the length, or max_dist ('None')."""
    H, W = mask.shape
    if not (0 <= sx < W and 0 <= sy < H and 0 <= tx < W and 0 <= ty < H) or (tx - sx) ** 2 + (ty - sy) ** 2 >= max_dist ** 2:
        return max_dist
    L = int(lengths_from(mask, conn8, sx, sy)[ty, tx])
    return L if L <= max_dist else max_dist


def pairs(case):
    """Every (t, i, gap, j) the arc builder looks at: slots below count, rows below src_count."""
    x, y, cnt = case.arrays()
    F = len(cnt)
    for t in range(F):
        n_src = min(int(cnt[t]) if case.src_count is None else int(case.src_count[t]), case.cap)
        for i in (case.slots(t) if case.fill else range(n_src)):
            if i >= n_src:
                continue
            for g in range(1, case.max_gap + 1):
                if t + g >= F:
                    continue
                for j in (case.slots(t + g) if case.fill else range(min(int(cnt[t + g]), case.cap))):
                    yield t, i, g, j


def expected_arcs(case):
    """{(tail, head): (length, gap)} in global numbering (out-of-grid fillers have no arcs: they are left out of `pairs`)."""
    x, y, _ = case.arrays()
    H, W = case.shape
    offs = case.offsets()
    out = {}
    for t, i, g, j in pairs(case):
        sx, sy, tx, ty = int(x[t, i]), int(y[t, i]), int(x[t + g, j]), int(y[t + g, j])
        if not (0 <= sx < W and 0 <= sy < H and 0 <= tx < W and 0 <= ty < H):
            continue
        if (tx - sx) ** 2 + (ty - sy) ** 2 >= case.max_dist ** 2:
            continue
        L = int(lengths_from(case.mask, case.conn8, sx, sy)[ty, tx])
        if L <= case.dmax[g - 1]:
            out[(int(offs[t] + i), int(offs[t + g] + j))] = (L, g)
    return out


# ------------------------------------------------------------------------------------------------ dispatch model
class Fields:
    """What axt_grid_create derives from a mask: labels (raster order of each component's first cell), and per
    component the fewest off-mask cells to every cell, saturated at 255 (None with 0 or more than 64 components)."""

    def __init__(self, mask, conn8):
        H, W = mask.shape
        m = mask == 1
        src, dst = _edges(H, W, conn8)
        on = m.ravel()
        keep = on[src] & on[dst]
        n, lab = connected_components(coo_matrix((np.ones(keep.sum()), (src[keep], dst[keep])), (H * W, H * W)), directed=False)
        lab = np.where(on, lab, -1)
        first = {}
        for c in np.flatnonzero(on):                      # raster order
            first.setdefault(int(lab[c]), len(first) + 1)
        self.label = np.array([first.get(int(v), 0) for v in lab], np.int64).reshape(H, W)
        self.n_comp = len(first)
        self.off = None
        if 1 <= self.n_comp <= MAX_COMP:
            G = graph(mask, conn8)
            self.off = np.empty((self.n_comp, H, W), np.int64)
            for a in range(self.n_comp):
                cost = dijkstra(G, indices=np.flatnonzero(self.label.ravel() == a + 1), min_only=True)
                self.off[a] = np.minimum(cost.astype(np.int64) // OFF, 255).reshape(H, W)
        self.has_fields = self.n_comp == 0 or self.off is not None
        # all-off walks: the graph over the off-mask cells alone
        keep = ~on[src] & ~on[dst]
        self._off_graph = coo_matrix((np.ones(keep.sum()), (src[keep], dst[keep])), (H * W, H * W)).tocsr()
        self._walks = {}
        self.W = W

    def all_off_moves(self, sx, sy):
        """Moves of the shortest walk over off-mask cells from an off-mask source to every cell (inf: none)."""
        if (sx, sy) not in self._walks:
            self._walks[(sx, sy)] = dijkstra(self._off_graph, indices=sy * self.W + sx, unweighted=True)
        return self._walks[(sx, sy)]


_FIELDS = {}


def fields(case):
    k = _key(case.mask, case.conn8)
    if k not in _FIELDS:
        _FIELDS[k] = Fields(case.mask, case.conn8)
    return _FIELDS[k]


@dataclasses.dataclass
class Pair:
    t: int
    i: int
    gap: int
    j: int
    route: str          # one of ROUTES, or 'gate' / 'identical'
    length: int         # reference length (0: an end outside the grid)
    arc: bool
    info: dict


@dataclasses.dataclass
class Model:
    pairs: list
    source_route: dict          # {(t, i): 'tight' | 'two-front' | 'plain'} of the in-grid sources
    source_info: dict           # {(t, i): dict(v=[...], best_comp, best_a)} of the two-front sources
    n_windowed: int             # sources the windowed search is started for
    n_general: int              # sources left for the general search
    off_mode_ok: bool
    n_comp: int


@functools.lru_cache(None)
def model(case):
    f = fields(case)
    x, y, cnt = case.arrays()
    H, W = case.shape
    dm = case.dmax
    nbr = STEPS8[:8 if case.conn8 else 4]
    tight_ok = f.off is not None
    off_mode_ok = tight_ok and lds4(case.max_gap, case.cap) <= LDS_LIMIT and 'AXT_PATH_NO_OFFMODE' not in case.env
    assert (lds4 if off_mode_ok else lds3)(case.max_gap, case.cap) <= LDS_LIMIT
    out, s_route, s_info, flagged = [], {}, {}, set()
    for t, i, g, j in pairs(case):
        sx, sy, tx, ty = int(x[t, i]), int(y[t, i]), int(x[t + g, j]), int(y[t + g, j])
        s_in, t_in = 0 <= sx < W and 0 <= sy < H, 0 <= tx < W and 0 <= ty < H
        if not s_in:
            out.append(Pair(t, i, g, j, 'gate', 0, False, {}))
            continue
        ls = int(f.label[sy, sx])
        sr = 'tight' if tight_ok and ls > 0 else 'two-front' if off_mode_ok and ls == 0 else 'plain'
        s_route[(t, i)] = sr
        if sr == 'two-front' and (t, i) not in s_info:
            best, ba, vs = 0, 1 << 30, [int(f.off[a, sy, sx]) for a in range(f.n_comp)]
            for a, v in enumerate(vs):
                if v < 255 and v - 1 < ba:
                    ba, best = v - 1, a + 1
            s_info[(t, i)] = dict(v=vs, best_comp=best, best_a=ba)
        lim = dm[g - 1]
        dx, dy = abs(tx - sx), abs(ty - sy)
        lower = (max(dx, dy) if case.conn8 else dx + dy) + 1
        if not (t_in and dx * dx + dy * dy < case.max_dist ** 2 and lower <= lim):
            L = int(lengths_from(case.mask, case.conn8, sx, sy)[ty, tx]) if t_in else 0
            out.append(Pair(t, i, g, j, 'gate', L, False, {}))
            continue
        L = int(lengths_from(case.mask, case.conn8, sx, sy)[ty, tx])
        arc = L <= lim
        info = {}
        if dx == 0 and dy == 0:
            route = 'identical'
        elif sr == 'two-front':
            si = s_info[(t, i)]
            best, ba = si['best_comp'], si['best_a']
            kv, amb = 0x7fff, False
            if best > 0:
                ft = int(f.off[best - 1, ty, tx])
                if ft < 255:
                    kv = ba + ft
                for a in range(f.n_comp):
                    fs, fb = si['v'][a], int(f.off[a, ty, tx])
                    if a != best - 1 and fs < 255 and fb < 255 and fs - 1 + fb <= kv:
                        amb = True
            P = f.all_off_moves(sx, sy)[ty * W + tx]
            info = dict(kv=kv, s=P, best_comp=best, best_a=ba)
            route = 'windowed' if amb else 'front_off' if P <= kv else 'front_mask'
        elif sr == 'tight':
            route = 'tight'
        else:
            labs = [ls] if ls else [int(f.label[sy + oy, sx + ox]) for oy, ox in nbr if 0 <= sy + oy < H and 0 <= sx + ox < W]
            lt = int(f.label[ty, tx])
            route = 'plain' if lt != 0 and lt in labs else 'windowed' if f.has_fields else 'general'
        if route in ('windowed', 'general'):
            flagged.add((t, i))
        out.append(Pair(t, i, g, j, route, L, arc, info))
    return Model(out, s_route, s_info, len(flagged) if f.has_fields else 0, 0 if f.has_fields else len(flagged), off_mode_ok, f.n_comp)


# ------------------------------------------------------------------------------------------------ masks
def serpentine(H, W, rows, right_first=True):
    """1-pixel corridors along x on `rows`, consecutive ones joined alternately at the right and the left end."""
    m = np.zeros((H, W), np.uint8)
    for r in rows:
        m[r, :] = 1
    right = right_first
    for a, b in zip(rows, rows[1:]):
        m[a:b + 1, W - 1 if right else 0] = 1
        right = not right
    return m


def _rand(seed, n, H, W, lo=0):
    rng = np.random.default_rng(seed)
    return [(int(a), int(b)) for a, b in zip(rng.integers(lo, W - lo, n), rng.integers(lo, H - lo, n))]


def _row(xs, y):
    return [(int(v), y) for v in xs]


def _pixels(mask, n, y0):
    """n isolated pixels on a 4-cell lattice from row y0 on: n components, 4- and 8-connected."""
    k = 0
    for yy in range(y0, mask.shape[0], 2):
        for xx in range(3, mask.shape[1] - 1, 4):
            if k < n:
                mask[yy, xx] = 1
                k += 1
    assert k == n
    return mask


# ------------------------------------------------------------------------------------------------ the battery
def _serp_frames():
    """Sources on the serpentine (rows 0 and 3 of a 140-wide grid, joined at the right end) and one cell below row 0;
    targets on row 3 whose on-mask lengths straddle 251 / 252 (gap 1) and 86 / 87 (gap 2)."""
    f0 = [(10, 0), (100, 0), (10, 1), (100, 1)]
    f1 = _row(range(14, 27), 3) + [(120, 0), (139, 2)]
    f2 = _row(range(89, 101), 3) + [(130, 3)]
    return [f0, f1, f2]


def _named_serp(conn8):
    """Hand-computed: from (10, 0) to (x, 3) the on-mask path has 272 - x cells 4-connected (129 + 3 + 139 - x moves) and
    270 - x 8-connected (the corners are cut); from (10, 1), one cell off the mask, 273 - x and 270 - x. From (100, 0) to
    (x, 3): 182 - x and 180 - x; from (100, 1): 183 - x and 180 - x. Slots: frame 1 holds x = 14 + j, frame 2 x = 89 + j."""
    if not conn8:
        return {'on_251': ((0, 0), (1, 21 - 14), 251), 'on_252': ((0, 0), (1, 20 - 14), None),
                'on_86': ((0, 1), (2, 96 - 89), 86), 'on_87': ((0, 1), (2, 95 - 89), None),
                'off_251': ((0, 2), (1, 22 - 14), 251), 'off_252': ((0, 2), (1, 21 - 14), None),
                'off_86': ((0, 3), (2, 97 - 89), 86), 'off_87': ((0, 3), (2, 96 - 89), None)}
    return {'on_251': ((0, 0), (1, 19 - 14), 251), 'on_252': ((0, 0), (1, 18 - 14), None),
            'on_86': ((0, 1), (2, 94 - 89), 86), 'on_87': ((0, 1), (2, 93 - 89), None),
            'off_251': ((0, 2), (1, 19 - 14), 251), 'off_252': ((0, 2), (1, 18 - 14), None),
            'off_86': ((0, 3), (2, 94 - 89), 86), 'off_87': ((0, 3), (2, 93 - 89), None)}


def _two_front_mask(H=60, W=130):
    """Component 1: row 3 with a bump over rows 0..3 between x = 60 and x = 100 (a detour); component 2: row 5, straight."""
    m = np.zeros((H, W), np.uint8)
    m[3, :61] = 1
    m[0:4, 60] = 1
    m[0, 60:101] = 1
    m[0:4, 100] = 1
    m[3, 100:] = 1
    m[5, :] = 1
    return m


def _comb_mask(H=10, W=200, pixel=None):
    """Rows 0 and 4 joined at the right end (one component, a long detour); row 8 a component of its own."""
    m = np.zeros((H, W), np.uint8)
    m[0, :] = 1
    m[4, :] = 1
    m[0:5, W - 1] = 1
    m[8, :] = 1
    if pixel:
        m[pixel[1], pixel[0]] = 1
    return m


def _few_field_mask(n_pix, H=16, W=140):
    """The serpentine of cases A plus n_pix isolated pixels: n_pix + 1 components. Rows 5 and 15 hold the values 2 and 255,
    which are off the mask."""
    m = np.zeros((H, W), np.uint8)
    m[:4] = serpentine(4, W, [0, 3])
    _pixels(m, n_pix, 7)
    m[5, :] = 2
    m[15, :] = 255
    return m


@functools.lru_cache(None)
def battery():
    cases = []
    add = cases.append
    # ---------------------------------------------------------------- A: word carries, lengths at the limits
    for c8 in (False, True):
        sfx = '_conn8' if c8 else ''
        serp = serpentine(4, 140, [0, 3])
        add(Case('A_serpentine' + sfx, serp, c8, _serp_frames(), 24, routes=('tight', 'front_mask'), named=_named_serp(c8),
                 source_route={(0, 0): 'tight', (0, 2): 'two-front'}))
        add(Case('A_serpentine_plain' + sfx, serp, c8, _serp_frames(), 24, env={'AXT_PATH_NO_OFFMODE': '1'},
                 routes=('tight', 'plain'), named=_named_serp(c8), source_route={(0, 0): 'tight', (0, 2): 'plain'}))
        # a 1-pixel diagonal staircase across the word boundary at x = 32: one component 8-connected, 60 components 4-connected
        stair = np.zeros((64, 64), np.uint8)
        stair[np.arange(2, 62), np.arange(2, 62)] = 1
        add(Case('A_staircase' + sfx, stair, c8, [[(5, 5), (30, 30), (6, 5), (31, 33)] + _rand(2, 3, 64, 64),
                                                  [(50, 50), (40, 40), (33, 33), (33, 32), (60, 61)] + _rand(3, 4, 64, 64),
                                                  [(61, 61), (45, 45), (31, 31), (20, 21)] + _rand(4, 4, 64, 64)], 12,
                 routes=('tight',) if c8 else ('tight', 'windowed'),
                 named={'stair': ((0, 0), (1, 0), 46 if c8 else 91), 'stair_gap2': ((0, 0), (2, 1), 41 if c8 else 81)}))
        # straight 1-pixel corridors along x: lengths 251 / 252 where the gate decides (lower bound == length)
        line = np.zeros((3, 330), np.uint8)
        line[1, :] = 1
        add(Case('A_corridor' + sfx, line, c8, [[(5, 1), (5, 0), (300, 1)], _row(range(252, 260), 1) + _row((255, 256), 0) + [(40, 1)],
                                                 _row(range(88, 93), 1) + [(310, 2)]], 12, routes=('tight', 'front_mask'),
                 named={'line_251': ((0, 0), (1, 255 - 252), 251), 'line_252': ((0, 0), (1, 256 - 252), None)}))
    # ---------------------------------------------------------------- B: windows
    big = np.zeros((520, 608), np.uint8)
    big[::40, :] = 1
    big[:, 10::90] = 1
    big[250:262, 100:500] = 1
    add(Case('B_window_inside_grid_conn8', big, True, [[(266, 255), (300, 40)], [(20, 10), (500, 500), (266, 6), (515, 255)],
                                                       [(266, 505), (30, 255), (280, 250), (100, 80)]], 6, routes=('tight',)))
    from axtrack_amd import synth
    corr = synth.corridor_mask(300, 420, width=24, pitch=80).astype(np.uint8)
    corr[100:140, :] = 0
    edge = [(0, 0), (419, 0), (0, 299), (419, 299), (200, 0), (200, 299), (0, 150), (419, 150), (7, 90), (282, 60), (281, 200)]
    for c8 in (False, True):
        add(Case('B_corners_edges' + ('_conn8' if c8 else ''), corr, c8,
                 [edge, [(3, 3), (415, 2), (2, 296), (417, 297), (230, 20), (190, 280), (60, 150), (380, 160), (282, 61), (250, 200)],
                  [(40, 10), (400, 30), (10, 260), (390, 270), (200, 60), (281, 100)]], 12, routes=('tight', 'front_mask')))
    for W in (96, 97, 95, 20):
        m = serpentine(20, W, [1, 5, 9, 13, 17])
        m[19, :] = 1                                      # a second component along the bottom edge
        for c8 in (False, True):
            add(Case(f'B_width{W}' + ('_conn8' if c8 else ''), m, c8,
                     [[(0, 1), (W - 1, 17), (W - 1, 0), (W // 2, 3)] + _rand(W, 3, 20, W),
                      [(W - 1, 5), (0, 9), (W - 1, 19), (0, 19), (W - 2, 18)] + _rand(W + 1, 4, 20, W),
                      [(W - 1, 13), (0, 17), (W - 1, 1), (W - 1, 18)] + _rand(W + 2, 4, 20, W)], 9, routes=('tight', 'front_mask')))
    one = np.zeros((1, 40), np.uint8)
    one[0, 5:20] = 1
    one[0, 30:36] = 1
    add(Case('B_one_row', one, False, [[(0, 0), (6, 0), (25, 0), (39, 0)], [(39, 0), (19, 0), (33, 0), (2, 0)], [(31, 0), (0, 0), (22, 0)]], 4,
             routes=('tight', 'front_mask')))
    # ---------------------------------------------------------------- C: a short wall crossing versus a long detour
    for c8 in (False, True):
        add(Case('C_comb' + ('_conn8' if c8 else ''), _comb_mask(), c8,
                 [[(100, 0), (60, 0), (100, 4), (150, 0)] + _row(range(40, 120, 10), 0),
                  [(100, 4), (60, 4), (100, 8), (100, 6), (150, 4), (100, 2)] + _row(range(45, 125, 10), 4),
                  [(160, 4), (170, 4), (100, 8), (150, 6)] + _row(range(150, 190, 8), 4)], 16, routes=('tight',),
                 named={'detour_short': ((0, 0), (1, 0), 201 if c8 else 203), 'detour_long': ((0, 1), (1, 1), None),
                        'other_component': ((0, 2), (1, 2), 5), 'off_the_mask': ((0, 2), (1, 3), 3)}))
    # ---------------------------------------------------------------- D: two-front rules
    for c8 in (False, True):
        tf = _two_front_mask()
        if not c8:      # S0 = (40, 6): a = 0; S1 = (20, 7): a = 1; S40 = (70, 46): a = 40; Stie = (20, 4)
            f1 = [(41, 8), (42, 8), (23, 8), (24, 8), (111, 26), (112, 26), (110, 4), (90, 5), (60, 5), (20, 5)]
        else:
            f1 = [(42, 7), (43, 7), (24, 8), (25, 8), (121, 16), (122, 16), (110, 4), (90, 5), (60, 5), (20, 5)]
        f0 = [(40, 6), (20, 7), (70, 46), (20, 4)]
        # (8-connected, a walk over the mask with one on-mask cell has as many moves as the all-off walk of kv + 1 cells:
        # there the s == kv + 1 pairs pin the rule, the 4-connected ones also the length)
        L = {False: dict(a0=(4, 7), a1=(5, 10), a40=(62, 105), tie=93), True: dict(a0=(3, 4), a1=(5, 6), a40=(52, 53), tie=91)}[c8]
        add(Case('D_two_front' + ('_conn8' if c8 else ''), tf, c8,
                 [f0, f1 + _rand(7, 6, 60, 130), f1[:8] + [(110, 4), (125, 4), (80, 2), (128, 58)] + _rand(8, 6, 60, 130)], 20,
                 routes=('front_off', 'front_mask', 'windowed'),
                 source_route={(0, 0): 'two-front', (0, 1): 'two-front', (0, 2): 'two-front', (0, 3): 'two-front'},
                 named={'a0_s_eq_kv': ((0, 0), (1, 0), L['a0'][0]), 'a0_s_eq_kv_plus_1': ((0, 0), (1, 1), L['a0'][1]),
                        'a1_s_eq_kv': ((0, 1), (1, 2), L['a1'][0]), 'a1_s_eq_kv_plus_1': ((0, 1), (1, 3), L['a1'][1]),
                        'a40_s_eq_kv': ((0, 2), (1, 4), L['a40'][0]), 'a40_s_eq_kv_plus_1': ((0, 2), (1, 5), L['a40'][1]),
                        'tie': ((0, 3), (1, 6), L['tie']), 'a40_mask_front': ((0, 2), (1, 7), 62 if not c8 else 42)}))
        # the window result that must be rejected: rows 0 and 6 are one component, joined by a detour of more than 250 moves;
        # S = (60, 3) touches the pixel (60, 2) (a = 0), from which row 0 is one off-mask cell away (a = 1 for the rows: a
        # tie for every target). T = (60, 6) on row 6: the optimum enters one off-mask cell, (60, 1), and walks the detour;
        # straight down there are 4 cells with two off-mask ones, which a search limited to the window finds
        rej = serpentine(9, 200, [0, 6])
        rej[2, 60] = 1
        frames = [[(60, 3), (90, 3), (61, 4)], [(60, 6), (60, 5), (61, 6), (59, 6), (90, 6), (91, 6), (60, 4), (150, 6), (160, 5)],
                  [(60, 6), (62, 6), (90, 6), (58, 5), (170, 6), (175, 6), (178, 5), (90, 1)]]
        add(Case('D_rejected_window' + ('_conn8' if c8 else ''), rej, c8, frames, 10, routes=('windowed', 'front_mask'),
                 named={'rejected': ((0, 0), (1, 0), None)}))
        add(Case('D_rejected_window_plain' + ('_conn8' if c8 else ''), rej, c8, frames, 10, env={'AXT_PATH_NO_OFFMODE': '1'},
                 routes=('windowed', 'plain'), named={'rejected': ((0, 0), (1, 0), None)}))
    # ---------------------------------------------------------------- E: saturation of the off-cell fields
    sat = np.zeros((6, 620), np.uint8)
    sat[:, :2] = 1
    sat[:, 618:] = 1
    for c8 in (False, True):
        srcs = [(254, 2), (255, 3), (256, 1), (291, 4)]
        f1 = [(sx + d, sy) for sx, sy in srcs for d in (249, 250, 251)] + [(1, 2), (300, 0)]
        f2 = [(sx + d, sy) for sx, sy in srcs for d in (84, 85, 86)] + [(sx - 85, 5 - sy) for sx, sy in srcs]
        add(Case('E_saturation' + ('_conn8' if c8 else ''), sat, c8, [srcs, f1, f2], 16, routes=('front_off',),
                 named={'v253_250_moves': ((0, 0), (1, 1), 251), 'v254_250_moves': ((0, 1), (1, 4), 251),
                        'v255_250_moves': ((0, 2), (1, 7), 251), 'v290_250_moves': ((0, 3), (1, 10), 251),
                        'v255_249_moves': ((0, 2), (1, 6), 250)}))
    # ---------------------------------------------------------------- F: with and without the component fields
    for n_comp in (64, 65):
        for c8 in (False, True):
            m = _few_field_mask(n_comp - 1)
            fr = _serp_frames()
            f0 = fr[0] + [(3, 7), (4, 7), (60, 10), (139, 15)]
            f1 = fr[1] + _row(range(15, 27, 2), 4) + [(7, 7), (3, 9), (20, 5), (10, 15)]
            f2 = fr[2] + _row(range(90, 100, 2), 4) + [(11, 7), (60, 12), (100, 5)]
            add(Case(f'F_{n_comp}_components' + ('_conn8' if c8 else ''), m, c8, [f0, f1, f2], 32,
                     routes=('tight', 'front_mask') if n_comp == 64 else ('plain', 'general'), named=_named_serp(c8),
                     source_route={(0, 0): 'tight' if n_comp == 64 else 'plain', (0, 2): 'two-front' if n_comp == 64 else 'plain'}))
    for c8 in (False, True):
        fr = [_rand(20 + c8, 6, 40, 70) + [(0, 0)], _rand(22 + c8, 7, 40, 70) + [(69, 39)], _rand(24 + c8, 6, 40, 70) + [(0, 0)]]
        add(Case('F_empty_mask' + ('_conn8' if c8 else ''), np.zeros((40, 70), np.uint8), c8, fr, 8, routes=('windowed',)))
        add(Case('F_all_ones_mask' + ('_conn8' if c8 else ''), np.ones((40, 70), np.uint8), c8, fr, 8, routes=('tight',)))
    # ---------------------------------------------------------------- G: the LDS layout at its limit
    # lds4 = 4 * 501 * 18 * 4 + 8 * max_gap * cap + 16 == 159 * 1024 at max_gap = 2, cap = 1157; cap = 1158 takes three bitmaps
    assert lds4(2, 1157) == LDS_LIMIT and lds4(2, 1158) > LDS_LIMIT and lds3(2, 1158) <= LDS_LIMIT
    gfr = [[(10, 1), (100, 0), (10, 0)], [(20, 3), (22, 3), (21, 3)], [(96, 3), (97, 3), (95, 3)]]
    serp = serpentine(4, 140, [0, 3])
    add(Case('G_cap1157_four_bitmaps', serp, False, gfr, 1157, fill=True, routes=('front_mask', 'tight'), source_route={(0, 0): 'two-front'}))
    add(Case('G_cap1158_three_bitmaps', serp, False, gfr, 1158, fill=True, routes=('plain', 'tight'), source_route={(0, 0): 'plain'}))
    add(Case('G_cap8_no_offmode', serp, False, gfr, 8, fill=True, env={'AXT_PATH_NO_OFFMODE': '1'}, routes=('plain', 'tight'),
             source_route={(0, 0): 'plain'}))
    # ---------------------------------------------------------------- H: shapes of the call
    hm = _comb_mask(H=12, W=200)
    hf = [[(100, 0), (60, 1), (100, 4), (-1, 3), (100, 0), (50, 6)], [(100, 4), (100, 0), (60, 1), (200, 3), (3, -1), (3, 12), (150, 4), (50, 6)],
          [], [(100, 8), (100, 0), (60, 1), (61, 1), (150, 8)], [(100, 4), (60, 1), (30, 0), (199, 2)], [(100, 0), (60, 1), (50, 6)]]
    for c8 in (False, True):
        sfx = '_conn8' if c8 else ''
        add(Case('H_max_gap1' + sfx, hm, c8, hf, 8, misses=0, routes=('tight', 'front_mask')))
        add(Case('H_max_gap4' + sfx, hm, c8, hf, 8, misses=3, routes=('tight', 'front_mask')))
        add(Case('H_rows' + sfx, hm, c8, hf, 8, src_count=[2, 0, 0, 5, 1, 3], routes=('tight', 'front_mask')))
        add(Case('H_max_dist120' + sfx, hm, c8, [hf[0] + [(10, 0)], hf[1] + [(125, 0), (135, 0), (180, 4)], hf[3] + [(130, 4), (10, 8)]], 12,
                 max_dist=120, routes=('tight', 'front_mask')))
        m65 = _few_field_mask(64)
        add(Case('H_max_dist120_no_fields' + sfx, m65, c8, [[(10, 0), (100, 0), (10, 1), (60, 10)],
                                                            _row(range(15, 27, 2), 4) + [(120, 0), (125, 4), (7, 7), (135, 4)],
                                                            _row(range(90, 100, 2), 4) + [(11, 7), (130, 4)]], 12, max_dist=120,
                 routes=('plain', 'general')))
    return cases


def case(name):
    return next(c for c in battery() if c.name == name)


# ------------------------------------------------------------------------------------------------ X: the exact search alone
@dataclasses.dataclass(eq=False)
class ExactCase:
    name: str
    mask: np.ndarray
    conn8: bool
    sources: list
    targets: list
    max_dist: int = 500
    named: dict = dataclasses.field(default_factory=dict)     # {name: (i, j, length or None)}

    def __repr__(self):
        return self.name

    def expected(self):
        return np.array([[path_length(self.mask, self.conn8, sx, sy, tx, ty, self.max_dist) for tx, ty in self.targets]
                         for sx, sy in self.sources], np.int32)


@functools.lru_cache(None)
def battery_x():
    cases = []
    # rows 0, 2, 4, 6 of a 7 x 160 grid: from (0, 0) to (x, 6) the on-mask path has 159 * 3 + 6 + (159 - x) moves 4-connected
    serp = serpentine(7, 160, [0, 2, 4, 6])
    for c8 in (False, True):
        # 4-connected: 643 - x cells; 8-connected every turn saves two moves (enter and leave the joining cell diagonally)
        x499 = 643 - 499 if not c8 else 643 - 6 - 499
        cases.append(ExactCase('X_serpentine' + ('_conn8' if c8 else ''), serp, c8, [(0, 0), (1, 1), (-1, 0)],
                               _row((x499, x499 - 1, x499 - 2, x499 + 5), 6) + [(0, 0), (80, 3), (160, 2)],
                               named={'len_499': (0, 0, 499), 'len_500': (0, 1, None), 'len_501': (0, 2, None)}))
        stair = np.zeros((64, 64), np.uint8)
        stair[np.arange(2, 62), np.arange(2, 62)] = 1
        cases.append(ExactCase('X_staircase' + ('_conn8' if c8 else ''), stair, c8, [(5, 5), (6, 5), (30, 30)],
                               [(50, 50), (33, 32), (61, 61), (2, 2), (63, 0)], max_dist=90,
                               named={'stair': (0, 0, 46 if c8 else None)}))
    return cases
