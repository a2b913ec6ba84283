"""CPU reference, dispatch model and case battery for the axon-reconstruction kernels (axtrack_amd/csrc/recon.hip):
axt_track_links, axt_link_paths and axt_link_cells. numpy / scipy only; no product code.

Reference. The path of a link is the one csrc/grid.h defines: on the whole grid a move into a cell costs 1 on the mask and
65536 off it; the Dijkstra of tests/pathsearch_reference.py (f64, exact) gives every cell's cost, hence its key (off-mask
cells entered, moves); the walk back from the target steps to the FIRST neighbour in STEPS8 order whose cost is the
current cost minus the current cell's weight. The all-ones grid has the closed-form staircase. The links of a track
table, the CSR cells and the interpolation anchors are restated from the header of recon.hip.

Dispatch model (stage_model / route): which stage of axt_link_paths decides a link, restated once from recon.hip. It also
carries every stage's own way to the cells (the breadth-first distance field, the window keys and their certificate), so
that tests/test_recon_routes_cpu.py can show (a) that the stages, as documented, give the reference's cells on every pair
of the battery and (b) that each stage with one rule broken does not. It is never the source of an expected value: what
the kernels must return is always the reference.

  classifier   outside the grid or dx^2 + dy^2 >= max_dist^2 -> 'gate' (none). S == T -> pending. Target off the mask, or
               source on the mask with another label than the target -> exact-pending. Otherwise pending.
  bfs R        (31, then 127; pending links) limit = min(R, max_dist - 2). d = breadth-first distance S -> T over on-mask
               cells (S itself may be off the mask). d <= limit: decided, d + 1 cells. Otherwise, with limit == max_dist - 2
               and S on the mask: decided, none. Otherwise passed on; radius 127 passes on to exact-pending.
  key R        (31, then 63; exact-pending links; only with 1 .. 64 components) cheb(S, T) > R: passed on. (o, m) = optimum
               of the search confined to the window of radius R around S, clipped to the grid. Accepted iff m <= R and
               o == lb; lb = d_off[label(S)][T] for a source on the mask, else min(metric distance,
               min_A d_off[A][S] - 1 + d_off[A][T]). Accepted: m + 1 cells, or none if m + 1 >= max_dist.
  exact        everything left."""
import collections
import dataclasses
import functools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import dijkstra

import pathsearch_reference as pr
from pathsearch_reference import OFF, STEPS8, costs_from, graph

ROUTES = ('gate', 'bfs31', 'bfs127', 'key31', 'key63', 'exact')
MAX_COMP = 64                       # components up to which axt_grid_create keeps the off-cell fields
EMIT_CHUNK = 256                    # LT of links_emit_kernel
BROKEN = ('diagonals_first', 'no_o_eq_lb', 'no_m_le_R', 'rule_for_off_source', 'limit_R')


# ------------------------------------------------------------------------------------------------ reference: paths
def _in_gate(H, W, sx, sy, tx, ty, max_dist):
    """The gate of axt_path_cost: end points inside the grid and dx^2 + dy^2 < max_dist^2."""
    return (0 <= sx < W and 0 <= sy < H and 0 <= tx < W and 0 <= ty < H
            and (tx - sx) ** 2 + (ty - sy) ** 2 < max_dist ** 2)


def _walk(cost, weight, sx, sy, tx, ty, order, x0=0, y0=0, W=None):
    """Walk back over a cost field [h, w] from (tx, ty) to (sx, sy) (field coordinates): at each cell to the first
    neighbour in `order` whose cost is the cell's cost minus weight(cell). Cells y*W + x in grid coordinates, source first."""
    h, w = cost.shape
    cy, cx = ty, tx
    out = [(y0 + cy) * W + x0 + cx]
    while (cx, cy) != (sx, sy):
        want = cost[cy, cx] - weight(cy, cx)
        for dy, dx in order:
            ny, nx = cy + dy, cx + dx
            if 0 <= ny < h and 0 <= nx < w and cost[ny, nx] == want:
                cy, cx = ny, nx
                break
        else:
            raise AssertionError('no neighbour continues an optimal path')
        out.append((y0 + cy) * W + x0 + cx)
        assert len(out) <= h * w
    return np.array(out[::-1], np.int64)


def _order(conn8, diagonals_first=False):
    if not conn8:
        return STEPS8[:4]
    return STEPS8[4:] + STEPS8[:4] if diagonals_first else STEPS8


def path_cells(mask, conn8, sx, sy, tx, ty, max_dist, order=None):
    """The cells of the link (sx, sy) -> (tx, ty) on a masked grid, source first, or None for "none"."""
    H, W = mask.shape
    if not _in_gate(H, W, sx, sy, tx, ty, max_dist):
        return None
    cost = costs_from(mask, conn8, sx, sy)
    off = int(cost[ty, tx]) // OFF
    moves = int(cost[ty, tx]) % OFF + off
    if moves + 1 >= max_dist:
        return None
    c = _walk(cost, lambda y, x: 1 if mask[y, x] == 1 else OFF, sx, sy, tx, ty, order or _order(conn8), W=W)
    assert len(c) == moves + 1
    return c


def open_staircase(xa, ya, xb, yb, W, conn8):
    """The closed form of AxonDetections._open_dets_paths on the all-ones grid: 4-connected columns first, then rows;
    8-connected the diagonal first, then straight."""
    sx, sy = (1 if xb >= xa else -1), (1 if yb >= ya else -1)
    cells = []
    if conn8:
        k = min(abs(xb - xa), abs(yb - ya))
        cells += [(ya + sy * q, xa + sx * q) for q in range(k + 1)]
        cells += [(ya + sy * k, xa + sx * (k + q)) for q in range(1, abs(xb - xa) - k + 1)]
        cells += [(ya + sy * (k + q), xb) for q in range(1, abs(yb - ya) - k + 1)]
    else:
        cells += [(ya, xa + sx * q) for q in range(abs(xb - xa) + 1)]
        cells += [(ya + sy * q, xb) for q in range(1, abs(yb - ya) + 1)]
    return np.array([r * W + c for r, c in cells], np.int64)


def open_path_cells(H, W, conn8, sx, sy, tx, ty, max_dist):
    """The link on the all-ones grid: the staircase behind the same gate (fewer than max_dist cells), or None."""
    dx, dy = abs(tx - sx), abs(ty - sy)
    if not _in_gate(H, W, sx, sy, tx, ty, max_dist) or (max(dx, dy) if conn8 else dx + dy) + 1 >= max_dist:
        return None
    return open_staircase(sx, sy, tx, ty, W, conn8)


# ------------------------------------------------------------------------------------------------ reference: links, cells
def track_links(track, count, max_gap):
    """i32 [F, cap] (-1: none), i32 [F] -> i64 [n, 3] rows (tail slot f*cap + i, head slot, gap) in ascending tail order:
    the head is the first detection of the same id in frames f+1 .. f+max_gap; counts are clamped to cap."""
    F, cap = track.shape
    n = np.minimum(np.asarray(count, np.int64), cap)
    rows = []
    for f in range(F):
        for i in range(int(n[f])):
            k = int(track[f, i])
            if k < 0:
                continue
            for g in range(1, max_gap + 1):
                if f + g >= F:
                    break
                hit = np.flatnonzero(track[f + g, :n[f + g]] == k)
                if len(hit):
                    rows.append((f * cap + i, (f + g) * cap + int(hit[0]), g))
                    break
    return np.array(rows, np.int64).reshape(-1, 3)


def links_model(track, count, max_gap, broken=None):
    """axt_track_links as its three kernels do it: heads per slot, a prefix sum over the frames, and per frame an ordered
    compaction in chunks of EMIT_CHUNK slots with a carry from chunk to chunk. broken: 'no_chunk_carry' | 'gap_plus_one'."""
    F, cap = track.shape
    n = np.minimum(np.asarray(count, np.int64), cap)
    reach = max_gap + (broken == 'gap_plus_one')
    head = np.full((F, cap), -1, np.int64)
    gap = np.zeros((F, cap), np.int64)
    for f in range(F):
        for i in range(int(n[f])):
            k = int(track[f, i])
            for g in range(1, reach + 1):
                if k < 0 or f + g >= F or head[f, i] >= 0:
                    break
                hit = np.flatnonzero(track[f + g, :n[f + g]] == k)
                if len(hit):
                    head[f, i], gap[f, i] = (f + g) * cap + int(hit[0]), g
    frame_off = np.concatenate([[0], np.cumsum((head >= 0).sum(1))])
    out = np.full((int(frame_off[-1]), 3), -1, np.int64)
    for f in range(F):
        base = int(frame_off[f])
        for i0 in range(0, int(n[f]), EMIT_CHUNK):
            sl = np.arange(i0, min(i0 + EMIT_CHUNK, int(n[f])))
            has = head[f, sl] >= 0
            pos = base + np.cumsum(has) - has
            for i, p in zip(sl[has], pos[has]):
                out[p] = (f * cap + i, head[f, i], gap[f, i])
            if broken != 'no_chunk_carry':
                base += int(has.sum())
    return out


def interp_index(k, L, g, half_down=False):
    """Cell index of the anchor of frame tail + k on a path of L cells over a gap of g frames: k (L-1) / g, half up."""
    return (2 * k * (L - 1) + g - (1 if half_down else 0)) // (2 * g)


def link_cells(lens, paths, gaps, max_dist, max_gap, half_down=False):
    """lens [n] (max_dist: none), paths: per link its cells or None -> (cell_ptr i64 [n+1], cells i64, interp i64
    [n, max_gap-1]: the cell of the anchor of frame tail + k, -1 where k >= gap or the link has no path)."""
    n = len(lens)
    has = [0 < int(L) < max_dist for L in lens]
    cell_ptr = np.concatenate([[0], np.cumsum([int(L) if h else 0 for L, h in zip(lens, has)])]).astype(np.int64)
    cells = np.concatenate([np.asarray(p, np.int64) for p, h in zip(paths, has) if h] + [np.zeros(0, np.int64)])
    interp = np.full((n, max_gap - 1), -1, np.int64)
    for l in range(n):
        for k in range(1, max_gap):
            if has[l] and k < gaps[l]:
                interp[l, k - 1] = paths[l][interp_index(k, int(lens[l]), int(gaps[l]), half_down)]
    return cell_ptr, cells, interp


# ------------------------------------------------------------------------------------------------ component fields
_COMPONENTS, _BFS = {}, {}


def component_fields(mask, conn8):
    """(label i64 [H, W]: 1 .. n_comp on the mask by a flood fill in raster order, 0 off it; n_comp; d_off i64
    [n_comp, H, W] or None with 0 or more than 64 components): d_off[A][c] = fewest off-mask cells a path from component
    A + 1 enters to reach c (c included when off the mask), saturated at 255 -- the multi-source Dijkstra cost // 65536."""
    key = pr._key(mask, conn8)
    if key in _COMPONENTS:
        return _COMPONENTS[key]
    H, W = mask.shape
    steps = _order(conn8)
    label = np.zeros((H, W), np.int64)
    n_comp = 0
    for y, x in zip(*np.nonzero(mask == 1)):                # raster order
        if label[y, x]:
            continue
        n_comp += 1
        label[y, x] = n_comp
        todo = collections.deque([(int(y), int(x))])
        while todo:
            cy, cx = todo.popleft()
            for dy, dx in steps:
                ny, nx = cy + dy, cx + dx
                if 0 <= ny < H and 0 <= nx < W and mask[ny, nx] == 1 and not label[ny, nx]:
                    label[ny, nx] = n_comp
                    todo.append((ny, nx))
    d_off = None
    if 1 <= n_comp <= MAX_COMP:
        G = graph(mask, conn8)
        d_off = np.empty((n_comp, H, W), np.int64)
        for a in range(n_comp):
            cost = dijkstra(G, indices=np.flatnonzero(label.ravel() == a + 1), min_only=True)
            d_off[a] = np.minimum(cost.astype(np.int64) // OFF, 255).reshape(H, W)
    _COMPONENTS[key] = (label, n_comp, d_off)
    return _COMPONENTS[key]


def bfs_field(mask, conn8, sx, sy):
    """f64 [H, W]: moves of the shortest walk from (sx, sy) that enters on-mask cells only (inf: none); the source, on the
    mask or off it, has 0."""
    key = pr._key(mask, conn8) + (sx, sy)
    if key not in _BFS:
        H, W = mask.shape
        src, dst = pr._edges(H, W, conn8)
        keep = mask.ravel()[dst] == 1
        G = coo_matrix((np.ones(keep.sum()), (src[keep], dst[keep])), (H * W, H * W)).tocsr()
        _BFS[key] = dijkstra(G, indices=sy * W + sx, unweighted=True).reshape(H, W)
    return _BFS[key]


# ------------------------------------------------------------------------------------------------ dispatch model
def stage_model(mask, conn8, max_dist, S, T, broken=None):
    """(route, cells or None, info) of one link on a masked grid, stage by stage as recon.hip documents them (see the top).
    broken: None or one of BROKEN, the same stages with that one rule changed."""
    assert broken is None or broken in BROKEN
    (sx, sy), (tx, ty) = S, T
    H, W = mask.shape
    order = _order(conn8, broken == 'diagonals_first')
    if not _in_gate(H, W, sx, sy, tx, ty, max_dist):
        return 'gate', None, {}
    label, n_comp, d_off = component_fields(mask, conn8)
    s_on, t_on = mask[sy, sx] == 1, mask[ty, tx] == 1
    pending = S == T or (t_on and not (s_on and label[sy, sx] != label[ty, tx]))
    adx, ady = abs(tx - sx), abs(ty - sy)
    if pending:
        dist = bfs_field(mask, conn8, sx, sy)
        d = dist[ty, tx]
        for R in (31, 127):
            limit = R if broken == 'limit_R' else min(R, max_dist - 2)
            if d <= limit:
                return f'bfs{R}', _walk(dist, lambda y, x: 1, sx, sy, tx, ty, order, W=W), dict(d=int(d))
            if limit == max_dist - 2 and (s_on or broken == 'rule_for_off_source'):
                return f'bfs{R}', None, dict(d=d)
    if d_off is not None:
        if s_on:
            lb = int(d_off[label[sy, sx] - 1, ty, tx])
        else:
            lb = min([max(adx, ady) if conn8 else adx + ady] + [int(d_off[a, sy, sx]) - 1 + int(d_off[a, ty, tx]) for a in range(n_comp)])
        for R in (31, 63):
            if max(adx, ady) > R:
                continue
            x0, y0, x1, y1 = max(sx - R, 0), max(sy - R, 0), min(sx + R, W - 1), min(sy + R, H - 1)
            sub = np.ascontiguousarray(mask[y0:y1 + 1, x0:x1 + 1])
            cost = costs_from(sub, conn8, sx - x0, sy - y0)
            o = int(cost[ty - y0, tx - x0]) // OFF
            m = int(cost[ty - y0, tx - x0]) % OFF + o
            if (m <= R or broken == 'no_m_le_R') and (o == lb or broken == 'no_o_eq_lb'):
                info = dict(o=o, m=m, lb=lb)
                if m + 1 >= max_dist:
                    return f'key{R}', None, info
                return f'key{R}', _walk(cost, lambda y, x: 1 if sub[y, x] == 1 else OFF, sx - x0, sy - y0, tx - x0, ty - y0,
                                        order, x0, y0, W), info
    return 'exact', path_cells(mask, conn8, sx, sy, tx, ty, max_dist, order), {}


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass
class Pair:
    """One link: its name, source and target (x, y), the route the name stands for (a pair (4-connected, 8-connected)
    where they differ) and the frame of its head (two_grids)."""
    name: str
    S: tuple
    T: tuple
    route: object
    frame: int = 1


@dataclasses.dataclass(eq=False)
class Case:
    """masks: one mask u8 [H, W] per group, None for the all-ones grid; head_group: None (one group) or the group of the
    links whose head lies in frame f."""
    name: str
    masks: list
    conn8: bool
    max_dist: int
    pairs: list
    shape: tuple
    head_group: list = None

    def __repr__(self):
        return self.name

    def mask_of(self, p):
        return self.masks[0 if self.head_group is None else self.head_group[p.frame]]

    def claimed(self, p):
        return p.route if isinstance(p.route, str) else p.route[int(self.conn8)]

    def pair(self, name):
        return next(p for p in self.pairs if p.name == name)

    @property
    def n_frames(self):
        return 2 if self.head_group is None else len(self.head_group)

    def arrays(self):
        """(x i32 [F, cap], y i32 [F, cap], links i32 [n, 3]): pair i has its tail in slot i of frame 0 and its head in slot
        i of its head frame; gaps alternate 1, 2 (max_gap = 2)."""
        n = len(self.pairs)
        x, y = np.zeros((self.n_frames, n), np.int32), np.zeros((self.n_frames, n), np.int32)
        links = np.zeros((n, 3), np.int32)
        for i, p in enumerate(self.pairs):
            x[0, i], y[0, i] = p.S
            x[p.frame, i], y[p.frame, i] = p.T
            links[i] = (i, p.frame * n + i, 1 + i % 2)
        return x, y, links


def route(case, i, broken=None):
    """The stage that decides pair i of the case ('open' on the all-ones grid, which has no stages)."""
    p = case.pairs[i]
    m = case.mask_of(p)
    return 'open' if m is None else stage_model(m, case.conn8, case.max_dist, p.S, p.T, broken)[0]


@functools.lru_cache(None)
def expected_paths(case):
    """Per pair the reference cells or None."""
    H, W = case.shape
    out = []
    for p in case.pairs:
        m = case.mask_of(p)
        out.append(open_path_cells(H, W, case.conn8, *p.S, *p.T, case.max_dist) if m is None
                   else path_cells(m, case.conn8, *p.S, *p.T, case.max_dist))
    return out


def expected_arrays(case, max_gap=2):
    """(len, cell_ptr, cells, interp) as hp.link_paths returns them for case.arrays()."""
    paths = expected_paths(case)
    lens = np.array([case.max_dist if p is None else len(p) for p in paths], np.int64)
    return (lens,) + link_cells(lens, paths, case.arrays()[2][:, 2], case.max_dist, max_gap)


def stage_counts(case):
    """{route: selected links it decides} over the masked groups of the case, and the number of those links."""
    routes = [route(case, i) for i in range(len(case.pairs))]
    return {r: routes.count(r) for r in ROUTES}, sum(r != 'open' for r in routes)


# ------------------------------------------------------------------------------------------------ the battery
def _u_turn(m, ya, yb, xa, xr):
    """Rows ya and yb from xa to xr, joined by the column xr."""
    m[ya, xa:xr + 1] = 1
    m[yb, xa:xr + 1] = 1
    m[ya:yb + 1, xr] = 1


def _case(name, mask, c8, pairs, max_dist=500):
    return Case(name + ('_conn8' if c8 else ''), [mask], c8, max_dist, pairs, mask.shape)


def _two_rows_mask(H=40, W=120, shift=0):
    """Component A: row 5; component B: row 9 (three off-mask rows between them); rows 10 .. H-1 a void."""
    m = np.zeros((H, W), np.uint8)
    m[5 + shift, :] = 1
    m[9 + shift, :] = 1
    return m


def _reject_moves_mask():
    """One component around S = (50, 20): row 20 out to x = 82, down the column 82 and back along row 23 to x = 76 (a route
    that leaves the radius-31 window of S); and down the column 50, along row 32 and up the column 74 to (74, 23) (a
    longer route inside it). (75, 23), off the mask, lies between the two ends."""
    m = np.zeros((45, 110), np.uint8)
    m[20, 50:83] = 1
    m[20:24, 82] = 1
    m[23, 76:83] = 1
    m[20:33, 50] = 1
    m[32, 50:75] = 1
    m[23:33, 74] = 1
    return m


def _pixel_mask(n_comp):
    """Row 1 and n_comp - 1 isolated pixels on a lattice (x = 3, 7, ..; y = 5, 7, ..): n_comp components either way."""
    m = np.zeros((24, 140), np.uint8)
    m[1, :] = 1
    return pr._pixels(m, n_comp - 1, 5)


@functools.lru_cache(None)
def battery():
    cases = []
    add = cases.append
    for c8 in (False, True):
        # ---------------------------------------------------------------- bfs_steps: 31 | 32 and 127 | 128 moves
        m = np.zeros((12, 300), np.uint8)
        m[2, :] = 1
        d = 16 if c8 else 15                                 # the u-turn: 2 d + 2 moves, 8-connected two corners cut
        _u_turn(m, 6, 8, 200, 200 + d)
        add(_case('bfs_steps', m, c8, [
            Pair('straight_31', (5, 2), (36, 2), 'bfs31'), Pair('straight_32', (5, 2), (37, 2), 'bfs127'),
            Pair('straight_127', (5, 2), (132, 2), 'bfs127'), Pair('straight_128', (5, 2), (133, 2), 'exact'),
            Pair('left_31', (290, 2), (259, 2), 'bfs31'), Pair('left_32', (290, 2), (258, 2), 'bfs127'),
            Pair('detour_31', (200, 6), (201, 8), 'bfs31'), Pair('detour_32', (200, 6), (200, 8), 'bfs127'),
            Pair('same_cell_on', (5, 2), (5, 2), 'bfs31'), Pair('same_cell_off', (5, 0), (5, 0), 'bfs31')]))
        # ---------------------------------------------------------------- bfs_border: windows clipped at the grid border
        m = np.zeros((40, 50), np.uint8)
        m[[0, -1], :] = 1
        m[:, [0, -1]] = 1
        add(_case('bfs_border', m, c8, [
            Pair('tl_along_x', (0, 0), (20, 0), 'bfs31'), Pair('tl_along_y', (0, 0), (0, 25), 'bfs31'),
            Pair('tl_round_corner', (0, 0), (49, 10), 'bfs127'),
            Pair('tr_along_x', (49, 0), (29, 0), 'bfs31'), Pair('tr_along_y', (49, 0), (49, 39), 'bfs127'),
            Pair('bl_along_y', (0, 39), (0, 10), 'bfs31'), Pair('bl_along_x', (0, 39), (40, 39), 'bfs127'),
            Pair('br_along_y', (49, 39), (49, 9), 'bfs31'), Pair('br_along_x', (49, 39), (0, 39), 'bfs127'),
            Pair('br_round_corner', (49, 39), (0, 30), 'bfs127'),
            Pair('top_round_corner', (25, 0), (49, 5), 'bfs31'), Pair('top_far', (25, 0), (0, 20), 'bfs127'),
            Pair('bottom_along', (25, 39), (5, 39), 'bfs31'), Pair('bottom_far', (25, 39), (49, 20), 'bfs127'),
            Pair('left_along', (0, 20), (0, 0), 'bfs31'), Pair('left_far', (0, 20), (30, 0), 'bfs127'),
            Pair('right_along', (49, 20), (49, 39), 'bfs31'), Pair('right_far', (49, 20), (20, 39), 'bfs127')]))
        # ---------------------------------------------------------------- bfs_plaza: many equally cheap paths
        m = np.zeros((40, 40), np.uint8)
        m[8:33, 8:33] = 1
        octants = [(7, 3), (3, 7), (-3, 7), (-7, 3), (-7, -3), (-3, -7), (3, -7), (7, -3), (6, 0), (0, 6), (-6, 0), (0, -6),
                   (5, 5), (-5, 5), (-5, -5), (5, -5)]
        add(_case('bfs_plaza', m, c8, [Pair(f'octant_{dx}_{dy}', (20, 20), (20 + dx, 20 + dy), 'bfs31') for dx, dy in octants] + [
            Pair('off_source', (7, 20), (15, 25), 'bfs31'), Pair('off_source_up', (20, 33), (26, 27), 'bfs31'),
            Pair('corner_to_corner', (8, 8), (32, 30), ('bfs127', 'bfs31'))]))
        # ---------------------------------------------------------------- no_path_rule: limit == max_dist - 2
        m = np.zeros((30, 130), np.uint8)
        m[2, :] = 1
        _u_turn(m, 8, 11, 40, 48 + c8)                       # (40, 8) -> (41, 11): 18 moves, -> (40, 11): 19
        m[20, 60:62] = 1                                     # an island of two cells
        m[24, 55:71] = 1                                     # and a bar below it
        k = int(c8)                                          # from (5, 1), off the mask, the first move is diagonal
        add(_case('no_path_rule_20', m, c8, [
            Pair('on_18', (5, 2), (23, 2), 'bfs31'), Pair('on_19_none', (5, 2), (24, 2), 'bfs31'),
            Pair('detour_18', (40, 8), (41, 11), 'bfs31'), Pair('detour_19_none', (40, 8), (40, 11), 'bfs31'),
            Pair('off_source_18', (5, 1), (22 + k, 2), 'bfs31'), Pair('off_source_19_none', (5, 1), (23 + k, 2), 'key31'),
            Pair('off_source_island_to_bar', (59, 20), (62, 24), 'key31'),
            Pair('gate_equal', (100, 5), (112, 21), 'gate'), Pair('gate_inside', (100, 5), (112, 20), ('key63', 'key31')),
            Pair('source_outside', (-1, 2), (5, 2), 'gate'), Pair('target_outside', (120, 2), (130, 2), 'gate'),
            Pair('target_below', (5, 20), (5, 30), 'gate')], max_dist=20))
        m = np.zeros((12, 130), np.uint8)
        m[2, :] = 1
        _u_turn(m, 6, 9, 10, 58 + c8)                        # (10, 6) -> (11, 9): 98 moves, -> (10, 9): 99
        add(_case('no_path_rule_100', m, c8, [
            Pair('on_98', (5, 2), (103, 2), 'bfs127'), Pair('on_99_none', (5, 2), (104, 2), 'bfs127'),
            Pair('detour_98', (10, 6), (11, 9), 'bfs127'), Pair('detour_99_none', (10, 6), (10, 9), 'bfs127'),
            Pair('off_source_98', (5, 1), (102 + k, 2), 'bfs127'), Pair('off_source_99_none', (5, 1), (103 + k, 2), 'exact')],
            max_dist=100))
        # ---------------------------------------------------------------- key_accept
        m = _two_rows_mask()
        a = (lambda mv: mv) if c8 else (lambda mv: mv - 2)   # T = (10 + a, 3), two off-mask cells above row 5: a + 2 | a moves
        b = (lambda mv: mv) if c8 else (lambda mv: mv - 4)   # T = (10 + b, 9) on the other row: b + 4 | b moves
        add(_case('key_accept', m, c8, [
            Pair('off_target_m31', (10, 5), (10 + a(31), 3), 'key31'), Pair('off_target_m32', (10, 5), (10 + a(32), 3), 'key63'),
            Pair('off_target_m63', (10, 5), (10 + a(63), 3), 'key63'), Pair('off_target_m64', (10, 5), (10 + a(64), 3), 'exact'),
            Pair('other_component_m31', (10, 5), (10 + b(31), 9), 'key31'),
            Pair('other_component_m32', (10, 5), (10 + b(32), 9), 'key63'),
            Pair('other_component_left', (100, 9), (80, 5), 'key31'),
            Pair('void_metric_bound', (30, 30), (45, 34), 'key31'), Pair('void_metric_bound_up_left', (45, 34), (33, 25), 'key31'),
            Pair('off_source_crosses_component', (60, 7), (80, 7), 'key31')]))
        # ---------------------------------------------------------------- key_reject_off
        m = np.zeros((10, 180), np.uint8)
        _u_turn(m, 2, 6, 40, 170)
        add(_case('key_reject_off', m, c8, [
            Pair('long_route', (100, 2), (100, 5), 'exact'), Pair('long_route_too_long_none', (45, 2), (45, 5), 'exact'),
            Pair('next_to_source', (100, 2), (100, 3), 'key31')], max_dist=200))
        # ---------------------------------------------------------------- key_reject_moves
        add(_case('key_reject_moves', _reject_moves_mask(), c8, [
            Pair('winding_inside_window', (50, 20), (73, 26), 'key63'), Pair('optimum_leaves_window', (50, 20), (75, 23), 'key63'),
            Pair('short', (50, 20), (49, 25), 'key31')]))
        # ---------------------------------------------------------------- exhausted
        m = np.zeros((30, 60), np.uint8)
        m[10, 21:23] = 1
        m[14, :] = 1
        add(_case('exhausted', m, c8, [
            Pair('island_to_corridor', (20, 10), (25, 14), 'key31'), Pair('onto_the_island', (20, 10), (22, 10), 'bfs31'),
            Pair('no_on_mask_neighbour', (20, 5), (25, 14), 'key31')]))
        # ---------------------------------------------------------------- components_64_65
        for n_comp in (64, 65):
            key = 'key31' if n_comp == 64 else 'exact'
            add(_case(f'components_{n_comp}', _pixel_mask(n_comp), c8, [
                Pair('along_the_row', (10, 1), (30, 1), 'bfs31'), Pair('row_to_pixel', (10, 1), (11, 5), key),
                Pair('row_to_off_target', (10, 1), (12, 3), key), Pair('pixel_to_pixel', (3, 5), (7, 5), key),
                Pair('pixel_to_row', (7, 7), (20, 1), key), Pair('off_source_exhausted', (20, 3), (30, 1), key),
                Pair('void_many_ties', (60, 15), (70, 21), key), Pair('far', (0, 1), (100, 6), 'exact')]))
        # ---------------------------------------------------------------- two_grids
        m0, m1 = _two_rows_mask(), _two_rows_mask(shift=4)
        pairs = []
        for f, tag in ((1, 'first'), (2, 'second'), (3, 'open')):
            r = (lambda first, second: 'open' if f == 3 else first if f == 1 else second)
            pairs += [Pair(f'{tag}_off_target', (10, 5), (39, 3), r('key31', ('key63', 'key31')), f),
                      Pair(f'{tag}_void', (30, 30), (45, 34), r('key31', 'key31'), f),
                      Pair(f'{tag}_crossing', (60, 7), (80, 7), r('key31', 'key31'), f),
                      Pair(f'{tag}_along_row_9', (10, 9), (30, 9), r('bfs31', 'bfs31'), f),
                      Pair(f'{tag}_up_left', (80, 30), (60, 12), r(('key63', 'key31'), ('key63', 'key31')), f)]
        add(Case('two_grids' + ('_conn8' if c8 else ''), [m0, m1, None], c8, 500, pairs, m0.shape, head_group=[0, 0, 1, 2]))
    return cases


def case(name):
    return next(c for c in battery() if c.name == name)


# ------------------------------------------------------------------------------------------------ links_shapes
@functools.lru_cache(None)
def links_table():
    """track i32 [1030, 300], count i32 [1030]: most frames hold a few of the ids 0 .. 7 in changing slots with -1 between
    them; frames 10 .. 12 hold 300 ids each (frame 11 drops every third, frame 12 claims a count above cap), frame 500 holds
    270 (more than one chunk); id 900 reappears after 2, 3 and 4 frames; the last frames hold ids too."""
    F, cap = 1030, 300
    rng = np.random.default_rng(11)
    track = np.full((F, cap), -1, np.int32)
    count = np.zeros(F, np.int32)
    for f in range(F):
        n = int(rng.integers(2, 9))
        ids = rng.permutation(8)[:n].astype(np.int32)
        ids[rng.random(n) < 0.2] = -1
        track[f, :n] = ids
        count[f] = n
        track[f, n:n + 3] = rng.permutation(8)[:3]           # ids beyond the count: not detections
    for f, drop in ((10, 0), (11, 3), (12, 0)):
        ids = 1000 + rng.permutation(cap).astype(np.int32)
        if drop:
            ids[ids % drop == 0] = -1
        track[f], count[f] = ids, cap
    count[12] = 350                                          # clamped to cap
    track[500, :270], count[500] = 2000 + rng.permutation(270), 270
    track[501, :270], count[501] = 2000 + rng.permutation(270), 270
    track[F - 2, :4], count[F - 2] = (4, 6, -1, 2), 4          # the last frame as a head, and ids that end with the table
    track[F - 1, :3], count[F - 1] = (6, -1, 4), 3
    for f0, g in ((20, 2), (40, 3), (60, 4), (80, 1)):
        for f in (f0, f0 + g):
            track[f, count[f]] = 900
            count[f] += 1
    track.setflags(write=False)
    count.setflags(write=False)
    return track, count


# ------------------------------------------------------------------------------------------------ cells_shapes
@dataclasses.dataclass(eq=False)
class CellsCase:
    """Links on the all-ones grid for axt_link_cells: x, y i32 [2, cap], links i32 [n, 3]."""
    name: str
    conn8: bool
    max_gap: int
    max_dist: int
    shape: tuple
    x: np.ndarray
    y: np.ndarray
    links: np.ndarray

    def __repr__(self):
        return self.name

    def expected(self):
        H, W = self.shape
        cap = self.x.shape[1]
        xf, yf = self.x.ravel(), self.y.ravel()
        paths = [open_path_cells(H, W, self.conn8, int(xf[a]), int(yf[a]), int(xf[b]), int(yf[b]), self.max_dist)
                 for a, b, _ in self.links]
        assert cap * 2 == len(xf)
        lens = np.array([self.max_dist if p is None else len(p) for p in paths], np.int64)
        return (lens,) + link_cells(lens, paths, self.links[:, 2], self.max_dist, self.max_gap)


@functools.lru_cache(None)
def cells_battery():
    """1100 links (more than the 1024 partitions of the scan) on a 100 x 200 grid at max_dist = 150: paths of up to 149
    cells (the 64-thread fill strides), links without a path mixed in (too long, outside the grid), gaps 1 .. max_gap."""
    H, W, n = 100, 200, 1100
    out = []
    for c8 in (False, True):
        for max_gap in (3, 1):
            rng = np.random.default_rng(5 + max_gap)
            x = rng.integers(0, W, (2, n)).astype(np.int32)
            y = rng.integers(0, H, (2, n)).astype(np.int32)
            x[1, ::7] = x[0, ::7] + rng.integers(-3, 4, len(x[0, ::7]))          # short links among the long ones
            x[1, 5::97] = W                                                   # heads outside the grid
            x[1, 6::97] = x[0, 6::97]                                         # single cells
            y[1, 6::97] = y[0, 6::97]
            links = np.stack([np.arange(n), n + np.arange(n), 1 + np.arange(n) % max_gap], 1).astype(np.int32)
            out.append(CellsCase(f'cells_max_gap{max_gap}' + ('_conn8' if c8 else ''), c8, max_gap, 150, (H, W), x, y, links))
    return out
