"""CPU reference, scene generators, case batteries and judge for the Hungarian association kernels
(axtrack_amd/csrc/hungarian.hip). No GPU and no product code: everything here is built from oracle/ and from the
definition in the header comment of hungarian.hip --

    pass 1, every pair (t, t+1):  min  sum_{linked} c(a, b) + sum_{rows without link} U(a)     (exact, integer costs)
    pass 2, every pair (t, t+2):  the same between rows without successor and columns without predecessor after pass 1
    chains numbered by (first frame, index)

-- solved with SciPy's linear_sum_assignment on the n x (m + n) matrix with one private dummy column per row, exactly as
oracle.hungarian_assoc builds it. Used by tests/test_hungarian_cpu.py (which proves the cases are what their names say)
and tests/test_hungarian_paths_gpu.py (which runs them through the kernels)."""
import functools

import numpy as np

from oracle import oracle as orc

NO_LINK = 0x3fffffffffffffff                       # a link that is not admitted (include/axtrack_hip.h)
THR_UNITS = int(np.rint(orc.DEFAULTS['MCF_EDGE_COST_THR'] * orc.COST_SCALE))
EXACT_F64 = 1 << 37                                # costs below this: sums of up to 2^15 of them are exact in f64


# ------------------------------------------------------------------------------------------------ costs
def arc_cost_vec(units, kind, a, b):
    """oracle.arc_cost_int for arrays, with the cost already in integer units (rint(cost * COST_SCALE)): pinned to the
    oracle's scalar function by tests/test_hungarian_cpu.py."""
    units, a, b = np.broadcast_arrays(np.asarray(units, np.int64), np.asarray(a, np.int64), np.asarray(b, np.int64))
    x = (np.uint64(int(kind) << 60) ^ (a.astype(np.uint64) << np.uint64(30)) ^ b.astype(np.uint64)).reshape(-1)
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    pert = (x & np.uint64((1 << orc.PERT_BITS) - 1)).astype(np.int64).reshape(units.shape)
    return (units << orc.PERT_BITS) + pert


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def dummy_costs(counts, thr_units=THR_UNITS):
    """Per frame, the cost of leaving each detection without a successor: arc_cost_int(thr, 1, global index, 0)."""
    offs = offsets(counts)
    return [arc_cost_vec(thr_units, 1, offs[t] + np.arange(n), 0) for t, n in enumerate(counts)]


def geometric_costs(dets, H, W, mask=None, conn8=False, P=orc.DEFAULTS):
    """{(t, gap): i64 [n_t, n_{t+gap}]} link costs of a scene from the oracle's path lengths and transition model
    (NO_LINK where transition_cost >= MCF_EDGE_COST_THR), as oracle.hungarian_assoc.solve fills its matrix."""
    counts = [len(d[0]) for d in dets]
    offs = offsets(counts)
    out = {}
    for g in range(1, P['MCF_MAX_NUM_MISSES'] + 2):
        for t in range(len(dets) - g):
            n, m = counts[t], counts[t + g]
            if n == 0 or m == 0:
                out[(t, g)] = np.full((n, m), NO_LINK, np.int64)
                continue
            D = orc.path_matrix(dets[t], dets[t + g], H, W, orc.mask_of_frame(mask, t + g), conn8=conn8)
            c = orc.transition_cost(D, g, P['MCF_MISS_RATE'])
            adm = c < P['MCF_EDGE_COST_THR']
            units = np.rint(np.where(adm, c, 0.0) * orc.COST_SCALE).astype(np.int64)
            cost = arc_cost_vec(units, 3, offs[t] + np.arange(n)[:, None], offs[t + g] + np.arange(m)[None, :])
            out[(t, g)] = np.where(adm, cost, NO_LINK)
    return out


def costs_to_table(costs, counts, cap, gaps=2):
    """The dense table axt_hungarian_pairs reads as d_ctab: i64 [F, cap, gaps, cap], NO_LINK where nothing is given."""
    F = len(counts)
    tab = np.full((F, cap, gaps, cap), NO_LINK, np.int64)
    for (t, g), c in costs.items():
        if g <= gaps:
            tab[t, :c.shape[0], g - 1, :c.shape[1]] = c
    return tab


def costs_from_table(ctab, counts):
    F, _, gaps, _ = ctab.shape
    return {(t, g): np.asarray(ctab[t, :counts[t], g - 1, :counts[t + g]], np.int64)
            for g in range(1, gaps + 1) for t in range(F - g)}


# ------------------------------------------------------------------------------------------------ reference
def pair_reference(cost, dummy):
    """Exact optimum of one pair: cost i64 [n, m] (NO_LINK = not admitted), dummy i64 [n].
    Returns (match i64 [n]: column or -1, the integer optimum: links plus dummies)."""
    from scipy.optimize import linear_sum_assignment
    cost, dummy = np.asarray(cost, np.int64), np.asarray(dummy, np.int64)
    n, m = cost.shape
    if n == 0:
        return np.zeros(0, np.int64), 0
    adm = cost != NO_LINK
    assert (cost[adm] < EXACT_F64).all() and (cost[adm] >= 0).all() and (dummy < EXACT_F64).all() and n < (1 << 15), \
        'costs too large for exact f64 sums'
    M = np.full((n, m + n), np.inf)
    M[:, :m][adm] = cost[adm].astype(np.float64)
    M[np.arange(n), m + np.arange(n)] = dummy.astype(np.float64)
    ri, ci = linear_sum_assignment(M)
    assert np.array_equal(ri, np.arange(n))
    match = np.where(ci < m, ci, -1).astype(np.int64)
    linked = match >= 0
    total = int(cost[np.nonzero(linked)[0], match[linked]].sum()) + int(dummy[~linked].sum())
    return match, total


class Reference:
    """trajs: list of [(frame, idx), ...] in id order; pairs: {(t, gap): dict(rows, cols, match, total)} with match in
    indices of the full frame (-1: no link); succ / succ_gap per frame."""

    def __init__(self, trajs, pairs, succ, succ_gap):
        self.trajs, self.pairs, self.succ, self.succ_gap = trajs, pairs, succ, succ_gap


def reference_from_costs(costs, counts, thr_units=THR_UNITS, max_gap=2):
    counts = [int(c) for c in counts]
    F = len(counts)
    dummies = dummy_costs(counts, thr_units)
    succ = [np.full(n, -1, np.int64) for n in counts]
    succ_gap = [np.zeros(n, np.int64) for n in counts]
    has_pred = [np.zeros(n, bool) for n in counts]
    pairs = {}

    def solve(t, g, rows, cols):
        sub = costs[(t, g)][np.ix_(rows, cols)]
        match, total = pair_reference(sub, dummies[t][rows])
        full = np.full(len(rows), -1, np.int64)
        full[match >= 0] = cols[match[match >= 0]]
        pairs[(t, g)] = dict(rows=rows, cols=cols, match=full, total=total)
        li = match >= 0
        succ[t][rows[li]] = full[li]
        succ_gap[t][rows[li]] = g
        has_pred[t + g][full[li]] = True

    for t in range(F - 1):
        solve(t, 1, np.arange(counts[t]), np.arange(counts[t + 1]))
    if max_gap >= 2:
        pred1 = [h.copy() for h in has_pred]
        succ1 = [s.copy() for s in succ]
        for t in range(F - 2):      # gap 2: rows without a successor, columns without a predecessor after pass 1
            solve(t, 2, np.nonzero(succ1[t] < 0)[0], np.nonzero(~pred1[t + 2])[0])
    trajs = []
    for t in range(F):              # chains numbered by (first frame, index)
        for i in range(counts[t]):
            if has_pred[t][i]:
                continue
            tr, f, k = [], t, i
            while True:
                tr.append((f, int(k)))
                if succ[f][k] < 0:
                    break
                f, k = f + int(succ_gap[f][k]), int(succ[f][k])
            trajs.append(tr)
    return Reference(trajs, pairs, succ, succ_gap)


def reference_from_table(ctab, counts, thr_units=THR_UNITS):
    """The two passes and the chain numbering on a GIVEN cost table i64 [F, cap, gaps, cap]."""
    ctab = np.asarray(ctab)
    return reference_from_costs(costs_from_table(ctab, counts), counts, thr_units, max_gap=ctab.shape[2])


def needs_search(cost, dummy):
    """Number of rows that lose the initialisation's contest (header comment of hungarian.hip: every row takes its cheapest
    option, a column or its own dummy, if it is still free): rows, in order, whose cheapest option is a column already
    taken by an earlier row. cost i64 [n, m] of the rows and columns that take part, dummy i64 [n]."""
    cost, dummy = np.asarray(cost, np.int64), np.asarray(dummy, np.int64)
    n, m = cost.shape
    if n == 0 or m == 0:
        return 0
    best = cost.argmin(axis=1)
    wants = cost[np.arange(n), best] < dummy
    taken, lost = set(), 0
    for i in range(n):
        if wants[i]:
            if int(best[i]) in taken:
                lost += 1
            else:
                taken.add(int(best[i]))
    return lost


# ------------------------------------------------------------------------------------------------ judge
class JudgeError(AssertionError):
    def __init__(self, step, msg):
        super().__init__(f'step {step}: {msg}')
        self.step = step


def judge(costs, counts, track, n_tracks, name='', thr_units=THR_UNITS, max_gap=2, ref=None):
    """Judge a track table i32 [F, cap] and a track count against the definition, in five steps; raises JudgeError(step)
    at the first that fails:
      1 the links recovered from `track` form a matching (at most one detection of a frame per track, gaps in {1, 2} --
        so every detection has at most one successor and one predecessor, and a gap-2 link joins detections pass 1 left free);
      2 every link is admitted;
      3 per pair and gap, the integer total (links plus dummies) equals the SciPy optimum of that pair;
      4 the trajectories equal the reference list;
      5 slots beyond count are -1 and n_tracks is the number of trajectories."""
    counts = [int(c) for c in counts]
    F = len(counts)
    track = np.asarray(track)
    dummies = dummy_costs(counts, thr_units)
    where = lambda t, g: f'{name}: pair ({t},{t + g}) gap {g}, n={counts[t]} m={counts[t + g]}'
    # ---- 1
    members = {}
    for t in range(F):
        for i in range(counts[t]):
            k = int(track[t, i])
            if k < 0:
                raise JudgeError(1, f'{name}: detection ({t},{i}) has no track')
            members.setdefault(k, []).append((t, i))
    succ = [np.full(n, -1, np.int64) for n in counts]
    succ_gap = [np.zeros(n, np.int64) for n in counts]
    has_pred = [np.zeros(n, np.int64) for n in counts]           # gap of the link that ends here, 0: none
    for k, mem in members.items():
        for (t0, i0), (t1, i1) in zip(mem, mem[1:]):
            if t1 == t0:
                raise JudgeError(1, f'{name}: track {k} holds ({t0},{i0}) and ({t1},{i1}) of one frame: a detection of frame '
                                    f'{t0 - 1} or {t0 - 2} has two successors, or one of a later frame two predecessors')
            if t1 - t0 > max_gap:
                raise JudgeError(1, f'{name}: track {k} links ({t0},{i0}) to ({t1},{i1}): gap {t1 - t0}')
            succ[t0][i0], succ_gap[t0][i0], has_pred[t1][i1] = i1, t1 - t0, t1 - t0
    # ---- 2
    for t in range(F):
        for i in np.nonzero(succ[t] >= 0)[0]:
            g, j = int(succ_gap[t][i]), int(succ[t][i])
            if costs[(t, g)][i, j] == NO_LINK:
                raise JudgeError(2, f'{where(t, g)}: link {i} -> {j} is not admitted')
    # ---- 3 (pass 2 on what the judged table's own pass 1 left free: pass 1 has been proven by then)
    for g in range(1, max_gap + 1):
        for t in range(F - g):
            if g == 1:
                rows, cols = np.arange(counts[t]), np.arange(counts[t + 1])
            else:
                rows = np.nonzero(succ_gap[t] != 1)[0]
                cols = np.nonzero(has_pred[t + 2] != 1)[0]
            li = rows[succ_gap[t][rows] == g]
            total = int(costs[(t, g)][li, succ[t][li]].sum()) + int(dummies[t][rows[succ_gap[t][rows] != g]].sum())
            _, opt = pair_reference(costs[(t, g)][np.ix_(rows, cols)], dummies[t][rows])
            if total != opt:
                raise JudgeError(3, f'{where(t, g)} ({len(rows)} rows x {len(cols)} columns take part): total {total}, optimum {opt}')
    # ---- 4
    ref = ref or reference_from_costs(costs, counts, thr_units, max_gap)
    got = [members[k] for k in sorted(members)]
    if got != ref.trajs:
        bad = next((k for k, (a, b) in enumerate(zip(got, ref.trajs)) if a != b), min(len(got), len(ref.trajs)))
        raise JudgeError(4, f'{name}: {len(got)} trajectories, reference {len(ref.trajs)}; first difference at id {bad}: '
                            f'{got[bad] if bad < len(got) else None} vs {ref.trajs[bad] if bad < len(ref.trajs) else None}')
    # ---- 5
    cap = track.shape[1]
    beyond = np.arange(cap)[None, :] >= np.asarray(counts)[:, None]
    if not (track[beyond] == -1).all():
        t, i = np.argwhere(beyond & (track != -1))[0]
        raise JudgeError(5, f'{name}: slot ({t},{i}) beyond count {counts[t]} holds {track[t, i]}')
    if int(n_tracks) != len(ref.trajs):
        raise JudgeError(5, f'{name}: n_tracks {int(n_tracks)}, {len(ref.trajs)} trajectories')
    return ref


def track_table(trajs, counts, cap):
    """The table a correct run writes: i32 [F, cap], -1 beyond count."""
    track = np.full((len(counts), cap), -1, np.int32)
    for k, tr in enumerate(trajs):
        for f, i in tr:
            track[f, i] = k
    return track


# ------------------------------------------------------------------------------------------------ dispatch (restated)
def dispatch(cap, max_dist=500):
    """(NC, cdim) of axt_hungarian_pairs for a slot count, restated from its formulas in axtrack_amd/csrc/hungarian.hip:
    `lds_base` (the two lines of `const size_t lds_base = ...`), `int cdim = cap < 96 ? cap : 96; if (lds_base + cdim*cdim*8 >
    160 KiB) cdim = 0;`, and the launches' `cap <= 192 ? <.,3> : cap <= 576 ? <.,9> : <.,0>`."""
    lds_base = cap * (3 * 8 + 8 * 4 + 2) + 8 + (max_dist + 2) * 8 + 8 + cap * 8 + (cap * 48 if cap <= 576 else 0)
    assert lds_base <= 160 * 1024
    cdim = min(cap, 96)
    if lds_base + cdim * cdim * 8 > 160 * 1024:
        cdim = 0
    return (3 if cap <= 192 else 9 if cap <= 576 else 0), cdim


def first_cap_without_cache(max_dist=500):
    return next(c for c in range(577, 2049) if dispatch(c, max_dist)[1] == 0)


def pair_path(cap, n, m):
    """The path a pair of n x m detections takes: (NC, register slots or None, cached) -- `resident(...)`'s choice
    `m <= 64 / m <= 128 / else` under NC == 3, and `cached = n <= cdim && m <= cdim` in hungarian_pair_kernel."""
    nc, cdim = dispatch(cap)
    slots = (1 if m <= 64 else 2 if m <= 128 else 3) if nc == 3 else None
    return nc, slots, (n <= cdim and m <= cdim)


# ------------------------------------------------------------------------------------------------ scenes
def _frame(rng, x, y):
    conf = np.sort(rng.uniform(0.55, 1.2, len(x)).astype(np.float32))[::-1]
    return conf, np.asarray(x, np.int64), np.asarray(y, np.int64)


def clustered(F, n_per_frame, H, W, clusters, spread, seed=0):
    """Detections within +-spread px of a few cluster centres, drawn anew in every frame: most rows of a pair want a column
    another row wants too. n_per_frame: one count or one per frame. A few points fall just outside the image (no links)."""
    rng = np.random.default_rng(seed)
    counts = [n_per_frame] * F if np.isscalar(n_per_frame) else list(n_per_frame)
    assert len(counts) == F
    lo = min(spread - 4, W // 2, H // 2)
    cx = rng.integers(lo, max(W - lo, lo + 1), clusters)
    cy = rng.integers(lo, max(H - lo, lo + 1), clusters)
    dets = []
    for n in counts:
        k = rng.integers(0, clusters, n)
        dets.append(_frame(rng, cx[k] + rng.integers(-spread, spread + 1, n), cy[k] + rng.integers(-spread, spread + 1, n)))
    return dets


def alternating(F, n_big, n_small, H, W, clusters, spread, seed=0, pattern='BsBBssB'):
    """Crowded and sparse frames side by side: n >> m, m >> n, big x big and small x small pairs."""
    counts = [n_big if pattern[t % len(pattern)] == 'B' else n_small for t in range(F)]
    return clustered(F, counts, H, W, clusters, spread, seed)


def lattice(F, nx, ny, pitch, counts=None, seed=0):
    """Detections on a regular nx x ny grid that moves by one cell per frame, listed in a random order: every detection
    has several links of the same length, hence of equal `units`, and only the identity hash separates them.
    counts: optionally fewer detections in some frames (a random subset of the grid). Returns (dets, H, W)."""
    rng = np.random.default_rng(seed)
    H, W = (ny + 1) * pitch, (nx + F + 1) * pitch
    dets = []
    for t in range(F):
        ix, iy = np.meshgrid(np.arange(nx), np.arange(ny))
        keep = rng.permutation(nx * ny)[:(nx * ny if counts is None else counts[t])]
        dets.append(_frame(rng, (pitch // 2 + (ix.reshape(-1) + t) * pitch)[keep], (pitch // 2 + iy.reshape(-1) * pitch)[keep]))
    return dets, H, W


def on_mask(F, counts, mask, clusters, spread, seed=0):
    """A clustered scene whose detections sit on the mask (the nearest mask cells to clustered draws)."""
    rng = np.random.default_rng(seed)
    H, W = mask.shape
    ys, xs = np.nonzero(mask)
    cx, cy = rng.integers(spread, W - spread, clusters), rng.integers(spread, H - spread, clusters)
    dets = []
    for n in counts:
        k = rng.integers(0, clusters, n)
        px, py = cx[k] + rng.integers(-spread, spread + 1, n), cy[k] + rng.integers(-spread, spread + 1, n)
        near = np.array([np.argmin(np.abs(xs - a) + np.abs(ys - b)) for a, b in zip(px, py)], np.int64).reshape(-1)
        dets.append(_frame(rng, xs[near], ys[near]))
    return dets


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """One battery case: name, cap, counts, costs {(t, gap): matrix}, max_gap, the path its name claims (`claims`:
    list of dict(slots=, cached=) a gap-1 pair of the case must land in, NC following from cap) and how to run it:
    kind 'geo' (dets, H, W, conn8, mask) or 'ctab'."""

    def __init__(self, name, cap, kind, costs_fn, counts, claims=(), crowded=True, gap2=False, max_gap=2, thr_units=THR_UNITS, **kw):
        self.name, self.cap, self.kind, self._costs_fn, self.counts = name, cap, kind, costs_fn, [int(c) for c in counts]
        self.claims, self.crowded, self.gap2, self.max_gap, self.thr_units = list(claims), crowded, gap2, max_gap, thr_units
        self.__dict__.update(kw)
        assert max(self.counts) <= cap

    @functools.cached_property
    def costs(self):
        return self._costs_fn()

    @functools.cached_property
    def reference(self):
        return reference_from_costs(self.costs, self.counts, self.thr_units, self.max_gap)

    def __repr__(self):
        return self.name


def _geo(name, cap, dets, H, W, conn8=False, mask=None, **kw):
    return Case(name + ('_conn8' if conn8 else ''), cap, 'geo', lambda: geometric_costs(dets, H, W, mask, conn8),
                [len(d[0]) for d in dets], dets=dets, H=H, W=W, conn8=conn8, mask=mask, **kw)


@functools.lru_cache(None)
def battery_a():
    """Geometric costs on the open grid. Counts dip in some frame so that pass 2 is crowded too; several cases hold an
    empty frame in the middle and an empty last frame."""
    c0 = first_cap_without_cache()
    cases = []
    for conn8 in (False, True):
        s = 1000 * conn8
        cases += [
            _geo('a64', 64, clustered(8, [60, 60, 38, 60, 0, 57, 64, 0], 300, 300, 3, 60, 1 + s), 300, 300, conn8,
                 claims=[dict(slots=1, cached=True)], gap2=True),
            _geo('a144_two_slots', 144, clustered(6, [100, 104, 70, 90, 128, 90], 512, 512, 4, 60, 2 + s), 512, 512, conn8,
                 claims=[dict(slots=2, cached=False), dict(slots=2, cached=True)], gap2=True),
            _geo('a192_three_slots', 192, clustered(6, [180, 180, 130, 180, 192, 176], 1024, 1024, 3, 60, 3 + s), 1024, 1024, conn8,
                 claims=[dict(slots=3, cached=False)], gap2=True),
            _geo('a192_alternating', 192, alternating(7, 180, 20, 1024, 1024, 3, 60, 4 + s), 1024, 1024, conn8,
                 claims=[dict(slots=3, cached=False, n_max=20), dict(slots=1, cached=False, n_min=129), dict(slots=1, cached=True)]),
            _geo('a193_nc9_cached', 193, clustered(6, [90, 90, 60, 90, 96, 88], 512, 512, 3, 60, 5 + s), 512, 512, conn8,
                 claims=[dict(cached=True)], gap2=True),
            _geo('a193_nc9_uncached', 193, clustered(5, [190, 193, 140, 190, 185], 1024, 1024, 3, 60, 6 + s), 1024, 1024, conn8,
                 claims=[dict(cached=False)], gap2=True),
            _geo('a576_nc9_cached', 576, clustered(7, [90, 92, 0, 90, 60, 96, 0], 512, 512, 3, 60, 7 + s), 512, 512, conn8,
                 claims=[dict(cached=True)], gap2=True),
            _geo('a576_nc9_deep', 576, clustered(5, [500, 500, 350, 500, 576], 1024, 1024, 5, 60, 8 + s), 1024, 1024, conn8,
                 claims=[dict(cached=False)], gap2=True),
            _geo('a577_nc0', 577, clustered(6, [500, 577, 90, 80, 500, 400], 1024, 1024, 5, 60, 9 + s), 1024, 1024, conn8,
                 claims=[dict(cached=False), dict(cached=True)]),
            _geo('a1304_nc0', 1304, clustered(5, [700, 650, 90, 96, 700], 1024, 1024, 6, 60, 10 + s), 1024, 1024, conn8,
                 claims=[dict(cached=False), dict(cached=True)]),
            _geo(f'a{c0}_no_cache', c0, clustered(7, [700, 700, 500, 700, 96, 90, 0], 1024, 1024, 6, 60, 11 + s), 1024, 1024, conn8,
                 claims=[dict(cached=False, n_max=96, m_max=96), dict(cached=False, n_min=500)], gap2=True),
            _geo('a2048_no_cache', 2048, clustered(6, [700, 720, 500, 700, 90, 80], 1024, 1024, 6, 60, 12 + s), 1024, 1024, conn8,
                 claims=[dict(cached=False, n_max=96, m_max=96), dict(cached=False, n_min=500)], gap2=True),
        ]
    for cap, seed in ((c0, 13), (2048, 14)):
        rng = np.random.default_rng(seed)
        dets = [_frame(rng, rng.integers(0, 1024, n), rng.integers(0, 1024, n)) for n in (10, 12, 0, 9, 11, 0)]
        cases.append(_geo(f'a{cap}_sparse', cap, dets, 1024, 1024, crowded=False, claims=[dict(cached=False)]))
    for cap, (nx, ny), cnt, seed in ((192, (15, 12), [180, 180, 100, 180, 180], 15), (576, (24, 20), [480, 480, 260, 480, 480], 16)):
        dets, H, W = lattice(5, nx, ny, 40, cnt, seed)
        cases.append(_geo(f'a{cap}_lattice', cap, dets, H, W, gap2=True, lattice=True,
                          claims=[dict(slots=3, cached=False)] if cap == 192 else [dict(cached=False)]))
    return cases


CTAB_CAPS = (64, 192, 576, 640)
CTAB_PATTERNS = ('dense', 'machol_wien', 'equal', 'no_link', 'one_row_per_column')


def _ctab_costs(pattern, counts, seed, thr_units=THR_UNITS):
    """Costs of the documented form arc_cost_int(units / 1e6, 3, a, b) for one pattern of `units`."""
    rng = np.random.default_rng(seed)
    offs = offsets(counts)
    out = {}
    for g in (1, 2):
        for t in range(len(counts) - g):
            n, m = counts[t], counts[t + g]
            i, j = np.arange(n)[:, None], np.arange(m)[None, :]
            adm = np.ones((n, m), bool)
            if pattern == 'dense':
                units = rng.integers(1000, thr_units, (n, m))
            elif pattern == 'machol_wien':          # c = (i+1)(j+1): the longest augmenting paths there are
                units = (i + 1) * (j + 1) * ((thr_units - 1) // max(n * m, 1))
            elif pattern == 'equal':                # equal units in a band of columns around the row: only the hash decides
                units = np.full((n, m), 300000)
                adm = np.abs(i * max(m, 1) // max(n, 1) - j) <= 3
            elif pattern == 'no_link':
                units, adm = np.zeros((n, m), np.int64), np.zeros((n, m), bool)
            elif pattern == 'one_row_per_column':   # every column admitted for exactly one row (rows own several when m > n)
                units = rng.integers(1000, thr_units, (n, m))
                owner = rng.permutation(np.arange(m) % max(n, 1)) if n else np.zeros(m, np.int64)
                adm = i == owner[None, :]
            elif pattern == 'above_dummy':          # some admitted links cost more than leaving the row unlinked
                units = rng.integers(1000, 2 * thr_units, (n, m))
            else:
                raise ValueError(pattern)
            cost = arc_cost_vec(np.broadcast_to(units, (n, m)), 3, offs[t] + i, offs[t + g] + j)
            out[(t, g)] = np.where(adm, cost, NO_LINK)
    return out


@functools.lru_cache(None)
def battery_b():
    """Given cost tables. Three frames; the middle one smaller, so that pass 2 has rows and columns left."""
    cases = []
    for cap in CTAB_CAPS:
        counts = [cap - 2, int(0.6 * cap), cap]
        for p, pattern in enumerate(CTAB_PATTERNS):
            for max_gap in (1, 2):
                cases.append(Case(f'b{cap}_{pattern}_gap{max_gap}', cap, 'ctab',
                                  functools.partial(_ctab_costs, pattern, counts, 100 * cap + p), counts, max_gap=max_gap,
                                  crowded=pattern in ('dense', 'machol_wien', 'equal'), pattern=pattern))
    for cap in (64, 576):
        counts = [cap - 2, int(0.6 * cap), cap]
        cases.append(Case(f'b{cap}_above_dummy', cap, 'ctab', functools.partial(_ctab_costs, 'above_dummy', counts, 7 + cap),
                          counts, crowded=True, pattern='above_dummy'))
    return cases


@functools.lru_cache(None)
def battery_c():
    """Masked grid: crowded scenes on synth.corridor_mask (24-px corridors on an 80-px lattice)."""
    from axtrack_amd import synth
    H, W = 256, 320
    mask = synth.corridor_mask(H, W, width=24, pitch=80)
    return [
        _geo('c192_masked_three_slots', 192, on_mask(4, [150, 160, 110, 150], mask, 2, 50, 21), H, W, mask=mask,
             claims=[dict(slots=3, cached=False)], gap2=True),
        _geo('c256_masked_nc9', 256, on_mask(4, [200, 210, 150, 200], mask, 2, 50, 22), H, W, mask=mask,
             claims=[dict(cached=False)], gap2=True),
    ]


def all_cases():
    return battery_a() + battery_b() + battery_c()


# ------------------------------------------------------------------------------------------------ chain numbering alone
def chain_walk(count, cap, pred1, pred2):
    """Track table of hand-made links: every slot walks back to its root (over pred1 where there is one, else pred2), the
    roots are numbered in slot order. pred1 / pred2 i32 [F, cap]: index in frame t-1 / t-2, or -1. Returns (track, n)."""
    F = len(count)
    s = np.arange(F * cap)
    t, i = s // cap, s % cap
    valid = i < np.minimum(np.asarray(count), cap)[t]
    p1, p2 = np.asarray(pred1).reshape(-1), np.asarray(pred2).reshape(-1)
    by1 = valid & (t >= 1) & (p1 >= 0)
    by2 = valid & ~by1 & (t >= 2) & (p2 >= 0)
    parent = np.where(by1, (t - 1) * cap + p1, np.where(by2, (t - 2) * cap + p2, s))
    root = parent
    for _ in range(F):                      # a chain has fewer than F links
        root = parent[root]
    ids = np.cumsum(valid & (root == s)) - 1
    return np.where(valid, ids[root], -1).astype(np.int32).reshape(F, cap), int(ids[-1] + 1) if len(ids) else 0


def chain_scene(F, cap, kind, seed=0):
    """(count, pred1, pred2) for the chain numbering alone. kind: 'spanning' (every detection of frame 0 starts a chain
    through all frames, gaps alternating 1 and 2, the skipped detections roots of their own), 'roots' (no links), 'single'
    (one chain through every frame, everything else roots), 'holes' (spanning, with count 0 in some frames)."""
    rng = np.random.default_rng(seed)
    count = np.full(F, cap, np.int32)
    if kind == 'holes':
        count[2::5] = 0
    elif kind != 'roots':
        count[1::3] = max(cap - 3, 1)
    pred1 = np.full((F, cap), -1, np.int32)
    pred2 = np.full((F, cap), -1, np.int32)
    if kind == 'roots':
        return count, pred1, pred2
    n_chain = 1 if kind == 'single' else int(min(count[count > 0].min(), cap))
    cur_t, cur = 0, rng.permutation(int(count[0]))[:n_chain] if count[0] else None
    step = 1
    while cur is not None:
        nt = cur_t + step
        if nt < F and count[nt] == 0:           # step over an empty frame if a gap of 2 allows it
            nt = cur_t + 2 if step == 1 else F
        if nt >= F or count[nt] == 0:
            break
        nxt = rng.permutation(int(count[nt]))[:n_chain]
        (pred1 if nt - cur_t == 1 else pred2)[nt, nxt] = cur
        cur_t, cur, step = nt, nxt, 3 - step
    return count, pred1, pred2
