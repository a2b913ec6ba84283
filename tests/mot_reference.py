"""CPU reference of the device tracking scorer (csrc/mot.hip) and the scenes its tests share. No product
code except axtrack_amd.mot_metrics (pair_cost_int, and accumulate for the tie-free check). Step 2 is solved by SciPy in
f64 where that is exact and by solve_int -- int64, any size, its answer certified by its own duals -- beyond;
limit_cases() holds the scenes at the stated limits and on both sides of every route threshold, with their route facts.

A scene is a dict of numpy arrays in the layout of axt_mot_scores: x, y i32 [F,cap], count i32 [F], tracks i32 [K,F,cap],
gid, gx, gy i32 [F,gcap], gcount i32 [F], and no, nh, max_dist."""
import functools

import numpy as np
from scipy.optimize import linear_sum_assignment

from axtrack_amd import mot_metrics as mm

KINDS = {1: 'MATCH', 2: 'SWITCH', 3: 'MISS'}
RULES = ('exclusive_threshold', 'clear_on_miss', 'sum_before_cardinality', 'higher_slot_wins', 'fragment_outside_span')


def make_scene(labels, dets, tracks, max_dist=23, no=None, nh=None):
    """labels: per frame a list of (identity, x, y); dets: per frame a list of (x, y); tracks: K lists, per frame the
    track identity of every detection slot (-1 = none)."""
    F = len(labels)
    gcap = max([len(l) for l in labels] + [1]); cap = max([len(d) for d in dets] + [1])
    s = dict(x=np.zeros((F, cap), np.int32), y=np.zeros((F, cap), np.int32), count=np.zeros(F, np.int32),
             tracks=np.full((len(tracks), F, cap), -1, np.int32), gid=np.zeros((F, gcap), np.int32),
             gx=np.zeros((F, gcap), np.int32), gy=np.zeros((F, gcap), np.int32), gcount=np.zeros(F, np.int32),
             max_dist=int(max_dist))
    for f in range(F):
        s['gcount'][f] = len(labels[f]); s['count'][f] = len(dets[f])
        for i, (g, a, b) in enumerate(labels[f]):
            s['gid'][f, i], s['gx'][f, i], s['gy'][f, i] = g, a, b
        for j, (a, b) in enumerate(dets[f]):
            s['x'][f, j], s['y'][f, j] = a, b
        for k, tr in enumerate(tracks):
            assert len(tr[f]) == len(dets[f])
            s['tracks'][k, f, :len(tr[f])] = tr[f]
    s['no'] = int(no if no is not None else max([g for l in labels for g, _, _ in l] + [0]) + 1)
    s['nh'] = int(nh if nh is not None else max(int(s['tracks'].max()) + 1, 1))
    return s


IDENTITY_LDS_LIMIT = 64 * 1024         # csrc/mot.hip: the identity matching keeps its state in LDS up to this size


def identity_state_bytes(no, nh):
    """Bytes of the identity matching's solver state (lsap_bytes of csrc/mot.hip: duals and distances i64, four i32
    arrays padded to an even length, one flag byte per column padded to 8)."""
    even = lambda v: v + (v & 1)
    return 8 * no + 16 * nh + 8 * even(nh) + 8 * even(no) + ((nh + 7) & ~7)


def scratch_bytes(no, nh):
    """Scratch of one association: co i32 [no, nh], partner i32 [no], fragmentation state u8 [no] (each padded to 8) and
    the identity matching's state where it does not fit into LDS."""
    pad = lambda v: (v + 7) & ~7
    state = identity_state_bytes(no, nh)
    return pad(4 * no * nh) + pad(4 * no) + pad(no) + (state if state > IDENTITY_LDS_LIMIT else 0)


def f64_is_exact(cost, ok, sum_first=False):
    """The guard of the SciPy route: every total of the padded f64 problem stays below 2^53."""
    cmax = int(cost[ok].max())
    big = (cmax + 1) if sum_first else (min(cost.shape) + 1) * (cmax + 1)
    return min(cost.shape) * big < 2 ** 53


def _solve_f64(cost, ok, sum_first=False):
    """As many admissible pairs as possible first, then the smallest integer sum; exact in f64 (asserted)."""
    cmax = int(cost[ok].max())
    big = (cmax + 1) if sum_first else (min(cost.shape) + 1) * (cmax + 1)
    assert f64_is_exact(cost, ok, sum_first), 'totals would not be exact in f64'
    r, c = linear_sum_assignment(np.where(ok, cost, big).astype(np.float64))
    return [(int(i), int(j)) for i, j in zip(r, c) if ok[i, j]]


PENALTY_SHIFT = 42                     # csrc/mot.hip: P = (min(rows, cols) + 1) << 42, above every admissible total
RANGE_LIMIT = 1 << 62                  # no intermediate of solve_int may reach this (the kernel argues < 2^63)


def solve_int(cost, ok, dummy):
    """The definition of step 2 in exact integers, for any size: every row takes one admissible column (ok) or its private
    dummy column at `dummy`, no column is taken twice, the sum of the chosen int64 costs is smallest. Shortest augmenting
    paths with potentials: row by row, a Dijkstra search over the columns from the new row to the nearest way out -- a
    free column, or the dummy of any row met on the way -- one numpy pass over the columns per search step.
    -> (col4row i64 [n] (-2: the dummy), u i64 [n], v i64 [m]); (u, v) certify the answer, see certificate_holds."""
    n, m = cost.shape
    u, v = np.zeros(n, np.int64), np.zeros(m, np.int64)
    col4row, row4col = np.full(n, -1, np.int64), np.full(m, -1, np.int64)
    for i in range(n):
        dist = np.full(m, RANGE_LIMIT, np.int64)           # length of the shortest alternating path to the column
        pred = np.full(m, -1, np.int64)
        done = np.zeros(m, bool)
        seen, seen_at = [i], [0]                            # rows of the search tree and their distance
        cur, d, out, out_row = i, 0, RANGE_LIMIT, -1
        while True:
            leave = d + dummy - int(u[cur])                 # out through cur's own dummy
            assert 0 <= leave < RANGE_LIMIT
            if leave < out:
                out, out_row = leave, cur
            red = (cost[cur] - u[cur]) - v + d
            assert -RANGE_LIMIT < int(red.min()) and int(red.max()) < RANGE_LIMIT, 'an intermediate reached 2^62'
            better = ok[cur] & ~done & (red < dist)
            dist[better] = red[better]
            pred[better] = cur
            open_dist = np.where(done, RANGE_LIMIT, dist)
            j = int(open_dist.argmin())
            if out <= int(open_dist[j]):
                total, sink = out, -2
                break
            d = int(open_dist[j])
            done[j] = True
            if row4col[j] < 0:
                total, sink = d, j
                break
            cur = int(row4col[j])
            seen.append(cur); seen_at.append(d)
        u[seen] += total - np.array(seen_at, np.int64)
        v[done] -= total - dist[done]
        assert int(np.abs(u).max()) < RANGE_LIMIT and int(np.abs(v).max()) < RANGE_LIMIT, 'a dual reached 2^62'
        r, jnew = (out_row, -2) if sink == -2 else (int(pred[sink]), sink)
        while True:                                        # flip the path back to row i
            jprev = int(col4row[r])
            col4row[r] = jnew
            if jnew >= 0:
                row4col[jnew] = r
            if r == i:
                break
            jnew, r = jprev, int(pred[jprev])
    return col4row, u, v


def certificate_holds(cost, ok, dummy, col4row, u, v):
    """Optimality of col4row proved from the duals alone, O(n m): the assignment is feasible; every admissible pair and
    every dummy has a reduced cost >= 0 (cost - u[i] - v[j], dummy - u[i]; a private dummy column has dual 0); v <= 0, and
    = 0 on the columns nobody took; every chosen pair or dummy has reduced cost 0. Then every feasible assignment costs
    at least sum(u) + sum(v), and this one costs exactly that."""
    n, m = cost.shape
    col4row = np.asarray(col4row, np.int64)
    real = col4row >= 0
    rows, cols = np.nonzero(real)[0], col4row[real]
    if not ((col4row == -2) | real).all() or (cols >= m).any() or len(set(cols.tolist())) != len(cols):
        return False
    if not ok[rows, cols].all():
        return False
    red = cost - u[:, None] - v[None, :]
    free = np.ones(m, bool); free[cols] = False
    return bool((red[ok] >= 0).all() and (dummy - u >= 0).all() and (v <= 0).all() and (v[free] == 0).all()
                and (red[rows, cols] == 0).all() and (dummy - u[~real] == 0).all())


def _solve(cost, ok, sum_first=False, solver=None):
    """Step 2 of one frame -> (pairs, facts about the solve). solver: 'f64' (SciPy, asserted exact), 'int' (solve_int with
    its certificate) or None: SciPy wherever its guard holds -- and for the broken sum-first model -- else solve_int."""
    if not ok.any():
        return [], dict(solver='none', max_dual=0)
    if solver is None:
        solver = 'f64' if sum_first or f64_is_exact(cost, ok) else 'int'
    if solver == 'f64':
        return _solve_f64(cost, ok, sum_first), dict(solver='f64', max_dual=0)
    assert not sum_first
    dummy = (min(cost.shape) + 1) << PENALTY_SHIFT
    col4row, u, v = solve_int(cost, ok, dummy)
    assert certificate_holds(cost, ok, dummy, col4row, u, v), 'solve_int: the duals do not certify its answer'
    return ([(int(i), int(j)) for i, j in enumerate(col4row) if j >= 0],
            dict(solver='int', max_dual=max(int(np.abs(u).max()), int(np.abs(v).max()))))


def reference(s, k=0, broken=None, solver=None):
    """The definition on the CPU for association k. -> dict(counts i64 [10], tallies i64 [no,2], events set of
    (frame, kind, label slot, partner slot), fp set of (frame, slot), id_events set of (frame, kind, label identity,
    track identity), co i64 [no,nh], claimants: frames in which two labels claimed one remembered partner, claims: per
    such frame the label slots of every shared claim, step1: per frame the (label slot, detection slot) pairs kept,
    step2: per frame in which step 2 ran dict(nr, nc, pairs (label slot, detection slot), cost: their integer total,
    hash_sum, n_dummy, solver, max_dual), matched_d2, refused_d2: the d2 of matched / of inadmissible live pairs (the
    smallest of the latter), max_ok_d2). The counts are clamped as the kernels clamp them: max(min(count, cap), 0)."""
    assert broken is None or broken in RULES
    no, nh, md2 = s['no'], s['nh'], s['max_dist'] ** 2
    partner = np.full(no, -1, np.int64)
    state = np.zeros(no, np.int64)                 # 0 never tracked, 1 tracked last, 2 in a miss run after it
    tallies = np.zeros((no, 2), np.int64)
    co = np.zeros((no, nh), np.int64)
    c = dict.fromkeys(mm.MOT_COUNTS, 0)
    events, fps, id_events, claim_frames = set(), set(), set(), []
    claims, step1, step2, matched_d2, refused_d2, max_ok_d2 = {}, {}, {}, set(), None, -1
    cap, gcap = s['x'].shape[1], s['gid'].shape[1]
    for f in range(len(s['count'])):
        ng, nd = max(min(int(s['gcount'][f]), gcap), 0), max(min(int(s['count'][f]), cap), 0)
        lab = [(i, int(s['gid'][f, i])) for i in range(ng) if 0 <= s['gid'][f, i] < no]
        hyp = [(j, int(s['tracks'][k, f, j])) for j in range(nd) if 0 <= s['tracks'][k, f, j] < nh]
        li = np.array([i for i, _ in lab], np.int64); g = np.array([v for _, v in lab], np.int64)
        hj = np.array([j for j, _ in hyp], np.int64); h = np.array([v for _, v in hyp], np.int64)
        dx = s['gx'][f, li].astype(np.int64)[:, None] - s['x'][f, hj].astype(np.int64)[None, :]
        dy = s['gy'][f, li].astype(np.int64)[:, None] - s['y'][f, hj].astype(np.int64)[None, :]
        d2 = dx * dx + dy * dy
        ok = d2 < md2 if broken == 'exclusive_threshold' else d2 <= md2
        oa, ob = np.nonzero(ok)
        np.add.at(co, (g[oa], h[ob]), 1)
        if ok.any():
            max_ok_d2 = max(max_ok_d2, int(d2[ok].max()))
        if (~ok).any():
            refused_d2 = min(int(d2[~ok].min()), refused_d2 if refused_d2 is not None else 1 << 62)
        c['n_obj'] += len(lab); c['n_pred'] += len(hyp)
        tallies[g, 0] += 1
        kind = np.zeros(len(lab), np.int64); part = np.full(len(lab), -1, np.int64)
        h_done = np.zeros(len(hyp), bool)
        # 1. remembered partners
        want = {}
        for a in range(len(lab)):
            b = np.nonzero(h == partner[g[a]])[0] if partner[g[a]] >= 0 else []
            if len(b) and ok[a, b[0]]:
                want.setdefault(int(b[0]), []).append(a)
        if any(len(v) > 1 for v in want.values()):
            claim_frames.append(f)
            claims[f] = [[int(li[a]) for a in v] for v in want.values() if len(v) > 1]
        for b, claimants in want.items():
            a = max(claimants) if broken == 'higher_slot_wins' else min(claimants)
            kind[a], part[a], h_done[b] = 1, b, True
        step1[f] = {(int(li[a]), int(hj[part[a]])) for a in np.nonzero(kind == 1)[0]}
        # 2. the rest, exactly
        rows, cols = np.nonzero(kind == 0)[0], np.nonzero(~h_done)[0]
        if len(rows) and len(cols):
            cost = mm.pair_cost_int(d2[np.ix_(rows, cols)], g[rows][:, None], h[cols][None, :])
            pairs, info = _solve(cost, ok[np.ix_(rows, cols)], broken == 'sum_before_cardinality', solver)
            step2[f] = dict(info, nr=len(rows), nc=len(cols), pairs=[(int(li[rows[r]]), int(hj[cols[q]])) for r, q in pairs],
                            cost=sum(int(cost[r, q]) for r, q in pairs), hash_sum=sum(int(cost[r, q]) & 0xFFFF for r, q in pairs),
                            n_dummy=len(rows) - len(pairs))
            for r, q in pairs:
                a, b = rows[r], cols[q]
                kind[a] = 2 if partner[g[a]] >= 0 and partner[g[a]] != h[b] else 1
                part[a], h_done[b] = b, True
                partner[g[a]] = h[b]
        # 3. misses, false positives, tallies
        for a in range(len(lab)):
            if kind[a] == 0:
                kind[a] = 3
                c['n_miss'] += 1
                if broken == 'clear_on_miss':
                    partner[g[a]] = -1
                if state[g[a]] == 1:
                    state[g[a]] = 2
                    c['n_fragmentations'] += broken == 'fragment_outside_span'
            else:
                c['n_match' if kind[a] == 1 else 'n_switch'] += 1
                c['sum_d2'] += int(d2[a, part[a]])
                matched_d2.add(int(d2[a, part[a]]))
                tallies[g[a], 1] += 1
                c['n_fragmentations'] += state[g[a]] == 2 and broken != 'fragment_outside_span'
                state[g[a]] = 1
            events.add((f, int(kind[a]), int(li[a]), int(hj[part[a]]) if part[a] >= 0 else -1))
            id_events.add((f, KINDS[int(kind[a])], int(g[a]), int(h[part[a]]) if part[a] >= 0 else -1))
        for b in np.nonzero(~h_done)[0]:
            c['n_fp'] += 1
            fps.add((f, int(hj[b])))
            id_events.add((f, 'FP', -1, int(h[b])))
    c['n_unique_objects'] = int((tallies[:, 0] > 0).sum())
    r, q = linear_sum_assignment(-co)
    c['idtp'] = int(co[r, q].sum())
    return dict(counts=np.array([c[n] for n in mm.MOT_COUNTS], np.int64), tallies=tallies, events=events, fp=fps,
                id_events=id_events, co=co, claimants=claim_frames, claims=claims, step1=step1, step2=step2,
                matched_d2=matched_d2, refused_d2=refused_d2, max_ok_d2=max_ok_d2)


def accumulate_frames(s, k=0):
    """The scene as mot_metrics.accumulate's input (identities: the dense label identity, the track identity)."""
    out = []
    for f in range(len(s['count'])):
        ng, nd = int(s['gcount'][f]), int(s['count'][f])
        sel = np.nonzero(s['tracks'][k, f, :nd] >= 0)[0]
        out.append((s['gid'][f, :ng].astype(np.int64), np.stack([s['gx'][f, :ng], s['gy'][f, :ng]], 1).astype(np.float64),
                    s['tracks'][k, f, sel].astype(np.int64), np.stack([s['x'][f, sel], s['y'][f, sel]], 1).astype(np.float64)))
    return out


def host_events(s, k=0):
    ev = mm.accumulate(accumulate_frames(s, k), float(s['max_dist']) ** 2)
    return ev, set(zip(ev['frame'].tolist(), ev['kind'].tolist(), ev['obj'].tolist(), ev['hyp'].tolist()))


def is_tie_free(s, k=0):
    """The reference on integer costs and mot_metrics.accumulate on floats agree event for event."""
    return reference(s, k)['id_events'] == host_events(s, k)[1]


# ------------------------------------------------------------------ named cases
def _walk_scene(seed, F, n, spacing=60, jitter=3, drop=0.1, extra=2):
    """n objects on a grid drifting slowly; detections = the objects (some dropped) plus a few strays, slot order
    shuffled per frame; returns (positions [F,n,2], dets per frame, true identity per slot)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    pos = np.stack([(np.arange(n) % side) * spacing + 40, (np.arange(n) // side) * spacing + 40], 1)[None].repeat(F, 0)
    pos = pos + np.cumsum(rng.integers(-jitter, jitter + 1, (F, n, 2)), 0)
    dets, ident = [], []
    for f in range(F):
        keep = np.nonzero(rng.random(n) >= drop)[0]
        pts = [(int(pos[f, o, 0]), int(pos[f, o, 1]), int(o)) for o in keep]
        pts += [(int(a), int(b), -1) for a, b in rng.integers(0, side * spacing + 80, (extra, 2))]
        order = rng.permutation(len(pts))
        dets.append([(pts[q][0], pts[q][1]) for q in order])
        ident.append([pts[q][2] for q in order])
    return pos, dets, ident


def _track_variants(ident, seed):
    """Three track tables of one scene: the true identities; identities exchanged in pairs from the middle frame on;
    a new identity every three frames with some detections left without one."""
    rng = np.random.default_rng(seed)
    F = len(ident)
    n = max([max(i + [-1]) for i in ident]) + 1
    swap = np.arange(n); swap[:n - n % 2] = swap[:n - n % 2].reshape(-1, 2)[:, ::-1].reshape(-1)
    t0 = [list(i) for i in ident]
    t1 = [[(int(swap[o]) if f >= F // 2 else o) if o >= 0 else -1 for o in i] for f, i in enumerate(ident)]
    t2 = [[(o + n * (f // 3) if rng.random() > 0.15 else -1) if o >= 0 else -1 for o in i] for f, i in enumerate(ident)]
    return [t0, t1, t2]


def _lane_case(n_lab, n_hyp, seed, bump=1000, second_table=False):
    """n_lab labels and n_hyp detections on a 15 px grid (every label reaches several detections), three frames, slot
    order shuffled: lane strides of the claim, the compaction and the searches. In the last frame every seventh track
    has a new identity (+ bump); second_table adds an association with the identities counted from the other end."""
    rng = np.random.default_rng(seed)
    n = max(n_lab, n_hyp)
    side = int(np.ceil(np.sqrt(n)))
    base = np.stack([(np.arange(n) % side) * 15, (np.arange(n) // side) * 15], 1) + 30
    labels, dets, tr = [], [], []
    for f in range(3):
        lo = rng.permutation(n_lab)
        labels.append([(int(o), int(base[o, 0]), int(base[o, 1])) for o in lo])
        ho = rng.permutation(n_hyp)
        jit = rng.integers(-4, 5, (n, 2))
        dets.append([(int(base[o, 0] + jit[o, 0]), int(base[o, 1] + jit[o, 1])) for o in ho])
        tr.append([int(o) + (bump if f == 2 and o % 7 == 0 else 0) for o in ho])
    top = max(max(fr) for fr in tr)
    return make_scene(labels, dets, [tr, [[top - t for t in fr] for fr in tr]] if second_table else [tr])


@functools.lru_cache(maxsize=None)
def named_cases():
    L, D = [], []
    c = {}
    c['empty_labels'] = make_scene([[], []], [[(5, 5), (50, 50)], [(6, 5)]], [[[0, 1], [0]]])
    c['empty_detections'] = make_scene([[(0, 5, 5)], [(0, 6, 5), (1, 90, 90)]], [[], []], [[[], []]])
    c['both_empty'] = make_scene([[], []], [[], []], [[[], []]])
    c['empty_frame_between'] = make_scene([[(0, 5, 5)], [], [(0, 7, 5)]], [[(5, 6)], [], [(7, 6)]], [[[0], [], [0]]])
    c['threshold'] = make_scene([[(0, 0, 0), (1, 100, 100)]], [[(23, 0), (123, 101)]], [[[0, 1]]])
    c['kept_partner'] = make_scene([[(0, 0, 0)], [(0, 0, 0)]], [[(5, 0)], [(1, 0), (10, 0)]], [[[0], [1, 0]]])
    # identity 0 pairs with track 0, then identity 1 does (0 is absent), then both stand next to it; label slots: 1 first
    c['shared_partner'] = make_scene([[(0, 0, 0)], [(1, 10, 0)], [(1, 10, 0), (0, 0, 0)]],
                                     [[(1, 0)], [(9, 0)], [(5, 0), (12, 3)]], [[[0], [0], [0, 1]]])
    c['switch_after_miss'] = make_scene([[(0, 0, 0)], [(0, 0, 0)], [(0, 0, 0)]], [[(1, 0)], [(200, 0)], [(2, 0)]],
                                        [[[0], [0], [1]]])
    c['cardinality'] = make_scene([[(0, 0, 0), (1, 1, 15)]], [[(1, 0), (-20, 0)]], [[[0, 1]]])
    pattern = 'MTMMTMTMM'                                 # miss runs before, inside (two) and after the tracked span
    c['fragmentation'] = make_scene([[(0, 0, 0)]] * len(pattern), [[(1, 1) if p == 'T' else (300, 300)] for p in pattern],
                                    [[[0]] * len(pattern)])
    for n_lab, n_hyp in ((63, 65), (64, 64), (65, 63), (129, 129)):
        c[f'lanes_{n_lab}x{n_hyp}'] = _lane_case(n_lab, n_hyp, n_lab)
    pos, dets, ident = _walk_scene(5, 9, 65)
    labels = [[(o, int(pos[f, o, 0]) + 1, int(pos[f, o, 1])) for o in range(65) if (o + f) % 11] for f in range(9)]
    c['identities_65_k3'] = make_scene(labels, dets, _track_variants(ident, 6), no=70)
    # the same with track identities from 3000 on: the identity matching's state no longer fits into LDS
    far = [[[t + 3000 if t >= 0 else -1 for t in fr] for fr in tr] for tr in _track_variants(ident, 6)]
    c['identity_state_in_scratch_k3'] = make_scene(labels, dets, far, no=70)
    # exact ties: labels midway between two detections, on a dense lattice
    rng = np.random.default_rng(8)
    labels, dets, tr = [], [], []
    for f in range(4):
        pts = [(20 * a, 20 * b) for a in range(6) for b in range(5)]
        order = rng.permutation(len(pts))
        dets.append([pts[q] for q in order]); tr.append([int(q) for q in order])
        labels.append([(i, 20 * (i % 5) + 10, 20 * (i // 5) + (10 if f % 2 else 0)) for i in rng.permutation(20)])
    c['dense_ties'] = make_scene(labels, dets, [tr])
    return c


def hand_cases():
    """The seven hand cases of tests/test_mot_metrics.py as scenes: (gt, hyp, n_frames) of {id: {frame: (x, y)}}."""
    line = {f: (10 * f, 0) for f in range(5)}
    g1 = {1: {f: (10 * f, 5) for f in range(5)}, 2: {f: (300, 10 * f) for f in range(5)}}
    raw = [
        (g1, {7: g1[1], 8: g1[2]}, 5),
        ({1: line}, {10: {f: (10 * f, 0) for f in range(3)}, 11: {f: (10 * f, 0) for f in (3, 4)}}, 5),
        ({1: line}, {10: {f: (10 * f, 0) for f in (0, 1, 3, 4)}, 99: {2: (400, 400)}}, 5),
        ({1: {0: (0, 0), 1: (0, 0)}, 2: {0: (10, 0), 1: (10, 0)}}, {5: {0: (0, 0), 1: (6, 0)}, 6: {0: (10, 0), 1: (4, 0)}}, 2),
        ({1: {0: (0, 0)}}, {9: {0: (23, 0)}}, 1),
        ({1: {0: (0, 0)}}, {9: {0: (23, 1)}}, 1),
        ({1: {f: (0, 0) for f in range(4)}}, {}, 4),
        ({1: {0: (0, 0), 1: (5, 0), 2: (9, 0)}}, {4: {0: (1, 0), 2: (9, 3), 3: (9, 9)}}, 4),
    ]
    out = []
    for gt, hyp, n in raw:
        dense = {g: r for r, g in enumerate(sorted(gt))}
        labels = [[(dense[g], *p[f]) for g, p in gt.items() if f in p] for f in range(n)]
        hs = [[(h, p[f]) for h, p in hyp.items() if f in p] for f in range(n)]
        out.append(make_scene(labels, [[p for _, p in fr] for fr in hs], [[[h for h, _ in fr] for fr in hs]]))
    return out


@functools.lru_cache(maxsize=None)
def association_scenes():
    """Scenes whose labels are taken from an association of the same detections (the true identities, at the detections'
    own anchors), scored against three other track tables each."""
    out = []
    for seed, F, n in ((1, 12, 9), (2, 10, 40), (3, 8, 70)):
        pos, dets, ident = _walk_scene(seed, F, n)
        labels = [[(o, *dets[f][j]) for j, o in enumerate(ident[f]) if o >= 0] for f in range(F)]
        out.append(make_scene(labels, dets, _track_variants(ident, seed + 10), no=n))
    return out


def tie_free_battery():
    """(scene, k) pairs that are compared with mot_metrics; every one passes is_tie_free (asserted by the CPU tests)."""
    return [(s, 0) for s in hand_cases()] + [(s, k) for s in association_scenes() for k in range(s['tracks'].shape[0])]


INT_SCORES = ['num_unique_objects', 'mostly_tracked', 'partially_tracked', 'mostly_lost', 'num_false_positives',
              'num_misses', 'num_switches', 'num_fragmentations']


def assert_scores_equal(got, want):
    assert list(got.index) == list(want.index) == mm.MOTCHALLENGE_METRICS
    for name in INT_SCORES:
        assert got[name] == want[name], name
    assert np.allclose(got.to_numpy(float), want.to_numpy(float), rtol=0, atol=1e-12, equal_nan=True), (got, want)
    assert (np.isnan(got.to_numpy(float)) == np.isnan(want.to_numpy(float))).all()


# ------------------------------------------------------------------ reading a mismatch
def matching_cost(s, k, f, pairs):
    """Cardinality and integer total of (label slot, detection slot) pairs of frame f under mot_metrics.pair_cost_int;
    a pair that is not admissible makes the total None."""
    total = 0
    for i, j in pairs:
        dx, dy = int(s['gx'][f, i]) - int(s['x'][f, j]), int(s['gy'][f, i]) - int(s['y'][f, j])
        d2 = dx * dx + dy * dy
        if d2 > s['max_dist'] ** 2 or total is None:
            total = None
        else:
            total += int(mm.pair_cost_int(d2, int(s['gid'][f, i]), int(s['tracks'][k, f, j])))
    return len(pairs), total


def explain_mismatch(s, k, ref, events):
    """For a device event log that differs from the reference's: the first frame that differs (the partner table is still
    the same there, so step 1 is), then cardinality and integer cost of the device's step-2 matching, recomputed on the
    host from the log, against the reference's optimum. Equal cost = the scene has a tie (change the scene); fewer pairs
    or a larger cost = the kernel's matching is not the optimum."""
    for f in range(len(s['count'])):
        want, got = {e for e in ref['events'] if e[0] == f}, {e for e in events if e[0] == f}
        if want == got:
            continue
        dev_pairs = {(i, j) for _, kind, i, j in got if kind in (1, 2)} - ref['step1'].get(f, set())
        n, total = matching_cost(s, k, f, sorted(dev_pairs))
        r = ref['step2'].get(f, dict(pairs=[], cost=0))
        verdict = ('a tie: equal cardinality and cost, change the scene' if (n, total) == (len(r['pairs']), r['cost'])
                   else 'the device matching is not the optimum')
        return (f'association {k}, frame {f}: device step 2 has {n} pairs at cost {total}, the reference {len(r["pairs"])} at '
                f'{r["cost"]}: {verdict}; {len(want ^ got)} events differ, e.g. {sorted(want ^ got)[:4]}')
    return f'association {k}: the event logs agree'


# ------------------------------------------------------------------ limit and route cases
# The constants the route facts rest on, restated from the source. A change there sends you back to the cases.
MOT_MAX_SIDE = 1024                    # csrc/mot.hip `constexpr int MOT_MAX_SIDE = 1024`: cap, gcap
MOT_MAX_DIST = 255                     # csrc/mot.hip `constexpr int MOT_MAX_DIST = 255`
MOT_MAX_IDENTITIES = 1 << 24           # csrc/mot.hip axt_mot_scores `no <= (1 << 24) && ... nh <= (1 << 24)`
DEFAULT_DYNAMIC_LDS = 64 * 1024        # csrc/mot.hip axt_mot_scores `axt_max_dynamic_lds(mot_clear_kernel, 160 * 1024, once)`:
#                                        a launch with more dynamic LDS than this needs that attribute
WAVE = 64                              # csrc/mot.hip: `i += 64` in every lane loop of mot_clear_kernel


def lsap_bytes(n, m):
    """csrc/mot.hip lsap_bytes(n, m): `8 * n + 8 * m + 8 * m + 4 * (m + (m & 1)) + 4 * (n + (n & 1)) + 4 * (m + (m & 1)) +
    4 * (n + (n & 1)) + ((m + 7) & ~7)`."""
    even = lambda q: q + (q & 1)
    return 8 * n + 8 * m + 8 * m + 4 * even(m) + 4 * even(n) + 4 * even(m) + 4 * even(n) + ((m + 7) & ~7)


def clear_lds_bytes(gcap, cap):
    """csrc/mot.hip clear_lds_bytes(gcap, cap): `lsap_bytes(gcap, cap) + 4 * (6 * gc2 + 6 * c2) + ((gcap + 7) & ~7) +
    2 * ((cap + 7) & ~7)` with gc2, c2 the sides rounded up to even -- the dynamic LDS of every mot_clear_kernel launch."""
    even = lambda q: q + (q & 1)
    return lsap_bytes(gcap, cap) + 4 * (6 * even(gcap) + 6 * even(cap)) + ((gcap + 7) & ~7) + 2 * ((cap + 7) & ~7)


class LimitCase:
    def __init__(self, name, scene, facts):
        self.name, self.scene, self.facts = name, scene, tuple(facts)

    def __repr__(self):
        return self.name


def _dense_case(n_lab, n_hyp, F, seed, max_dist=255, side=180):
    """Every label within max_dist of every detection (a side x side square: the diagonal of 180 is 254.6 at most), slots
    shuffled, tracks renumbered in every frame so that nobody has a remembered partner and step 2 sees the whole frame."""
    rng = np.random.default_rng(seed)
    labels, dets, tr = [], [], []
    for f in range(F):
        lp, dp = rng.integers(0, side + 1, (n_lab, 2)) + 10, rng.integers(0, side + 1, (n_hyp, 2)) + 10
        labels.append([(int(g), int(a), int(b)) for g, (a, b) in zip(rng.permutation(n_lab), lp)])
        dets.append([(int(a), int(b)) for a, b in dp])
        tr.append([f * n_hyp + int(t) for t in rng.permutation(n_hyp)])
    return make_scene(labels, dets, [tr], max_dist=max_dist)


def _spread_identities(scene, no, nh, seed):
    """The scene with its label and track identities spread over [0, no) and [0, nh), both ends of each range in use."""
    rng = np.random.default_rng(seed)
    n_lab, n_tr = int(scene['gid'].max()) + 1, int(scene['tracks'].max()) + 1
    lmap, tmap = np.sort(rng.choice(no, n_lab, replace=False)), np.sort(rng.choice(nh, n_tr, replace=False))
    lmap[0], lmap[-1], tmap[0], tmap[-1] = 0, no - 1, 0, nh - 1
    s = dict(scene, gid=lmap[scene['gid']].astype(np.int32), no=int(no), nh=int(nh))
    s['tracks'] = np.where(scene['tracks'] >= 0, tmap[np.maximum(scene['tracks'], 0)], -1).astype(np.int32)
    return s


def _walk_k3(seed, F, n, **kw):
    pos, dets, ident = _walk_scene(seed, F, n)
    labels = [[(o, int(pos[f, o, 0]) + 1, int(pos[f, o, 1])) for o in range(n) if (o + f) % 11] for f in range(F)]
    return make_scene(labels, dets, _track_variants(ident, seed + 1), **kw)


def _claimants_case(n=70):
    """Track 0 pairs with a new label identity in each of the first n frames (so all n remember it); the last frame holds
    all n labels within reach of track 0, slots shuffled, and a second detection for one of the losers."""
    rng = np.random.default_rng(70)
    pts = [(100 + 4 * a, 100 + 4 * b) for a in range(-5, 6) for b in range(-5, 6) if 0 < 16 * (a * a + b * b) <= 400][:n]
    assert len(pts) == n
    labels = [[(g, *pts[g])] for g in range(n)] + [[(int(g), *pts[g]) for g in rng.permutation(n)]]
    dets = [[(pts[g][0] + 1, pts[g][1])] for g in range(n)] + [[(100, 100), (108, 101)]]
    return make_scene(labels, dets, [[[0]] * n + [[0, 1]]])


def _ignored_case():
    """Identities outside their range and counts outside [0, cap]: none of it takes part, and every ignored entry is a
    decoy that would pair with a label if it did."""
    no, nh, cap, gcap = 4, 5, 4, 4
    frames = [  # labels (identity, x, y) and detections (track, x, y); the counts are set below
        ([(0, 10, 10), (-1, 50, 10), (1, 90, 10), (no, 130, 10)], [(0, 11, 10), (1, 51, 10), (-2, 91, 10), (2, 131, 10)]),
        ([(0, 10, 10), (no + 5, 50, 10), (1, 90, 10), (2, 130, 10)], [(0, 11, 10), (nh, 91, 10), (nh + 7, 131, 10), (3, 51, 10)]),
        ([(0, 10, 10), (1, 90, 10), (2, 130, 10), (3, 50, 10)], [(0, 12, 10), (1, 92, 10), (2, 132, 10), (3, 52, 10)]),
        ([(0, 10, 10), (1, 90, 10), (2, 130, 10), (3, 50, 10)], [(0, 12, 10), (1, 92, 10), (2, 132, 10), (3, 52, 10)]),
        ([(0, 10, 10), (1, 90, 10), (2, 130, 10), (3, 50, 10)], [(0, 12, 10), (1, 92, 10), (2, 132, 10), (3, 52, 10)]),
        ([(0, 10, 10), (1, 90, 10), (2, 130, 10), (3, 50, 10)], [(0, 12, 10), (4, 92, 10), (2, 132, 10), (3, 52, 10)]),
    ]
    s = make_scene([l for l, _ in frames], [[(a, b) for _, a, b in d] for _, d in frames], [[[t for t, _, _ in d] for _, d in frames]],
                   no=no, nh=nh)
    assert s['x'].shape[1] == cap and s['gid'].shape[1] == gcap
    s['count'][:] = [4, 4, cap + 3, -4, 2, 4]              # frame 4: detections 2 and 3 are decoys beyond the count
    s['gcount'][:] = [4, 4, 4, 4, gcap + 2, 3]             # frame 5: label 3 is a decoy beyond the count
    return s


def _many_associations(K=300):
    """K track tables of one 9-frame walk scene: the true identities with k mod 5 detections left without one (so n_pred of
    neighbours differs) and, from frame (k // 5) % 9 on, the identities of one pair of objects exchanged."""
    F, n = 9, 12
    pos, dets, ident = _walk_scene(21, F, n)
    labels = [[(o, int(pos[f, o, 0]) + 1, int(pos[f, o, 1])) for o in range(n)] for f in range(F)]
    live = [(f, j) for f in range(F) for j, o in enumerate(ident[f]) if o >= 0]
    tables = []
    for k in range(K):
        rng = np.random.default_rng(1000 + k)
        a, b = rng.choice(n, 2, replace=False)
        swap = {int(a): int(b), int(b): int(a)}
        tab = [[(swap.get(o, o) if f >= (k // 5) % F else o) if o >= 0 else -1 for o in fr] for f, fr in enumerate(ident)]
        for q in rng.choice(len(live), k % 5, replace=False):
            tab[live[q][0]][live[q][1]] = -1
        tables.append(tab)
    return make_scene(labels, dets, tables, no=n, nh=n)


# Frames of the three all-admissible cases. They began with 3 each; on the MI355X the square one took 11.4 s with 3 frames
# (9 s of it the identity matching: with every co equal, row i's search walks over all i columns taken before it), the
# other two 3.0 and 2.6 s. A case that is too slow loses frames, never rows or columns.
DENSE_FRAMES = {'dense_1024x1024_md255': 1, 'rows_over_cols_1024x512_md255': 2, 'cols_over_rows_512x1024_md255': 2}


@functools.lru_cache(maxsize=None)
def limit_cases():
    """name -> LimitCase: the scorer at the limits its header states and on both sides of every route threshold, each
    with the route facts it claims (facts_of recomputes them; tests/test_mot_scores_cpu.py compares)."""
    c = {}

    def add(name, scene, *facts):
        c[name] = LimitCase(name, scene, facts)

    int_solver = 'the f64 guard fails: solved in integers'
    add('dense_1024x1024_md255', _dense_case(1024, 1024, DENSE_FRAMES['dense_1024x1024_md255'], 1),
        'cap 1024, gcap 1024, max_dist 255', 'clear LDS 94208 bytes', 'clear LDS above 64 KiB', 'largest min(nr, nc) + 1 = 1025',
        'every frame is full: count = cap, gcount = gcap', 'an admissible d2 >= 60000', int_solver)
    add('rows_over_cols_1024x512_md255', _dense_case(1024, 512, DENSE_FRAMES['rows_over_cols_1024x512_md255'], 2),
        'cap 512, gcap 1024, max_dist 255', 'at least 512 rows end on their dummy in every frame', 'largest dual >= 2^50',
        'clear LDS 68096 bytes', int_solver)
    # no row ends on its dummy here, so the duals stay at the size of a pair cost (< 2^43): the penalty enters the searches
    # (every row's way out through its dummy is weighed) but not the duals
    add('cols_over_rows_512x1024_md255', _dense_case(512, 1024, DENSE_FRAMES['cols_over_rows_512x1024_md255'], 3),
        'cap 1024, gcap 512, max_dist 255', 'at least 512 columns stay free in every frame', 'no row ends on its dummy',
        'largest dual < 2^43', 'clear LDS 73216 bytes', int_solver)
    add('lds_edge_712', _lane_case(712, 712, 712, bump=2000), 'cap 712, gcap 712, max_dist 23', 'clear LDS 65504 bytes',
        'clear LDS within 64 KiB', 'sparse: most pairs are not admissible')
    add('lds_edge_713', _lane_case(713, 713, 713, bump=2000, second_table=True), 'cap 713, gcap 713, max_dist 23',
        'clear LDS 65688 bytes', 'clear LDS above 64 KiB', 'sparse: most pairs are not admissible', 'K 2')
    add('tall_400x1024', _lane_case(400, 1024, 400, bump=2000), 'cap 1024, gcap 400, max_dist 23', 'clear LDS 68624 bytes',
        'clear LDS above 64 KiB')
    add('wide_1024x400', _lane_case(1024, 400, 1024, bump=2000), 'cap 400, gcap 1024, max_dist 23', 'clear LDS 62384 bytes',
        'clear LDS within 64 KiB')
    # (255, 0) -> 65 025 = 255^2 exactly, (180, 180) -> 64 800, (255, 1) -> 65 026; the three groups are out of each other's reach
    add('threshold_255', make_scene([[(0, 0, 0), (1, 0, 300), (2, 0, 700)]], [[(255, 0), (180, 480), (255, 701)]], [[[0, 1, 2]]],
                                    max_dist=255),
        'max_dist 255', 'matched d2 65025', 'matched d2 64800', 'smallest refused d2 65026')
    add('max_dist_0', make_scene([[(0, 5, 5), (1, 40, 40), (2, 80, 80)]] * 2,
                                 [[(5, 5), (40, 41), (80, 80)], [(5, 6), (40, 40), (80, 80)]], [[[0, 1, 2], [0, 1, 2]]], max_dist=0),
        'max_dist 0', 'every matched d2 is 0', 'smallest refused d2 1')
    # labels midway between two detections of their row: every admissible pair at d2 = 25, the only full matching is forced
    lat = [(10 * a + 10, 10 * b + 10) for b in range(32) for a in range(32)]
    rng = np.random.default_rng(1024)
    lo, ho = rng.permutation(1024), rng.permutation(1024)
    add('hash_sum_1024', make_scene([[(int(o), lat[o][0] + 5, lat[o][1]) for o in lo]], [[lat[o] for o in ho]],
                                    [[[int(o) for o in ho]]], max_dist=5),
        'cap 1024, gcap 1024, max_dist 5', 'no 1024, nh 1024', 'every admissible pair at one d2', '1024 pairs chosen in one frame',
        'hash sum of the chosen pairs < 2^26', 'the chosen costs carry more than 2^24 of hash')
    add('identity_lds_exact', _spread_identities(_walk_k3(31, 9, 40), 896, 2048, 1), 'no 896, nh 2048',
        'identity state 65536 bytes', 'identity state in LDS', 'K 3', 'both ends of both identity ranges in use')
    add('identity_scratch_first', _spread_identities(_walk_k3(31, 9, 40), 897, 2048, 1), 'no 897, nh 2048',
        'identity state 65560 bytes', 'identity state in scratch', 'K 3', 'both ends of both identity ranges in use')
    add('identity_1x1', make_scene([[(0, 5, 5)]] * 4, [[(6, 5)], [(90, 90)], [(5, 6)], [(5, 5), (7, 7)]], [[[0], [0], [0], [-1, 0]]]),
        'no 1, nh 1', 'identity state in LDS')
    add('odd_product_k3', _walk_k3(33, 6, 7, no=7, nh=21), 'no 7, nh 21', 'no * nh odd', 'K 3')
    add('claimants_70', _claimants_case(70), '71 frames', '70 claimants of one partner',
        'the lowest claiming slot does not hold the lowest identity', 'the claimants span two lane strides')
    add('ignored_inputs', _ignored_case(), 'label identities -1, no and no + 5', 'tracks -2, nh and nh + 7', 'count = cap + 3',
        'count = -4', 'gcount = gcap + 2', 'the entries beyond the counts are decoys', 'the out-of-range identities are decoys')
    add('many_associations', _many_associations(300), 'K 300', '9 frames', 'every association differs from its neighbours in a count')
    return c


@functools.lru_cache(maxsize=None)
def limit_reference(name, k=0):
    return reference(limit_cases()[name].scene, k)


def facts_of(case):
    """The route facts that hold for the case's scene, recomputed from its arrays, the reference and the constants above
    (a superset of what the case claims, if the case is right)."""
    s = case.scene
    K, F, cap = s['tracks'].shape
    gcap, no, nh, md = s['gid'].shape[1], s['no'], s['nh'], s['max_dist']
    assert 1 <= cap <= MOT_MAX_SIDE and 1 <= gcap <= MOT_MAX_SIDE and 0 <= md <= MOT_MAX_DIST
    assert 1 <= no <= MOT_MAX_IDENTITIES and 1 <= nh <= MOT_MAX_IDENTITIES
    refs = [limit_reference(case.name, k) for k in range(K)]
    lds, state = clear_lds_bytes(gcap, cap), lsap_bytes(no, nh)
    assert state == identity_state_bytes(no, nh)
    out = {f'cap {cap}, gcap {gcap}, max_dist {md}', f'max_dist {md}', f'no {no}, nh {nh}', f'K {K}', f'{F} frames',
           f'clear LDS {lds} bytes', 'clear LDS above 64 KiB' if lds > DEFAULT_DYNAMIC_LDS else 'clear LDS within 64 KiB',
           f'identity state {state} bytes', 'identity state in LDS' if state <= IDENTITY_LDS_LIMIT else 'identity state in scratch'}
    facts = {}
    step2 = [e for r in refs for e in r['step2'].values()]
    if step2:
        out.add(f'largest min(nr, nc) + 1 = {max(min(e["nr"], e["nc"]) for e in step2) + 1}')
        facts['the f64 guard fails: solved in integers'] = any(e['solver'] == 'int' for e in step2)
        facts['largest dual >= 2^50'] = max(e['max_dual'] for e in step2) >= 1 << 50
        facts['largest dual < 2^43'] = all(e['solver'] == 'int' for e in step2) and max(e['max_dual'] for e in step2) < 1 << 43
        facts['no row ends on its dummy'] = max(e['n_dummy'] for e in step2) == 0
        facts['hash sum of the chosen pairs < 2^26'] = max(e['hash_sum'] for e in step2) < 1 << 26
        facts['the chosen costs carry more than 2^24 of hash'] = max(e['hash_sum'] for e in step2) > 1 << 24
        facts['1024 pairs chosen in one frame'] = max(len(e['pairs']) for e in step2) == 1024
        per_frame = [refs[0]['step2'].get(f, dict(n_dummy=0, nc=0, pairs=[])) for f in range(F)]
        facts['at least 512 rows end on their dummy in every frame'] = min(e['n_dummy'] for e in per_frame) >= 512
        facts['at least 512 columns stay free in every frame'] = min(e['nc'] - len(e['pairs']) for e in per_frame) >= 512
    facts['every frame is full: count = cap, gcount = gcap'] = bool((s['count'] == cap).all() and (s['gcount'] == gcap).all())
    facts['an admissible d2 >= 60000'] = max(r['max_ok_d2'] for r in refs) >= 60000
    matched = set().union(*(r['matched_d2'] for r in refs))
    if len(matched) <= 4:
        out |= {f'matched d2 {v}' for v in matched}
    facts['every matched d2 is 0'] = matched == {0}
    if refs[0]['refused_d2'] is not None:
        out.add(f'smallest refused d2 {refs[0]["refused_d2"]}')
    # all pairs of live slots, frame by frame
    n_ok = n_all = 0
    ok_d2 = set()
    for f in range(F):
        ng, nd = max(min(int(s['gcount'][f]), gcap), 0), max(min(int(s['count'][f]), cap), 0)
        d2 = ((s['gx'][f, :ng, None].astype(np.int64) - s['x'][f, None, :nd]) ** 2
              + (s['gy'][f, :ng, None].astype(np.int64) - s['y'][f, None, :nd]) ** 2)
        n_ok += int((d2 <= md * md).sum()); n_all += d2.size
        ok_d2 |= set(np.unique(d2[d2 <= md * md]).tolist())
    facts['sparse: most pairs are not admissible'] = n_all > 0 and n_ok * 10 < n_all
    facts['every admissible pair at one d2'] = len(ok_d2) == 1
    facts['no * nh odd'] = (no * nh) % 2 == 1
    gid_live = {int(v) for f in range(F) for v in s['gid'][f, :max(min(int(s['gcount'][f]), gcap), 0)]}
    tr_live = {int(v) for f in range(F) for v in s['tracks'][:, f, :max(min(int(s['count'][f]), cap), 0)].reshape(-1)}
    facts['both ends of both identity ranges in use'] = {0, no - 1} <= gid_live and {0, nh - 1} <= tr_live
    facts['label identities -1, no and no + 5'] = {-1, no, no + 5} <= gid_live
    facts['tracks -2, nh and nh + 7'] = {-2, nh, nh + 7} <= tr_live
    facts['count = cap + 3'] = cap + 3 in s['count']
    facts['count = -4'] = -4 in s['count']
    facts['gcount = gcap + 2'] = gcap + 2 in s['gcount']
    if case.name == 'ignored_inputs':                      # a second and third reference: only this small case pays for them
        full = dict(s, count=np.full(F, cap, np.int32), gcount=np.full(F, gcap, np.int32))
        facts['the entries beyond the counts are decoys'] = reference(full)['counts'].tolist() != refs[0]['counts'].tolist()
        near = []                                          # every ignored identity stands within reach of a live opposite
        for f in range(F):
            ng, nd = max(min(int(s['gcount'][f]), gcap), 0), max(min(int(s['count'][f]), cap), 0)
            d2 = ((s['gx'][f, :ng, None].astype(np.int64) - s['x'][f, None, :nd]) ** 2
                  + (s['gy'][f, :ng, None].astype(np.int64) - s['y'][f, None, :nd]) ** 2)
            g, h = s['gid'][f, :ng], s['tracks'][0, f, :nd]
            g_ok, h_ok = (g >= 0) & (g < no), (h >= 0) & (h < nh)
            near += [bool((d2[i, h_ok] <= md * md).any()) for i in np.nonzero(~g_ok)[0]]
            near += [bool((d2[g_ok, j] <= md * md).any()) for j in np.nonzero(~h_ok & (h != -1))[0]]
        facts['the out-of-range identities are decoys'] = len(near) >= 6 and all(near)
    claims = [(cl, f) for r in refs for f, per in r['claims'].items() for cl in per]
    if claims:
        big, f = max(claims, key=lambda q: len(q[0]))
        out.add(f'{len(big)} claimants of one partner')
        facts['the lowest claiming slot does not hold the lowest identity'] = \
            int(s['gid'][f, min(big)]) != min(int(s['gid'][f, i]) for i in big)
        facts['the claimants span two lane strides'] = min(big) // WAVE != max(big) // WAVE
    if K > 1:
        cs = [r['counts'].tolist() for r in refs]
        facts['every association differs from its neighbours in a count'] = all(a != b for a, b in zip(cs, cs[1:]))
    return out | {name for name, holds in facts.items() if holds}
