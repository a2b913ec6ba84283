"""CPU reference of the device tracking scorer (csrc/mot.hip) and the scenes its tests share. No product
code except axtrack_amd.mot_metrics (pair_cost_int, and accumulate for the tie-free check).

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


def _solve(cost, ok, sum_first=False):
    """As many admissible pairs as possible first, then the smallest integer sum; exact in f64 (asserted)."""
    if not ok.any():
        return []
    cmax = int(cost[ok].max())
    big = (cmax + 1) if sum_first else (min(cost.shape) + 1) * (cmax + 1)
    assert min(cost.shape) * big < 2 ** 53, 'totals would not be exact in f64'
    r, c = linear_sum_assignment(np.where(ok, cost, big).astype(np.float64))
    return [(int(i), int(j)) for i, j in zip(r, c) if ok[i, j]]


def reference(s, k=0, broken=None):
    """The definition on the CPU for association k. -> dict(counts i64 [10], tallies i64 [no,2], events set of
    (frame, kind, label slot, partner slot), fp set of (frame, slot), id_events set of (frame, kind, label identity,
    track identity), co i64 [no,nh], claimants: frames in which two labels claimed one remembered partner)."""
    assert broken is None or broken in RULES
    no, nh, md2 = s['no'], s['nh'], s['max_dist'] ** 2
    partner = np.full(no, -1, np.int64)
    state = np.zeros(no, np.int64)                 # 0 never tracked, 1 tracked last, 2 in a miss run after it
    tallies = np.zeros((no, 2), np.int64)
    co = np.zeros((no, nh), np.int64)
    c = dict.fromkeys(mm.MOT_COUNTS, 0)
    events, fps, id_events, claim_frames = set(), set(), set(), []
    for f in range(len(s['count'])):
        ng, nd = int(s['gcount'][f]), int(s['count'][f])
        lab = [(i, int(s['gid'][f, i])) for i in range(ng) if 0 <= s['gid'][f, i] < no]
        hyp = [(j, int(s['tracks'][k, f, j])) for j in range(nd) if 0 <= s['tracks'][k, f, j] < nh]
        li = np.array([i for i, _ in lab], np.int64); g = np.array([v for _, v in lab], np.int64)
        hj = np.array([j for j, _ in hyp], np.int64); h = np.array([v for _, v in hyp], np.int64)
        dx = s['gx'][f, li].astype(np.int64)[:, None] - s['x'][f, hj].astype(np.int64)[None, :]
        dy = s['gy'][f, li].astype(np.int64)[:, None] - s['y'][f, hj].astype(np.int64)[None, :]
        d2 = dx * dx + dy * dy
        ok = d2 < md2 if broken == 'exclusive_threshold' else d2 <= md2
        for a, b in zip(*np.nonzero(ok)):
            co[g[a], h[b]] += 1
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
        for b, claimants in want.items():
            a = max(claimants) if broken == 'higher_slot_wins' else min(claimants)
            kind[a], part[a], h_done[b] = 1, b, True
        # 2. the rest, exactly
        rows, cols = np.nonzero(kind == 0)[0], np.nonzero(~h_done)[0]
        if len(rows) and len(cols):
            cost = mm.pair_cost_int(d2[np.ix_(rows, cols)], g[rows][:, None], h[cols][None, :])
            for r, q in _solve(cost, ok[np.ix_(rows, cols)], broken == 'sum_before_cardinality'):
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
                id_events=id_events, co=co, claimants=claim_frames)


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


def _lane_case(n_lab, n_hyp, seed):
    """n_lab labels and n_hyp detections on a 15 px grid (every label reaches several detections), three frames, slot
    order shuffled: lane strides of the claim, the compaction and the searches."""
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
        tr.append([int(o) + (1000 if f == 2 and o % 7 == 0 else 0) for o in ho])
    return make_scene(labels, dets, [tr])


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
