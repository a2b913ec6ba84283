"""Cases for the search step of the Hungarian pair kernels and for the chain numbering (axtrack_amd/csrc/hungarian.hip),
with a numpy model of the kernel's own rules. No GPU and no product code.

The pair kernels are judged by hungarian_reference.judge against SciPy. SciPy cannot say which of two optimal matchings
is the kernel's, so the cases that tie on purpose hand the judge the trajectories of `jv_model` below: the same
shortest-augmenting-path algorithm with the rules of the header of hungarian.hip written out -- the first column among
equal costs in the initialisation, the smallest column among equal keys in a search step, the dummy before a column of
the same key. tests/test_hungarian_step_cpu.py pins the model to SciPy wherever the optimum is unique.

All costs are given as a table (d_ctab of axt_hungarian_pairs), so that the keys of a search step are chosen freely:
in the `contest` scenes rows 0 and 1 both want column J0 at cost BASE and nothing else costs less, row 0 takes it, row 1
searches. In the second step of that search the key of column j is min(c[1, j], c[0, j]) - BASE, whatever else happens."""
import functools
import itertools

import numpy as np

import hungarian_reference as hr

HINF = hr.NO_LINK
KEY_LIMIT = 1 << 51                     # wave_argmin: keys from here on are no candidates
BASE = 1 << 16
J0 = 2


# ------------------------------------------------------------------------------------------------ the argmin, twice
def pack(keys, cols):
    """(key << 11) | column as the kernel forms it, ~0 for a key that is no candidate. u64 arrays."""
    keys, cols = np.asarray(keys, np.int64), np.asarray(cols, np.int64)
    v = (keys.astype(np.uint64) << np.uint64(11)) | cols.astype(np.uint64)
    return np.where(keys >= KEY_LIMIT, np.uint64(0xFFFFFFFFFFFFFFFF), v)


def unpack(best):
    best = int(best)
    return (HINF, 0x7fffffff) if best == 0xFFFFFFFFFFFFFFFF else (best >> 11, best & 2047)


def lane_words(keys):
    """What the 64 lanes hand to wave_argmin for the open columns' keys (HINF: closed or no link): every lane's best over
    its columns lane, lane + 64, ..., the first of equal keys, packed."""
    keys = np.asarray(keys, np.int64)
    m = len(keys)
    pad = np.full((-m) % 64, HINF, np.int64)
    k = np.concatenate([keys, pad]).reshape(-1, 64)              # [slot, lane]
    slot = k.argmin(axis=0)                                      # first smallest
    lane = np.arange(64)
    best = k[slot, lane]
    idx = np.where(best < HINF, slot * 64 + lane, 0x7ff)         # (the kernel's 0x7fffffff never reaches a packed word)
    return pack(best, idx)


def argmin_64(words):
    return unpack(np.asarray(words, np.uint64).min())


def argmin_two_phase(words):
    """The minimum of the high words, then the minimum of the low words among the lanes that hold it (the others offer
    0xffffffff)."""
    words = np.asarray(words, np.uint64)
    hi, lo = (words >> np.uint64(32)).astype(np.uint32), (words & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    mh = hi.min()
    ml = np.where(hi == mh, lo, np.uint32(0xFFFFFFFF)).min()
    return unpack((int(mh) << 32) | int(ml))


# ------------------------------------------------------------------------------------------------ the kernel's rules
def jv_model(cost, dummy, steps=None):
    """One pair as hungarian_pair_kernel solves it. cost i64 [n, m] (HINF: no link), dummy i64 [n]. Returns (match i64 [n]:
    column or -1, integer total). steps: optional list that receives, per search step, the keys of the open columns."""
    cost, dummy = np.asarray(cost, np.int64), np.asarray(dummy, np.int64)
    n, m = cost.shape
    u, v = np.zeros(n, np.int64), np.zeros(m, np.int64)
    col4row, row4col = np.full(n, -1, np.int64), np.full(m, -1, np.int64)
    for i in range(n):
        j = int(cost[i].argmin()) if m else -1
        if m and cost[i, j] < dummy[i]:
            u[i] = cost[i, j]
            if row4col[j] < 0:
                row4col[j], col4row[i] = i, j
        else:
            u[i], col4row[i] = dummy[i], -2
    for i in range(n):
        if col4row[i] != -1:
            continue
        spc, sc, pred = np.full(m, HINF, np.int64), np.zeros(m, bool), np.full(m, -1, np.int64)
        min_val, best_dummy, dummy_row, cur, sr = 0, HINF, -1, i, []
        while True:
            sr.append(cur)
            rd = min_val + int(dummy[cur]) - int(u[cur])
            if rd < best_dummy:
                best_dummy, dummy_row = rd, cur
            r = min_val + cost[cur] - u[cur] - v
            upd = ~sc & (cost[cur] != HINF) & (r < spc)
            spc[upd], pred[upd] = r[upd], cur
            keys = np.where(sc, HINF, spc)
            if steps is not None:
                steps.append(keys.copy())
            bkey, j = argmin_64(lane_words(keys))
            if best_dummy <= bkey:
                sink, min_val = -2, best_dummy
                break
            min_val = bkey
            sc[j] = True
            if row4col[j] < 0:
                sink = j
                break
            cur = int(row4col[j])
        for k, row in enumerate(sr):
            u[row] += min_val if k == 0 else min_val - spc[col4row[row]]
        dual = sc.copy()
        if sink >= 0:
            dual[sink] = False
        v[dual] -= min_val - spc[dual]
        row, jnew = (dummy_row, -2) if sink == -2 else (int(pred[sink]), sink)
        while True:
            jprev = int(col4row[row])
            col4row[row] = jnew
            if jnew >= 0:
                row4col[jnew] = row
            if row == i:
                break
            jnew = jprev
            row = int(pred[jnew])
    match = np.where(col4row >= 0, col4row, -1)
    li = match >= 0
    return match, int(sum(int(c) for c in cost[np.nonzero(li)[0], match[li]])) + int(sum(int(d) for d in dummy[~li]))


def model_reference(costs, counts, thr_units=hr.THR_UNITS, max_gap=2):
    """hungarian_reference.reference_from_costs with jv_model in SciPy's place."""
    solver, hr.pair_reference = hr.pair_reference, jv_model
    try:
        return hr.reference_from_costs(costs, counts, thr_units, max_gap)
    finally:
        hr.pair_reference = solver


def enumerated_optimum(cost, dummy):
    """Exact optimum of a pair with few admitted links, in Python integers: (total, list of the matchings that reach it)."""
    n = cost.shape[0]
    options = [[-1] + [int(j) for j in np.nonzero(cost[i] != HINF)[0]] for i in range(n)]
    best, where = None, []
    for pick in itertools.product(*options):
        cols = [j for j in pick if j >= 0]
        if len(cols) != len(set(cols)):
            continue
        total = sum(int(cost[i, j]) if j >= 0 else int(dummy[i]) for i, j in enumerate(pick))
        if best is None or total < best:
            best, where = total, [pick]
        elif total == best:
            where.append(pick)
    return best, where


# ------------------------------------------------------------------------------------------------ cases
def full_costs(counts, max_gap, given):
    out = {(t, g): np.full((counts[t], counts[t + g]), HINF, np.int64)
           for g in range(1, max_gap + 1) for t in range(len(counts) - g)}
    out.update(given)
    return out


def contest(name, m, keys, cap=144, thr_units=hr.THR_UNITS, wins=None, ties=False, exact='scipy'):
    """Two rows that both want column J0 of m. keys: {column: (key offered by row 1, key offered by row 0)} in the second
    step of row 1's search, None for no link; a key may be the string 'dummy' = the key of leaving a row unlinked.
    wins: the column that must join the tree in that step, or 'dummy'."""
    counts = [2, m]

    def costs():
        d = hr.dummy_costs(counts, thr_units)[0]
        c = np.full((2, m), HINF, np.int64)
        c[:, J0] = BASE
        for j, ks in keys.items():
            for row, k in zip((1, 0), ks):
                if k is not None:
                    c[row, j] = BASE + (int(d.min()) - BASE if k == 'dummy' else k)
        return full_costs(counts, 1, {(0, 1): c})

    return hr.Case(name, cap, 'ctab', costs, counts, max_gap=1, thr_units=thr_units, wins=wins, ties=ties, exact=exact,
                   family='argmin')


H7 = 7 << 21                            # keys that share their high word (bits 21.. of the key are the packed word's high word)


@functools.lru_cache(None)
def argmin_cases():
    return [
        contest('hi_equal_lo_differs', 140, {3: (H7 | 500, None), 70: (H7 | 499, None), 135: (None, H7 | 501)}, wins=70),
        contest('lo_equal_hi_differs', 140, {3: ((9 << 21) | 77, None), 70: (None, (8 << 21) | 77), 135: ((10 << 21) | 77, None)}, wins=70),
        contest('hi_decides_against_lo', 140, {3: ((9 << 21) | 5, None), 70: ((8 << 21) | 900, None), 135: (None, (10 << 21) | 1)}, wins=70),
        contest('tie_two_lanes', 64, {20: (H7 | 9, None), 17: (H7 | 9, None)}, wins=17, ties=True),
        contest('tie_two_rows_of_lanes', 64, {40: (H7 | 9, None), 5: (None, H7 | 9)}, wins=5, ties=True),
        contest('tie_two_slots_one_lane', 140, {74: (H7 | 9, None), 10: (H7 | 9, None)}, wins=10, ties=True),
        contest('tie_three_slots', 140, {139: (H7 | 9, None), 75: (None, H7 | 9), 12: (H7 | 9, None)}, wins=12, ties=True),
        contest('key_2p51_minus_1', 70, {66: (KEY_LIMIT - 1, None)}, thr_units=1 << 36, wins=66, exact='enumeration'),
        contest('key_2p51_minus_1_against_smaller', 140, {66: (KEY_LIMIT - 1, None), 131: (None, KEY_LIMIT - 2)}, thr_units=1 << 36,
                wins=131, exact='enumeration'),
        contest('no_admissible_column', 140, {}, wins='dummy'),
        contest('tie_column_and_dummy', 140, {90: ('dummy', None)}, wins='dummy', ties=True),
    ]


def _battery(name, cap, counts, pattern, seed, max_gap=2):
    return hr.Case(f'{name}_{pattern}', cap, 'ctab', functools.partial(hr._ctab_costs, pattern, counts, seed), counts, max_gap=max_gap,
                   pattern=pattern, ties=False, exact='scipy', family='boundary')


BOUNDARY_SIZES_144 = (1, 63, 64, 65, 127, 128, 129)


@functools.lru_cache(None)
def boundary_cases():
    """Frame counts on both sides of the 64-column slots, in both roles (rows, columns), below and beyond the 96 x 96 cost
    cache; the counts dip, so the gap-2 pairs find some of their rows and columns taken; empty frames on either side."""
    cases = []
    for pattern in ('dense', 'machol_wien'):
        cases += [
            _battery('b144_rising', 144, [1, 63, 64, 65, 127, 128, 129, 1], pattern, 31),
            _battery('b144_mixed', 144, [129, 64, 127, 65, 128, 63, 129, 127], pattern, 32),
            _battery('b144_cached', 144, [96, 63, 65, 64, 96, 65, 63, 1], pattern, 33),
            _battery('b192', 192, [191, 192, 150, 192, 191, 129], pattern, 34),
            _battery('b144_empty_frames', 144, [70, 0, 65, 66, 0, 0, 129, 64], pattern, 35),
        ]
    return cases


def pair_cases():
    return argmin_cases() + boundary_cases()


# ------------------------------------------------------------------------------------------------ chain numbering
CHAIN_SMALL_SLOTS = 8192                                    # axt_chain_tracks: `slots <= 8192`


def chain_route(slots, small=CHAIN_SMALL_SLOTS):
    return 'small' if slots <= small else 'launches'


def shape_of(slots):
    """(frames, cap) with frames * cap == slots and as many frames (up to 64) as divide it."""
    f = max(k for k in range(1, 65) if slots % k == 0)
    return f, slots // f


def chain_shapes(small=CHAIN_SMALL_SLOTS):
    """Both sides of the bound between the one workgroup and the launches, and frame counts on both sides of the powers of
    four (the rounds of pointer jumping) at slot counts that take the launches and are no multiple of 64 where the frame
    count allows it."""
    shapes = [shape_of(small), shape_of(small + 1)]
    for f in (1, 2, 3, 4, 5, 16, 17, 64, 65):
        cap = -(-(small + 200) // f)
        shapes.append((f, cap + (cap * f % 64 == 0)))
    return shapes


CHAIN_KINDS = ('spanning', 'single', 'holes', 'gap2_only', 'empty_middle')


def chain_scene(F, cap, kind, seed=0):
    """(count, pred1, pred2): hungarian_reference.chain_scene's kinds, and
    'gap2_only'     chains made of gap-2 links alone: one family through the even frames, one through the odd ones;
    'empty_middle'  spanning chains that step over one empty frame in the middle."""
    if kind in ('spanning', 'single', 'roots', 'holes'):
        return hr.chain_scene(F, cap, kind, seed)
    rng = np.random.default_rng(seed)
    count = np.full(F, cap, np.int32)
    pred1 = np.full((F, cap), -1, np.int32)
    pred2 = np.full((F, cap), -1, np.int32)
    if kind == 'gap2_only':
        count[1::2] = max(cap - 5, 1)
        for t in range(2, F):
            k = int(min(count[t], count[t - 2]))
            pred2[t, rng.permutation(int(count[t]))[:k]] = rng.permutation(int(count[t - 2]))[:k]
        return count, pred1, pred2
    assert kind == 'empty_middle'
    mid = F // 2
    if F >= 3:
        count[mid] = 0
    for t in range(1, F):
        if count[t] == 0:
            continue
        src, into = (t - 1, pred1) if count[t - 1] > 0 else (t - 2, pred2)
        if src < 0:
            continue
        k = int(min(count[t], count[src])) - 1
        if k > 0:
            into[t, rng.permutation(int(count[t]))[:k]] = rng.permutation(int(count[src]))[:k]
    return count, pred1, pred2
