"""The cases of tests/stagekernel_cases.py, checked on the CPU: every case reaches the route its facts name (computed from its
inputs and the restated launch constants), its decode lands on the intended pixels, the vectorised open-grid CSR builder
equals a per-pair loop over the oracle, and the inputs stay clear of the values where an exact comparison with the GPU would
hinge on the last bit of a logarithm. The last block breaks one route at a time in a CPU model of the kernels and shows that
a named case then differs from its reference -- the cases are sharp enough to see those bugs."""
import numpy as np
import pytest

import stagekernel_cases as sc
from helpers import golden_dets, csr_arcs_from_oracle
from oracle import oracle as orc

CASES = sc.all_cases()
BY_NAME = {(c.family, c.name): c for c in CASES}


def family(name):
    return [c for c in CASES if c.family == name]


def test_case_names_are_unique():
    assert len(BY_NAME) == len(CASES)


@pytest.mark.parametrize('case', CASES, ids=lambda c: f'{c.family}-{c.name}')
def test_route_facts_hold(case):
    have = sc.facts_of(case)
    assert case.facts and not set(case.facts) - have, f'{case.route}: claimed but not true: {sorted(set(case.facts) - have)}'


# ------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize('case', family('decode'), ids=repr)
def test_decode_lands_on_the_intended_pixels(case):
    """With every confidence forced above the threshold (NaN and the dropped ones included), the oracle's decode puts each
    crafted cell on the pixel its case intends."""
    y = case.yolo.copy()
    y[..., 0] = 1.0
    for (f, k, cell), want in case.want.items():
        if want is None:
            continue
        c, x, yy, cells = orc.decode_filter(y[f], sc.TILE, sc.S, np.float32(0.5))[k]
        at = int(np.nonzero(cells == cell)[0][0])
        iy, ix = case.keep[k]
        assert (int(x[at]) + ix * sc.TILE, int(yy[at]) + iy * sc.TILE) == tuple(want), (case.name, f, k, cell)


@pytest.mark.parametrize('n_tiles', [sc.LDS_TILES, sc.LDS_TILES + 1])
def test_decode_chain_survivors(n_tiles):
    """The 432-link chain leaves every other link (216), tile 4 its 144 isolated cells; the half-to-even, tie and distance cases
    of frame 1 resolve as intended."""
    case = BY_NAME[('decode', f'tiles{n_tiles}')]
    ref = sc.decode_reference(case)
    c2, x2, y2 = ref[2]
    chain = y2 == 2000
    assert chain.sum() == 216 and sorted(x2[chain].tolist()) == [20 + 30 * e for e in range(216)]
    assert len(c2) == 216 + 144 + 1 > sc.NMS_THREADS
    assert case.cap == n_tiles * sc.CELLS + 5 and max(case.keep) == (15, 3)
    surv = set(zip(ref[1][1].tolist(), ref[1][2].tolist()))
    assert {(0, 2), (130, 0), (128, 130), (2, 128)} <= surv                       # half to even
    assert (300, 300) in surv and (310, 300) not in surv and (300, 312) not in surv      # tie: the first in (tile, cell) order
    assert (400, 300) in surv and (410, 300) not in surv
    for n, (dx, dy) in enumerate(sc.NMS_PAIRS):
        assert ((100 + 100 * n + dx, 200 + dy) in surv) == (dx * dx + dy * dy >= 529)
    assert (-32, -21) in surv and (224, -43) in surv
    assert (40, 40) in surv and (80, 40) not in surv and (120, 40) not in surv and (160, 40) in surv


def test_decode_zero_cells_survive_once_per_tile():
    case = BY_NAME[('decode', 'zero_cells_thr0')]
    ref = sc.decode_reference(case)
    assert [len(r[0]) for r in ref] == [2, 4, 3]
    assert set(zip(ref[0][1].tolist(), ref[0][2].tolist())) == {(512, 0), (1536, 1024)}


# ------------------------------------------------------------------------------------------------- arcs
def csr_pair_loop(case, miss_rate=0.6):
    """The arcs, pair by pair: orc.path_matrix (or the table entry), admission by dmax, orc.transition_cost -> orc.arc_cost_int
    when the case's units are the transition table, units / 1e6 -> orc.arc_cost_int otherwise."""
    H, W = case.shape
    F, cap = case.x.shape
    cnt = [int(min(n, cap)) for n in case.count]
    src = cnt if case.src_count is None else [int(n) for n in case.src_count]
    offs = np.concatenate([[0], np.cumsum(cnt)])
    dets = [(None, case.x[t, :cnt[t]].astype(np.int64), case.y[t, :cnt[t]].astype(np.int64)) for t in range(F)]
    real = np.array_equal(case.units, sc.transition_units(len(case.dmax), case.max_dist, miss_rate))
    rows = [[] for _ in range(int(offs[-1]))]
    for t in range(F):
        for g in range(1, len(case.dmax) + 1):
            tb = t + g
            if tb >= F or not cnt[t] or not cnt[tb]:
                continue
            D = orc.path_matrix(dets[t], dets[tb], H, W, None, case.max_dist, case.conn8)
            for i in range(src[t]):
                for j in range(cnt[tb]):
                    d = int(D[i, j])
                    if case.length_table is not None:
                        d = int(case.length_table[t, i, g - 1, j])
                        if d <= 0:
                            continue
                    if d > case.dmax[g - 1]:
                        continue
                    a, b = int(offs[t] + i), int(offs[tb] + j)
                    c = float(orc.transition_cost(np.array([d]), g, miss_rate, max_px=case.max_dist)[0]) if real else case.units[g - 1, d] / 1e6
                    rows[a].append((g, b, d, orc.arc_cost_int(c, 3, a, b)))
    row_ptr, flat = [0], []
    for r in rows:
        flat += sorted(r)
        row_ptr.append(len(flat))
    return np.array(row_ptr), flat


def _shrunk(case, F, n):
    """The first F frames of a case with at most n detections each."""
    kw = dict(x=case.x[:F], y=case.y[:F], count=np.minimum(case.count[:F], n).astype(np.int32), shape=case.shape, dmax=case.dmax,
              max_dist=case.max_dist, units=case.units, conn8=case.conn8, vis=None,
              src_count=None if case.src_count is None else np.minimum(case.src_count[:F], n).astype(np.int32),
              length_table=None if case.length_table is None else case.length_table[:F])
    return sc.Case('arcs', case.name + '_small', [], **kw)


SMALL = [BY_NAME[('arcs', 'deep_gaps')], _shrunk(BY_NAME[('arcs', 'many_detections_conn8')], 4, 25),
         _shrunk(BY_NAME[('arcs', 'many_frames')], 40, 4), _shrunk(BY_NAME[('arcs', 'rows_partial_frame')], 4, 30),
         _shrunk(BY_NAME[('arcs', 'length_table')], 5, 30)]


@pytest.mark.parametrize('case', SMALL, ids=repr)
def test_vectorised_csr_equals_the_pair_loop(case):
    ref = sc.arcs_reference(case)
    row_ptr, flat = csr_pair_loop(case)
    assert len(flat) > 20
    assert np.array_equal(ref.row_ptr, row_ptr)
    got = list(zip(ref.gap.tolist(), ref.col.tolist(), ref.length.tolist(), ref.cost.tolist()))
    assert got == flat


def test_vectorised_csr_equals_the_helper_on_the_golden_detections(golden):
    dets = golden_dets(golden('detect_1024'))
    F, cap = len(dets), max(len(d[0]) for d in dets)
    x, y = np.zeros((F, cap), np.int32), np.zeros((F, cap), np.int32)
    for t, d in enumerate(dets):
        x[t, :len(d[1])], y[t, :len(d[2])] = d[1], d[2]
    cnt = np.array([len(d[0]) for d in dets], np.int32)
    P = orc.DEFAULTS
    gaps = P['MCF_MAX_NUM_MISSES'] + 1
    D = np.arange(orc.MAX_PX_ASSOC_DIST + 1)
    dmax = [int(np.nonzero(orc.transition_cost(D, g, P['MCF_MISS_RATE']) < P['MCF_EDGE_COST_THR'])[0].max()) for g in range(1, gaps + 1)]
    got = sc.open_grid_csr(x, y, cnt, 1024, 1024, dmax, units=sc.transition_units(gaps, orc.MAX_PX_ASSOC_DIST, P['MCF_MISS_RATE']))
    r_row, r_col, r_len, r_gap, r_cost, offs = csr_arcs_from_oracle(dets, 1024, 1024)
    assert len(r_col) > 1000
    for a, b in ((got.row_ptr, r_row), (got.col, r_col), (got.length, r_len), (got.gap, r_gap), (got.cost, r_cost), (got.offs, offs)):
        assert np.array_equal(a, b)


def test_vectorised_arc_cost_equals_the_oracles():
    rng = np.random.default_rng(0)
    units, a, b = rng.integers(-5_000_000, 20_000_000, 200), rng.integers(0, 400_000, 200), rng.integers(0, 400_000, 200)
    got = sc.arc_cost_int_vec(units, 3, a, b)
    assert got.tolist() == [orc.arc_cost_int(u / 1e6, 3, i, j) for u, i, j in zip(units.tolist(), a.tolist(), b.tolist())]


def test_row_subsets_add_up_to_the_whole():
    """Rows built for frames 0-2 and for frames 3-7 together are the rows of the whole timelapse; foreign rows are empty."""
    whole = sc.arcs_reference(BY_NAME[('arcs', 'many_detections')])
    lo, hi = (sc.arcs_reference(BY_NAME[('arcs', n)]) for n in ('rows_frames_0_2', 'rows_frames_3_7'))
    split = int(whole.offs[3])
    assert len(lo.col) + len(hi.col) == len(whole.col) and len(lo.col) and len(hi.col)
    assert (lo.tail < split).all() and (hi.tail >= split).all()
    for k in ('tail', 'col', 'length', 'gap', 'cost'):
        assert np.array_equal(np.concatenate([getattr(lo, k), getattr(hi, k)]), getattr(whole, k)), k
    part_case = BY_NAME[('arcs', 'rows_partial_frame')]
    part = sc.arcs_reference(part_case)
    n = np.diff(part.row_ptr)
    o = part.offs
    assert (n[o[2]:o[2] + 70] > 0).any() and not n[o[2] + 70:o[3]].any() and not n[o[0]:o[1]].any() and np.diff(whole.row_ptr)[o[2] + 70:o[3]].any()


# ------------------------------------------------------------------------------------------------- conditions of exactness
def test_observation_costs_stay_clear_of_half_units():
    """f64 log on the GPU is within 1 ulp: rint(cost * 1e6) is the same as long as no cost lies within 1e-4 units of a half."""
    case = BY_NAME[('obs', 'counts_0_1_130_200')]
    valid = np.arange(case.conf.shape[1])[None] < case.count[:, None]
    for method in ('scale_to_max', 'ceil'):
        u = sc.obs_reference(case, method)[valid] * 1e6
        assert np.abs(np.abs(u - np.floor(u)) - 0.5).min() > 1e-4, method
    stm = sc.obs_reference(case, 'scale_to_max')
    assert stm[1, 0] == 4.6 and stm[3, 150] == -4.6 and 4.0 < stm[2, 5] < 4.6       # conf 0.55, 60 and 1.0 against a maximum of 60


@pytest.mark.parametrize('case', [c for c in family('arcs') if c.vis is not None], ids=repr)
def test_appearance_costs_stay_clear_of_the_admission_threshold(case):
    ref, cost, margin = sc.vis_csr(case)
    assert margin > 1e-9, f'{case.name}: a candidate pair costs within {margin} of the threshold'
    assert len(ref.col) > 500
    u = cost * 1e6
    assert np.abs(np.abs(u - np.floor(u)) - 0.5).min() > 1e-6


@pytest.mark.parametrize('case', family('prep'), ids=repr)
def test_preprocess_inputs_stay_clear_of_the_clip(case):
    """Both sides compute the value the clip sees with the same correctly rounded f32 operations, so a value EQUAL to the clip
    (the case has one, on purpose) is safe; a value one ulp beside it would only be as long as that stays true."""
    v = sc.prep_prelog(case)
    clip = np.float32(case.clip)
    near = (v != clip) & (v >= np.nextafter(clip, np.float32(0))) & (v <= np.nextafter(clip, np.float32(1)))
    assert not near.any()
    raw = case.raw.reshape(-1)
    if raw.size > 100:
        assert (v == clip).any() and (sc.prep_reference(case).reshape(-1)[raw == sc.PREP_RAW_OFFSET] == 0).all()
        kept = sc.prep_reference(case)[(v == clip)]
        assert (kept > 0).all()                                                   # equal to the clip is kept


# ------------------------------------------------------------------------------------------------- a broken route shows
def _nocarry_offsets(counts, chunk):
    """The exclusive scan of a kernel that forgets its carry between chunks."""
    ex = np.zeros(len(counts), np.int64)
    for b in range(0, len(counts), chunk):
        c = np.asarray(counts[b:b + chunk], np.int64)
        ex[b:b + chunk] = np.cumsum(c) - c
    return ex


def test_a_dropped_chunk_carry_changes_a_named_case():
    """frame_offsets_kernel / row_ptr_kernel / ided_slot_kernel without their carry across chunks of 1024."""
    c = BY_NAME[('arcs', 'many_frames')]
    ref = sc.arcs_reference(c)
    bad = _nocarry_offsets(c.count.astype(np.int64), sc.FRAME_CHUNK)
    assert not np.array_equal(bad, ref.offs[:-1]) and np.array_equal(bad[:sc.FRAME_CHUNK], ref.offs[:sc.FRAME_CHUNK])
    heads_after = ref.col >= ref.offs[sc.FRAME_CHUNK]
    assert heads_after.sum() > 50, 'many_frames: arcs whose head number needs the carry'
    for name in ('many_frames', 'many_detections', 'length_table'):
        r = sc.arcs_reference(BY_NAME[('arcs', name)])
        n = np.diff(r.row_ptr)
        bad = _nocarry_offsets(n, sc.DET_CHUNK)
        assert not np.array_equal(bad, r.row_ptr[:-1]), f'{name}: row_ptr does not need the carry'
    for c in family('ided'):
        has = np.array([len(p) > 0 for p in sc.ided_tables_of(c)], np.int64)
        assert not np.array_equal(_nocarry_offsets(has, sc.FRAME_CHUNK)[has > 0], (np.cumsum(has) - has)[has > 0]), c.name


def test_max_dist_for_missing_table_entries_changes_a_named_case():
    """`if (d <= 0) d = max_dist` instead of lim + 1 admits the pairs without a path where max_dist <= the limit."""
    for c in [BY_NAME[('arcs', 'length_table')]]:
        ref = sc.arcs_reference(c)
        H, W = c.shape
        tab = np.where(c.length_table <= 0, c.max_dist, c.length_table).astype(np.int16)
        bad = sc.open_grid_csr(c.x, c.y, c.count, H, W, c.dmax, c.conn8, c.max_dist, c.units, c.src_count, tab)
        assert len(bad.col) > len(ref.col), c.route


@pytest.mark.parametrize('case', [c for c in family('arcs') if c.name in ('many_detections', 'many_frames', 'length_table', 'vis_table')], ids=repr)
def test_one_target_too_many_changes_a_named_case(case):
    """`j0 + lane <= nb` reads the slot behind a frame's last detection: in these cases that slot holds a plausible target."""
    H, W = case.shape
    cap = case.x.shape[1]
    more = np.minimum(case.count + 1, cap).astype(np.int32)
    more[case.count == 0] = 0
    ref = sc.open_grid_csr(case.x, case.y, case.count, H, W, case.dmax, case.conn8, case.max_dist, None, case.count, case.length_table)
    bad = sc.open_grid_csr(case.x, case.y, more, H, W, case.dmax, case.conn8, case.max_dist, None, case.count, case.length_table)
    assert len(bad.col) > len(ref.col), case.route


@pytest.mark.parametrize('case', [c for c in family('prep') if 'frame_px % 8 != 0' in c.facts], ids=repr)
def test_a_skipped_scalar_tail_changes_a_named_case(case):
    """Without the scalar branch nothing is written where frame_px % 8 != 0, and not the last n_px % 8 pixels otherwise."""
    ref = sc.prep_reference(case).reshape(-1)
    tail = ref[len(ref) - len(ref) % sc.PREP_VEC:] if len(ref) % sc.PREP_VEC else ref
    assert (tail != 0).any(), case.route


@pytest.mark.parametrize('name', ['tiles28', 'tiles29'])
def test_ranking_ties_by_cell_only_changes_a_named_case(name):
    case = BY_NAME[('decode', name)]
    ref = sc.decode_reference(case)[1]
    c, x, y, k, cell = sc.decode_candidates(case, 1)
    order = np.argsort(cell, kind='stable')                        # ties in cell order, whatever the tile
    bad = orc.nms(c[order], x[order], y[order], case.min_dist)
    assert sorted(zip(bad[1].tolist(), bad[2].tolist())) != sorted(zip(ref[1].tolist(), ref[2].tolist())), case.route


def _nms_in_32_bits(conf, x, y, min_dist):
    """orc.nms with dx * dx + dy * dy formed in int32 (wrapping), as a kernel that does not widen forms it."""
    order = np.argsort(-conf.astype(np.float64), kind='stable')
    x, y = x[order].astype(np.int32), y[order].astype(np.int32)
    alive = []
    with np.errstate(over='ignore'):
        for i in range(len(x)):
            dx, dy = x[alive] - x[i], y[alive] - y[i]
            if not ((dx * dx + dy * dy) < np.int32(min_dist * min_dist)).any():
                alive.append(i)
    return len(alive)


@pytest.mark.parametrize('case', sc.distant_tiles_cases(), ids=repr)
def test_distant_twins_separate_a_32_bit_nms_from_an_exact_one(case):
    """The twins' 32-bit squared distance is below 23^2 while the exact one is not: the reference keeps both, a kernel that
    forms the sum in int loses one per frame. The close pair inside tile 0 loses its weaker member either way."""
    ref = sc.decode_reference(case)
    assert len(case.yolo) == 2 and case.min_dist == 23
    for f in range(2):
        c, x, y, k, cell = sc.decode_candidates(case, f)
        assert len(c) == 4
        a, b = np.nonzero(c == np.float32(0.9))[0][0], np.nonzero(c == np.float32(0.8))[0][0]
        assert k[a] == 0 and k[b] == 1 and cell[a] == cell[b]
        dx, dy = int(x[b]) - int(x[a]), int(y[b]) - int(y[a])
        exact = dx * dx + dy * dy
        wrapped = ((exact + 2 ** 31) % 2 ** 32) - 2 ** 31                  # what int arithmetic keeps of it
        assert sorted((abs(dx), abs(dy))) == [0, int(case.name.split('_')[1]) * sc.TILE], case.route
        assert wrapped < 23 * 23 <= exact, f'{case.route}: 32-bit sum {wrapped}, exact {exact}'
        assert len(ref[f][0]) == 3 and {0.9, 0.8, 0.95} == {round(float(v), 2) for v in ref[f][0]}, case.route
        assert _nms_in_32_bits(c, x, y, case.min_dist) == 2, case.route


def test_the_256_tile_case_is_what_it_says():
    case = sc.decode_256_tiles_case()
    assert len(case.keep) == len(set(case.keep)) == 256 and case.cap == 256 * sc.CELLS and max(max(t) for t in case.keep) == 32767
    assert (15, 14) in case.keep
    for f in range(2):
        n = len(sc.decode_candidates(case, f)[0])
        assert 250 <= n <= 310, n
        assert len(sc.decode_reference(case)[f][0]) < n                      # something is suppressed


# ------------------------------------------------------------------------------------------------- the other references
def test_identity_reference_rows_are_the_kernels_rows():
    for c in family('ided'):
        for quirk in (True, False):
            vals = sc.ided_reference(c, quirk)
            assert vals.shape == ((c.n_ids if c.n_rows is None else c.n_rows), 3 * len(c.count))
            assert np.isnan(vals).any() and (~np.isnan(vals)).any()
        on, off = sc.ided_reference(c, True), sc.ided_reference(c, False)
        assert not np.array_equal(np.isnan(on), np.isnan(off))                   # the label quirk moves columns
        assert np.isnan(off[:, 3 * 1019:3 * 1029]).all()


def test_metrics_reference_edges():
    a, b = family('metrics')
    k7 = int(np.nonzero(a.thrs == 0.7)[0][0])
    cm, fp, fn = sc.metrics_reference(a, k7)
    assert cm[0, 0, 0] >= 6 and fn[0, 6] == 1 and fn[0, 7] == 1        # label (15, 15): its closest (a tie, j = 0) is taken
    assert fn[1, 2] == 1 and fn[1, 1] == 0                              # the second label of a shared closest detection
    assert cm[2].tolist() == [[0] * 13, [0] * 13, [3] * 13]
    # f32(0.59) is not above 0.59: at that threshold the detection is no candidate; f32(0.67) is above 0.67
    t59, t67 = int(np.nonzero(a.thrs == 0.59)[0][0]), int(np.nonzero(a.thrs == 0.67)[0][0])
    fn59 = orc.detection_confusion(*sc.metrics_frame(a, 1), a.thrs, 23, return_masks_at=t59)[1]
    fn67 = orc.detection_confusion(*sc.metrics_frame(a, 1), a.thrs, 23, return_masks_at=t67)[1]
    assert fn59[3] and not fn67[6]
    cm, fp, fn = sc.metrics_reference(b, k7)
    assert cm[0, 0, 0] == 1 and fn[0].tolist()[:2] == [0, 1] and cm[1, 0, 0] == 1 and cm[2].tolist() == [[0] * 13, [0] * 13, [1] * 13]


def test_histogram_reference_edges():
    c = BY_NAME[('hist', 'box70')]
    hist, hsum = sc.hist_reference(c)
    assert not hist[0, 4].any() and not hist[0, 5].any() and not hist[0, 6].any() and hist[0, 0].any() and hsum[0, 0] > 0
