"""The argument contract of the C ABI on the device: in-contract calls only (tests/contract_cases.py is the table; its
refusals never come here, tests/test_contract_cpu.py makes them where no device is visible).

  decode, distant tiles   twins 128 and 91 tiles apart (columns and rows, LDS and HBM kernel): the square of their distance
                          does not fit 32 bits; bit-equal to stagekernel_cases.decode_reference, which keeps both;
  decode, 256 tiles       n_tiles == 256, cap == 256 * 144, the largest tile index;
  every limit call        the smallest and largest accepted value of every bound: returns AXT_OK, and where the family has a
                          reference (REFERENCES below), equals it under the family's own comparison;
  h_dmax == max_dist      with path lengths from a table (arcs) and from a grid's searches (pairs), priced by cost units:
                          the largest combination the units table can serve.

Compared against a reference (REFERENCES): every family that has one in tests/ -- stagekernel_cases, the oracle's path
lengths, hungarian_reference, recon_reference, target_reference, mot_reference, segment_reference, render_cases. The few limit
calls that are run for AXT_OK only are named, with the reason, by contract_cases.uncompared(); the entry points without a
reference in tests/ for a single call (the pools, the tile stacks, TIFF, JPEG, the augmentation, the framewise and statistics
passes of the preprocessing, the host-side solver) are run for AXT_OK, and their families' own tests hold their references."""
import ctypes

import numpy as np
import pytest
import torch

import contract_cases as cc
import hungarian_reference as hr
import recon_reference as rr
import stagekernel_cases as sc
from axtrack_amd import _lib
from axtrack_amd import hotpath as hp
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

TORCH = {np.float32: torch.float32, np.float64: torch.float64, np.int8: torch.int8, np.uint8: torch.uint8, np.int16: torch.int16,
         np.uint16: torch.int16, np.int32: torch.int32, np.int64: torch.int64}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def to_device(v):
    """A Dev of the table as a device tensor (at least one element, so that its address is never NULL)."""
    n = int(np.prod(v.shape, dtype=np.int64))
    if v.data is not None and n > 0:
        a = v.data.view(np.int16) if v.data.dtype == np.uint16 else v.data
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = torch.full((max(n, 1),), v.fill, dtype=TORCH[v.dtype], device='cuda')
    return t.view(v.shape) if n > 0 else t


def launch(call):
    """Makes the call with every Dev on the device. Returns (rc, {name: tensor or host array}, {name: scalar})."""
    lib = _lib.load()
    cc.LIB = lib
    fn = getattr(lib, call.function)
    held, scalars, cargs = {}, {}, []
    for (name, v), t in zip(call.args, fn.argtypes):
        if isinstance(v, cc.Dev):
            held[name] = to_device(v)
            p = held[name].data_ptr()
        elif isinstance(v, cc.Host):
            held[name] = v.data.copy()
            p = held[name].ctypes.data
        else:
            scalars[name] = v
            cargs.append(v)
            continue
        cargs.append(ctypes.cast(ctypes.c_void_p(p), t) if isinstance(t, type) and issubclass(t, ctypes._Pointer) else p)
    rc = fn(*cargs)
    torch.cuda.synchronize()
    return rc, held, scalars


def check_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f'{what}: shape {got.shape} != {want.shape}'
    if not np.array_equal(got, want):
        at = tuple(int(v) for v in np.argwhere(got != want)[0])
        raise AssertionError(f'{what}: {int((got != want).sum())} differ, first at {at}: kernel {got[at]!r}, reference {want[at]!r}')


# ===================================================================================================== decode
def check_decode(case, conf, x, y, cnt):
    """As tests/test_stagekernels_gpu.py::test_decode_stitch_nms compares: bit for bit, by rank."""
    ref = sc.decode_reference(case)
    check_equal(cnt, [len(r[0]) for r in ref], f'{case.route}: count per frame')
    for f, (rc, rx, ry) in enumerate(ref):
        n = len(rc)
        check_equal(conf[f, :n].view(np.uint32), rc.view(np.uint32), f'{case.route}: frame {f}: confidence bits by rank')
        check_equal(x[f, :n], rx, f'{case.route}: frame {f}: x by rank')
        check_equal(y[f, :n], ry, f'{case.route}: frame {f}: y by rank')


def run_decode(case):
    return [host(t) for t in hp.decode_stitch_nms(dev(case.yolo), case.keep, float(case.conf_thr), case.min_dist, case.cap)]


@pytest.mark.parametrize('case', sc.distant_tiles_cases(), ids=repr)
def test_decode_keeps_twins_in_distant_tiles(case):
    """A kernel that forms dx * dx + dy * dy in int drops the less confident twin: the count is short by one per frame."""
    check_decode(case, *run_decode(case))


def test_decode_at_256_tiles():
    case = sc.decode_256_tiles_case()
    conf, x, y, cnt = run_decode(case)
    assert conf.shape == (2, 256 * sc.CELLS)
    check_decode(case, conf, x, y, cnt)


# ===================================================================================================== references of limit calls
def _case(**kw):
    return sc.Case('limit', 'limit', [], **kw)


def ref_tile_occupancy(call, held, s):
    fr = host(held['d_frames']).reshape(s['T_all'], s['H'], s['W'])
    occ = np.zeros(orc.tile_grid(s['H'], s['W']), np.uint8)
    for iy, ix in orc.kept_tiles(fr):
        occ[iy, ix] = 1
    check_equal(host(held['d_occ']), occ.reshape(-1), f'{call.id}: occupancy byte per tile')


def ref_decode(call, held, s):
    F, cap = s['n_frames'], s['cap']
    cnt = host(held['d_count'])[:F]
    if F == 0:
        assert (host(held['d_count']) == -7).all(), f'{call.id}: n_frames == 0 touched the counts'
        return
    case = _case(yolo=host(held['d_yolo']).reshape(F, s['n_tiles'], 12, 12, 3), keep=[tuple(t) for t in held['h_tile_yx'].reshape(-1, 2)],
                 conf_thr=np.float32(s['conf_thr']), min_dist=s['min_dist'], cap=cap)
    check_decode(case, host(held['d_conf']).reshape(F, cap), host(held['d_x']).reshape(F, cap), host(held['d_y']).reshape(F, cap), cnt)


def ref_obs_costs(call, held, s):
    F, cap = s['n_frames'], s['cap']
    if F == 0:
        return
    case = _case(conf=host(held['d_conf']).reshape(F, cap), count=host(held['d_count'])[:F], max_conf_cost=s['max_conf_cost'])
    got, ref = host(held['d_cost']).reshape(F, cap), sc.obs_reference(case, ('scale_to_max', 'ceil')[s['method']])
    valid = np.arange(cap)[None] < case.count[:, None]
    assert np.abs(got - ref)[valid].max() <= 1e-12, f'{call.id}: max |cost - oracle| = {np.abs(got - ref)[valid].max():.3e}'
    check_equal(np.rint(got * 1e6)[valid], np.rint(ref * 1e6)[valid], f'{call.id}: rint(cost * 1e6)')
    assert not got[~valid].any(), f'{call.id}: a cost beyond a frame\'s count was written'


def ref_preprocess(call, held, s):
    T, H, W = s['T'], s['H'], s['W']
    raw = host(held['d_raw']).view(np.uint16).reshape(T, H, W)
    mask = host(held['d_mask']).reshape(H, W).astype(bool) if 'd_mask' in held else None
    with np.errstate(over='ignore', divide='ignore'):
        ref = orc.preprocess(raw, mask, s['offset'], s['clip_lower'], bool(s['log_correct']), s['scale'])
    got = host(held['d_out']).reshape(T, H, W)
    check_equal(got == 0, ref == 0, f'{call.id}: sparsity pattern (t, y, x)')
    fin = np.isfinite(ref)
    check_equal(np.isfinite(got), fin, f'{call.id}: finite values (t, y, x)')
    ulp = np.abs(got[fin].view(np.int32).astype(np.int64) - ref[fin].view(np.int32).astype(np.int64))
    assert ulp.max(initial=0) <= (2 if s['log_correct'] else 0), f'{call.id}: {int(ulp.max())} ulp'
    check_equal(got[~fin], ref[~fin], f'{call.id}: infinite values')


def ref_box_histograms(call, held, s):
    F, cap = s['n_frames'], s['cap']
    case = _case(frames=host(held['d_frames']).reshape(s['T_all'], s['H'], s['W']), x=host(held['d_x']).reshape(F, cap),
                 y=host(held['d_y']).reshape(F, cap), count=host(held['d_count'])[:F], t_offset=s['t_offset'], box=s['box'])
    r_hist, r_sum = sc.hist_reference(case)
    valid = np.arange(cap)[None] < case.count[:, None]
    check_equal(host(held['d_hist']).reshape(F, cap, 180)[valid].view(np.uint32), r_hist[valid].view(np.uint32), f'{call.id}: histogram bits')
    check_equal(host(held['d_hist_sum']).reshape(F, cap)[valid].view(np.uint64), r_sum[valid].view(np.uint64), f'{call.id}: bin sum bits')


def ref_path_cost(call, held, s):
    na, nb = s['na'], s['nb']
    if na * nb == 0:
        assert (host(held['d_D']) == -3).all(), f'{call.id}: an empty call wrote D'
        return
    i64 = lambda n, k: host(held[n])[:k].astype(np.int64)
    D = orc.path_matrix((None, i64('d_xa', na), i64('d_ya', na)), (None, i64('d_xb', nb), i64('d_yb', nb)), s['H'], s['W'], None, s['max_dist'],
                        bool(s['conn8']))
    check_equal(host(held['d_D']).reshape(na, nb), D, f'{call.id}: D [na, nb]')


def _arc_inputs(held, s):
    F, cap = s['n_frames'], s['cap']
    return host(held['d_x']).reshape(F, cap), host(held['d_y']).reshape(F, cap), host(held['d_count'])[:F], held['h_dmax'].copy()


def ref_build_arcs(call, held, s):
    """Both phases through hp.build_arcs on the call's own inputs, against the CSR builder of the stage-kernel tests."""
    if cc.uncompared(call.function, dict(s, vis='d_hist' in held)):
        return
    x, y, count, dmax = _arc_inputs(held, s)
    tab = host(held['d_len_table']).reshape(s['n_frames'], s['cap'], s['max_gap'], s['cap']) if 'd_len_table' in held else None
    units = host(held['d_cost_units']) if 'd_cost_units' in held else None
    H, W = s['H'], s['W']
    row_ptr, col, length, gap, cost = hp.build_arcs(dev(x), dev(y), dev(count), H, W, dmax, units, None, s['max_dist'], bool(s['conn8']), None,
                                                    dev(tab) if tab is not None else None, None)
    ref = sc.open_grid_csr(x, y, count, H, W, dmax, bool(s['conn8']), s['max_dist'], units, None, tab)
    n_det = int(np.minimum(count, s['cap']).sum())
    check_equal(host(row_ptr)[:n_det + 1], ref.row_ptr, f'{call.id}: row_ptr')
    check_equal(held['n_arcs'], [len(ref.col)], f'{call.id}: *n_arcs of the counting phase')
    for name, got in (('col', col), ('length', length), ('gap', gap)):
        check_equal(host(got), getattr(ref, name), f'{call.id}: {name}')
    if units is not None:
        check_equal(host(cost), ref.cost, f'{call.id}: integer cost')


def open_grid_costs(x, y, count, H, W, dmax, units, max_dist, conn8, searched=False):
    """{(t, gap): i64 [n_t, n_t+gap]} as axt_hungarian_pairs prices links on an all-ones mask from path lengths and units:
    admitted iff the length is <= dmax[gap - 1]. The closed form answers max_dist where it has no path (a gate fails), and a
    limit that is not below max_dist admits that answer too; a grid's searches (searched=True) report no length for such a
    pair, so it is never admitted."""
    counts = [int(c) for c in count]
    offs = hr.offsets(counts)
    out = {}
    for g in range(1, len(dmax) + 1):
        for t in range(len(counts) - g):
            n, m = counts[t], counts[t + g]
            xa, ya, xb, yb = (v.astype(np.int64) for v in (x[t, :n, None], y[t, :n, None], x[t + g, None, :m], y[t + g, None, :m]))
            dx, dy = np.abs(xa - xb), np.abs(ya - yb)
            L = (np.maximum(dx, dy) if conn8 else dx + dy) + 1
            inb = (xa >= 0) & (xa < W) & (ya >= 0) & (ya < H) & (xb >= 0) & (xb < W) & (yb >= 0) & (yb < H)
            has_path = (dx * dx + dy * dy < max_dist * max_dist) & (L <= max_dist) & inb
            L = np.where(has_path, L, max_dist)
            adm = (L <= dmax[g - 1]) & (has_path | (not searched))
            cost = hr.arc_cost_vec(units[g - 1, np.minimum(L, max_dist)], 3, offs[t] + np.arange(n)[:, None], offs[t + g] + np.arange(m)[None, :])
            out[(t, g)] = np.where(adm, cost, hr.NO_LINK)
    return out


def ref_hungarian_pairs(call, held, s):
    """The whole association through hp.hungarian_assoc (pairs, then chains) on the call's inputs, judged as the Hungarian
    tests judge: a matching of admitted links, every pair at its integer optimum, the reference's trajectories."""
    if cc.uncompared(call.function, s):
        return
    x, y, count, dmax = _arc_inputs(held, s)
    units = host(held['d_cost_units'])
    track, n = hp.hungarian_assoc(dev(x), dev(y), dev(count), s['H'], s['W'], dmax, units, s['thr_units'], s['max_dist'], bool(s['conn8']))
    costs = open_grid_costs(x, y, count, s['H'], s['W'], dmax, units, s['max_dist'], bool(s['conn8']))
    hr.judge(costs, count, host(track), int(n.item()), name=call.id, thr_units=s['thr_units'], max_gap=s['max_gap'])


def ref_track_links(call, held, s):
    F, cap = s['n_frames'], s['cap']
    if F == 0:
        check_equal(held['n_links'], [0], f'{call.id}: *n_links')
        return
    ref = rr.track_links(host(held['d_track']).reshape(F, cap), host(held['d_count'])[:F], s['max_gap'])
    check_equal(held['n_links'], [len(ref)], f'{call.id}: *n_links')
    check_equal(host(held['d_links']).reshape(-1, 3)[:len(ref)], ref, f'{call.id}: links (tail slot, head slot, gap)')


def ref_ided_table(call, held, s):
    """The family's reference where every row occurs (sc.ided_reference needs that), and its definition in plain numpy always:
    NaN, then (x, y, conf) of the detection that carries the row's identity, at columns 3 f."""
    F, cap, n_ids, n_rows = s['n_frames'], s['cap'], s['n_ids'], s['n_rows']
    if n_rows == 0:
        assert not host(held['d_table']).any(), f'{call.id}: n_rows == 0 wrote the table'
        return
    track, conf = host(held['d_track']).reshape(F, cap), host(held['d_conf']).reshape(F, cap)
    x, y, count = host(held['d_x']).reshape(F, cap), host(held['d_y']).reshape(F, cap), host(held['d_count'])[:F]
    want = np.full((n_rows, 3 * F), np.nan)
    for f in range(F):
        for k in range(min(int(count[f]), cap)):
            if 0 <= track[f, k] < n_ids:
                want[track[f, k], 3 * f:3 * f + 3] = (x[f, k], y[f, k], conf[f, k])
    got = host(held['d_table']).reshape(n_rows, 3 * F)
    check_equal(got.view(np.uint64), want.view(np.uint64), f'{call.id}: table bits [row, 3 frame + (x, y, conf)]')
    if n_rows <= int(track[:, :max(int(count.max()), 1)].max()) + 1:
        case = _case(track=track, conf=conf, x=x, y=y, count=count, n_ids=n_ids, id_row=None, n_rows=n_rows)
        check_equal(got.view(np.uint64), np.ascontiguousarray(sc.ided_reference(case, bool(s['label_quirk']))).view(np.uint64),
                    f'{call.id}: table bits against orc.ided_dets_all')


def ref_detection_confusion(call, held, s):
    F, cap, gcap, n_thr = s['n_frames'], s['cap'], s['gcap'], s['n_thr']
    if cc.uncompared(call.function, s):
        return
    case = _case(conf=host(held['d_conf']).reshape(F, cap), x=host(held['d_x']).reshape(F, cap), y=host(held['d_y']).reshape(F, cap),
                 count=host(held['d_count'])[:F], gx=host(held['d_gx']).reshape(F, gcap), gy=host(held['d_gy']).reshape(F, gcap),
                 gcount=host(held['d_gcount'])[:F], thrs=host(held['d_thrs']), min_dist=s['min_dist'])
    cm, fp, fn = sc.metrics_reference(case, s['k_mask'])
    check_equal(host(held['d_confusion']).reshape(F, 3, n_thr), cm, f'{call.id}: confusion [frame, (TP, FP, FN), threshold]')
    if s['k_mask'] >= 0:
        check_equal(host(held['d_fp_mask']).reshape(F, cap), fp, f'{call.id}: FP mask')
        check_equal(host(held['d_fn_mask']).reshape(F, gcap), fn, f'{call.id}: FN mask')


def ref_mot_scores(call, held, s):
    """Counts and tallies against mot_reference.reference, exactly, as tests/test_mot_scores_gpu.py compares them; of a large
    batch of (identical) associations the first and the last."""
    import mot_reference as mr
    K, F, cap, gcap = s['n_assoc'], s['n_frames'], s['cap'], s['gcap']
    scene = dict(x=host(held['d_x']).reshape(F, cap), y=host(held['d_y']).reshape(F, cap), count=host(held['d_count'])[:F],
                 tracks=host(held['d_track']).reshape(K, F, cap), gid=host(held['d_gid']).reshape(F, gcap), gx=host(held['d_gx']).reshape(F, gcap),
                 gy=host(held['d_gy']).reshape(F, gcap), gcount=host(held['d_gcount'])[:F], max_dist=s['max_dist'], no=s['no'], nh=s['nh'])
    counts, tallies = host(held['d_counts']).reshape(K, 10), host(held['d_tallies']).reshape(K, s['no'], 2)
    for k in sorted({0, K - 1}):
        ref = mr.reference(scene, k)
        assert counts[k].tolist() == ref['counts'].tolist(), f'{call.id}: counts of association {k}'
        assert tallies[k].tolist() == ref['tallies'].tolist(), f'{call.id}: tallies of association {k}'


def ref_render_frames(call, held, s):
    import render_cases as rc
    n, H, W = s['n_out'], s['H'], s['W']
    if n == 0:
        assert not host(held['d_out']).any(), f'{call.id}: n_out == 0 wrote pixels'
        return
    case = rc.Case('limit', [], host(held['d_frames']).reshape(-1, H, W), None, host(held['d_ts'])[:n], (s['ymin'], s['xmin'], s['Ho'], s['Wo']),
                   s['grid'], s['bg'], [], [0, 0, 0, 0], [])
    check_equal(host(held['d_out']).reshape(n, s['Ho'], s['Wo'], 3), rc.reference(case), f'{call.id}: pixels [frame, y, x, rgb]')


def ref_target_field(call, held, s):
    import target_reference as tr
    H, W = s['H'], s['W']
    if cc.uncompared(call.function, s):
        return
    off, moves = tr.field(np.ones((H, W), np.uint8), host(held['d_target_cells'])[:s['n_targets']], bool(s['conn8']))
    check_equal(host(held['d_off']).reshape(H, W), off, f'{call.id}: off-mask cells')
    check_equal(host(held['d_moves']).reshape(H, W), moves, f'{call.id}: moves')


def ref_target_sample(call, held, s):
    import target_reference as tr
    F, cap, H, W = s['n_frames'], s['cap'], s['H'], s['W']
    if F == 0:
        return
    off, moves = host(held['d_off']).reshape(-1, H, W)[0], host(held['d_moves']).reshape(-1, H, W)[0]       # (one field: no index)
    x, y, count = host(held['d_x']).reshape(F, cap), host(held['d_y']).reshape(F, cap), host(held['d_count'])[:F]
    eo, em = tr.sample(off, moves, x, y)
    valid = np.arange(cap)[None] < count[:, None]
    check_equal(host(held['d_det_off']).reshape(F, cap), np.where(valid, eo, -1), f'{call.id}: off at the detections')
    check_equal(host(held['d_det_moves']).reshape(F, cap), np.where(valid, em, -1), f'{call.id}: moves at the detections')


def ref_target_paths(call, held, s):
    """The counting phase (d_cells == NULL): cell_ptr = prefix sum of moves + 1, 0 where moves is -1."""
    slots = s['n_frames'] * s['cap']
    m = host(held['d_det_moves'])[:slots].astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum(np.where(m >= 0, m + 1, 0))])
    check_equal(host(held['d_cell_ptr'])[:slots + 1], ptr, f'{call.id}: cell_ptr')
    check_equal(held['n_cells'], [ptr[-1]], f'{call.id}: *n_cells')


U32 = 2.0 ** -24                                  # unit roundoff of f32 (tests/test_segment_gpu.py)


def ref_segment_edges(call, held, s):
    """The bounds tests/test_segment_gpu.py derives: P within 8 U of the f64 Prewitt magnitude, G within (2 (2 r + 2) + 2) U of
    the f64 Gaussian of the kernel's own P, the minimum and maximum exact."""
    import segment_reference as sr
    H, W, sigma = s['H'], s['W'], s['sigma']
    img = host(held['d_img']).view(np.uint16).reshape(H, W)
    P, G, mm = host(held['d_P']).reshape(H, W), host(held['d_G']).reshape(H, W), host(held['d_minmax'])
    ref = sr.edge_magnitude(img)
    assert (np.abs(P - ref) <= 8 * U32 * ref).all(), f'{call.id}: P is off by {(np.abs(P - ref) / np.maximum(ref, 1e-300)).max() / U32:.2f} U > 8 U'
    r = sr.radius_of(sigma)
    ref = sr.smooth(P, sigma) if r > 0 else P.astype(np.float64)           # (radius 0: one tap of weight 1)
    bound = (2 * (2 * r + 2) + 2) * U32
    assert (np.abs(G - ref) <= bound * ref).all(), f'{call.id}: G is off by more than {bound / U32:.0f} U'
    assert mm[0] == G.min() and mm[1] == G.max(), f'{call.id}: min / max'


def ref_segment_histogram(call, held, s):
    import segment_reference as sr
    check_equal(host(held['d_hist']), sr.histogram(host(held['d_G'])[:s['n']], s['mn'], s['mx']), f'{call.id}: counts per bin')


def ref_segment_close(call, held, s):
    import segment_reference as sr
    H, W = s['H'], s['W']
    want = sr.closing(host(held['d_P']).reshape(H, W).astype(np.float64) > s['thr'], s['k'])
    check_equal(host(held['d_out']).reshape(H, W), want.astype(np.uint8), f'{call.id}: closed image')


def ref_segment_flood(call, held, s):
    import segment_reference as sr
    H, W = s['H'], s['W']
    want = sr.flood(host(held['d_img']).reshape(H, W), (s['seed_y'], s['seed_x']), 2 if s['conn8'] else 1)
    check_equal(host(held['d_out']).reshape(H, W), want.astype(np.uint8), f'{call.id}: flooded cells')


def ref_link_paths(call, held, s):
    """grid == NULL: the closed-form staircase of recon_reference.open_path_cells per link, max_dist where it has none."""
    n, cap, H, W, max_dist = s['n_links'], s['cap'], s['H'], s['W'], s['max_dist']
    if n == 0:
        return
    x, y, links = host(held['d_x']).reshape(-1), host(held['d_y']).reshape(-1), host(held['d_links']).reshape(-1, 3)
    length, stage = host(held['d_len'])[:n], host(held['d_stage']).reshape(-1, max_dist)
    for l, (a, b, _) in enumerate(links[:n]):
        p = rr.open_path_cells(H, W, bool(s['conn8']), int(x[a]), int(y[a]), int(x[b]), int(y[b]), max_dist)
        assert length[l] == (max_dist if p is None else len(p)), f'{call.id}: link {l}: length {length[l]}'
        if p is not None:
            check_equal(stage[l, :len(p)], np.asarray(p), f'{call.id}: link {l}: cells')


def ref_link_cells(call, held, s):
    """The counting phase (d_cells == NULL): cell_ptr as recon_reference.link_cells sums the lengths (none at max_dist)."""
    n = s['n_links']
    lens = host(held['d_len'])[:n]
    ptr = rr.link_cells(lens, [np.zeros(max(int(v), 0), np.int64) for v in lens], [1] * n, s['max_dist'], 1)[0] if n else np.zeros(1, np.int64)
    check_equal(host(held['d_cell_ptr'])[:n + 1], ptr, f'{call.id}: cell_ptr')
    check_equal(held['n_cells'], [ptr[-1]], f'{call.id}: *n_cells')


REFERENCES = {'axt_tile_occupancy': ref_tile_occupancy, 'axt_decode_stitch_nms': ref_decode, 'axt_obs_costs': ref_obs_costs,
              'axt_preprocess_u16': ref_preprocess, 'axt_box_histograms': ref_box_histograms, 'axt_path_cost': ref_path_cost,
              'axt_build_arcs': ref_build_arcs, 'axt_hungarian_pairs': ref_hungarian_pairs, 'axt_track_links': ref_track_links,
              'axt_ided_table': ref_ided_table, 'axt_detection_confusion': ref_detection_confusion, 'axt_mot_scores': ref_mot_scores,
              'axt_render_frames': ref_render_frames, 'axt_target_field': ref_target_field, 'axt_target_sample': ref_target_sample,
              'axt_target_paths': ref_target_paths, 'axt_segment_edges': ref_segment_edges, 'axt_segment_histogram': ref_segment_histogram,
              'axt_segment_close': ref_segment_close, 'axt_segment_flood': ref_segment_flood, 'axt_link_paths': ref_link_paths,
              'axt_link_cells': ref_link_cells}


@pytest.mark.parametrize('call', cc.limits(), ids=lambda c: c.id)
def test_limit_call(call):
    rc, held, scalars = launch(call)
    assert rc == cc.OK or (call.function.startswith('axt_jpeg_sc') and rc > 0), f'{call.id}: returned {rc}: {_lib.load().axt_last_error().decode()}'
    if call.function in REFERENCES:
        REFERENCES[call.function](call, held, scalars)


# ===================================================================================================== h_dmax == max_dist
def test_arcs_with_table_lengths_equal_to_max_dist():
    """The length-table route at its largest accepted limit, h_dmax[0] == max_dist, with table entries == max_dist priced by the
    last entry of the units table: stagekernel_cases.length_table_case is that case (tests/test_stagekernels_gpu.py runs it
    against open_grid_csr); here its claim is pinned, and the call one step beyond is the table's refusal."""
    case = sc.length_table_case()
    assert case.dmax[0] == case.max_dist and case.units.shape == (2, case.max_dist + 1)
    assert any(v == case.max_dist and g == 1 for _, _, g, _, v in case.edits)
    ref = sc.arcs_reference(case)
    assert ((ref.length == case.max_dist) & (ref.gap == 1)).sum() >= 3
    assert any('h_dmax[g] <= max_dist' in c.id for c in cc.refusals() if c.function == 'axt_build_arcs')
    row_ptr, col, length, gap, cost = hp.build_arcs(dev(case.x), dev(case.y), dev(case.count), *case.shape, case.dmax, case.units, None,
                                                    case.max_dist, case.conn8, None, dev(case.length_table), None)
    at = host(length) == case.max_dist
    check_equal(host(cost)[at], ref.cost[ref.length == case.max_dist], 'cost of the arcs whose length is max_dist')


def test_pairs_with_searched_lengths_equal_to_max_dist():
    """axt_hungarian_pairs with a grid (path lengths from the masked-grid searches, read from a table) and
    h_dmax[g] == max_dist: the largest limit the staged units serve. On an all-ones mask the searched lengths are the closed
    form's, |dx| + |dy| + 1, and the scene holds pairs at exactly max_dist cells."""
    H, W, max_dist, cap, F = 64, 64, 30, 8, 5
    rng = np.random.default_rng(77)
    count = np.array([6, 5, 6, 4, 6], np.int32)
    x = rng.integers(10, 50, (F, cap)).astype(np.int32)
    y = rng.integers(10, 50, (F, cap)).astype(np.int32)
    for t in range(F):                                         # detection 0 of every frame: 20 + 9 + 1 = max_dist cells from the next frame's
        x[t, 0], y[t, 0] = (20, 20) if t % 2 == 0 else (40, 29)
    dmax = np.array([max_dist, max_dist], np.int32)
    units = (np.arange(1, 3)[:, None] * 100000 + np.arange(max_dist + 1)[None] * 1000).astype(np.int64)       # distinct, far below the threshold
    units[:, max_dist] = 777                                   # the table's last entry: a length of max_dist cells is priced by it
    costs = open_grid_costs(x, y, count, H, W, dmax, units, max_dist, False, searched=True)
    at_limit = sum(int(((c[c != hr.NO_LINK] >> 16) == 777).sum()) for c in costs.values())
    assert at_limit >= 4                                       # (0 -> 0 of the four frame pairs at least)
    grid = hp.Grid(np.ones((H, W), np.uint8), False)
    track, n = hp.hungarian_assoc(dev(x), dev(y), dev(count), H, W, dmax, units, hr.THR_UNITS, max_dist, False, mask=grid)
    torch.cuda.synchronize()
    hr.judge(costs, count, host(track), int(n.item()), name='h_dmax == max_dist on a grid', max_gap=2)
