"""Every launch shape of the kernels between the CNN and the solver and behind the solver, through the hotpath wrappers, on the
cases of tests/stagekernel_cases.py: tile occupancy, decode + stitch + NMS (LDS and HBM kernel), observation costs, the
open-grid and table routes of the arc builder (with and without the appearance term and row subsets), the identity table,
the detection metrics, the box histograms and the fused preprocessing pass. tests/test_stagekernels_cpu.py proves on the CPU
that each case reaches the route its facts claim; here the kernels run them against the oracle.

Everything integer or copied is compared exactly; a failure names the first differing frame or slot and the case's route.
Floating point keeps the bounds the project already states: observation costs atol 1e-12 and identical rint(cost * 1e6);
appearance-term units |delta| <= 1 with identical arcs and hash bits; preprocess identical sparsity, <= 2 ulp with the log and
bit-equal without.

Differences observed: none recorded yet. The three floating-point tests print theirs (max |cost - oracle| and the number of
differing costs; the number of arcs whose cost units differ; the largest ulp distance and the number of differing pixels):
run with -s and write them here."""
import numpy as np
import pytest
import torch

import stagekernel_cases as sc
from axtrack_amd import hotpath as hp

pytestmark = pytest.mark.gpu

CASES = sc.all_cases()
_RUNS = {}


def family(name, pred=lambda c: True):
    return [c for c in CASES if c.family == name and pred(c)]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def first_diff(got, want):
    """Index (as a tuple) of the first element that differs, or the shapes if they do."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f'shape {got.shape} != {want.shape}'
    d = np.argwhere(got != want)
    at = tuple(int(v) for v in d[0])
    return f'{len(d)} differ, first at {at}: kernel {got[at]!r}, reference {want[at]!r}'


def check_equal(got, want, case, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want), f'{case.route}: {what}: {first_diff(got, want)}'


# ------------------------------------------------------------------------------------------------- tile occupancy
@pytest.mark.parametrize('case', family('occupancy'), ids=repr)
def test_tile_occupancy(case):
    got = host(hp.tile_occupancy_bytes(dev(case.frames())))
    check_equal(got, sc.occupancy_reference(case), case, 'occupancy byte per tile (row-major)')


# ------------------------------------------------------------------------------------------------- decode + stitch + NMS
@pytest.mark.parametrize('case', family('decode'), ids=repr)
def test_decode_stitch_nms(case):
    conf, x, y, cnt = (host(t) for t in hp.decode_stitch_nms(dev(case.yolo), case.keep, float(case.conf_thr), case.min_dist, case.cap))
    ref = sc.decode_reference(case)
    assert conf.shape == (len(ref), case.cap)
    check_equal(cnt, [len(r[0]) for r in ref], case, 'count per frame')
    for f, (rc, rx, ry) in enumerate(ref):
        n = len(rc)
        check_equal(conf[f, :n].view(np.uint32), rc.view(np.uint32), case, f'frame {f}: confidence bits by rank')
        check_equal(x[f, :n], rx, case, f'frame {f}: x by rank')
        check_equal(y[f, :n], ry, case, f'frame {f}: y by rank')
        for name, a in (('conf', conf.view(np.uint32)), ('x', x), ('y', y)):
            assert not a[f, n:].any(), f'{case.route}: frame {f}: {name} slot {n + int(np.nonzero(a[f, n:])[0][0])} beyond the count is not zero'


# ------------------------------------------------------------------------------------------------- observation costs
@pytest.mark.parametrize('method', ['scale_to_max', 'ceil'])
def test_observation_costs(method):
    case = sc.obs_case()
    got = host(hp.obs_costs(dev(case.conf), dev(case.count), method, case.max_conf_cost))
    ref = sc.obs_reference(case, method)
    valid = np.arange(case.conf.shape[1])[None] < case.count[:, None]
    assert not got[~valid].any(), f'{case.route}: a cost beyond a frame\'s count was written: {first_diff(got * ~valid, ref * 0)}'
    err = np.abs(got - ref)[valid]
    print(f'obs {method}: max |cost - oracle| = {err.max():.3e}, {int((err > 0).sum())} of {err.size} differ')
    assert err.max() <= 1e-12, f'{case.route}: {method}: {first_diff(np.abs(got - ref) <= 1e-12, np.ones(got.shape, bool))}'
    check_equal(np.rint(got * 1e6), np.rint(ref * 1e6), case, f'{method}: rint(cost * 1e6)')
    if method == 'scale_to_max':
        assert got[1, 0] == case.max_conf_cost and got[3, 150] == -case.max_conf_cost


# ------------------------------------------------------------------------------------------------- arcs
def _build(case):
    """hp.build_arcs on the case, once per session: dict of host arrays (row_ptr cut to n_det + 1)."""
    if case.name not in _RUNS:
        H, W = case.shape
        vis = None
        if case.vis is not None:
            vis = dict(case.vis, hist=dev(case.vis['hist']), hsum=dev(case.vis['hsum']))
        src = dev(case.src_count.astype(np.int32)) if case.src_count is not None else None
        tab = dev(case.length_table) if case.length_table is not None else None
        row_ptr, col, length, gap, cost = hp.build_arcs(dev(case.x), dev(case.y), dev(case.count), H, W, case.dmax, case.units, None,
                                                        case.max_dist, case.conn8, vis, tab, src)
        n_det = int(np.minimum(case.count, case.x.shape[1]).sum())
        _RUNS[case.name] = dict(row_ptr=host(row_ptr)[:n_det + 1], col=host(col), length=host(length), gap=host(gap), cost=host(cost))
    return _RUNS[case.name]


def _where(ref, case, e):
    """Arc number e of the reference in words."""
    f = lambda k: (int(np.searchsorted(ref.offs, k, 'right') - 1), int(k - ref.offs[np.searchsorted(ref.offs, k, 'right') - 1]))
    return f'tail (frame, slot) {f(ref.tail[e])} -> head {f(int(ref.col[e]))}, gap {int(ref.gap[e])}, length {int(ref.length[e])}'


def _check_structure(got, ref, case):
    rp = got['row_ptr']
    if not np.array_equal(rp, ref.row_ptr):
        k = int(np.nonzero(rp != ref.row_ptr)[0][0])
        t = int(np.searchsorted(ref.offs, max(k - 1, 0), 'right') - 1)
        raise AssertionError(f'{case.route}: row_ptr differs first at detection {k} (row {k - 1} is frame {t} slot {k - 1 - int(ref.offs[t])}): '
                             f'kernel {rp[k]}, reference {ref.row_ptr[k]}')
    for name in ('col', 'length', 'gap'):
        a, b = got[name], getattr(ref, name)
        assert a.dtype == b.dtype and a.shape == b.shape, f'{case.route}: {name}: {a.dtype}{a.shape} != {b.dtype}{b.shape}'
        if not np.array_equal(a, b):
            e = int(np.nonzero(a != b)[0][0])
            raise AssertionError(f'{case.route}: {name} differs in {int((a != b).sum())} arcs, first arc {e}: kernel {a[e]}, reference '
                                 f'{_where(ref, case, e)}')


@pytest.mark.parametrize('case', family('arcs', lambda c: c.vis is None), ids=repr)
def test_open_grid_and_table_arcs(case):
    """All five outputs of hp.build_arcs equal the CSR builder's: row_ptr, col, length, gap and the integer cost."""
    got, ref = _build(case), sc.arcs_reference(case)
    assert len(ref.col) > 50
    _check_structure(got, ref, case)
    if not np.array_equal(got['cost'], ref.cost):
        e = int(np.nonzero(got['cost'] != ref.cost)[0][0])
        raise AssertionError(f'{case.route}: cost differs in {int((got["cost"] != ref.cost).sum())} arcs, first arc {e}: kernel '
                             f'{got["cost"][e]} (units {got["cost"][e] >> 16}), reference {ref.cost[e]} (units {ref.cost[e] >> 16}), {_where(ref, case, e)}')


def test_row_subsets_add_up_to_the_whole_on_the_gpu():
    by = {c.name: c for c in family('arcs')}
    whole, lo, hi = (_build(by[n]) for n in ('many_detections', 'rows_frames_0_2', 'rows_frames_3_7'))
    for k in ('col', 'length', 'gap', 'cost'):
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), whole[k]), f'rows of frames 0-2 + rows of frames 3-7 != the whole: {k}'
    assert np.array_equal(np.diff(lo['row_ptr']) + np.diff(hi['row_ptr']), np.diff(whole['row_ptr']))


@pytest.mark.parametrize('case', family('arcs', lambda c: c.vis is not None), ids=repr)
def test_arcs_with_the_appearance_term(case):
    """Identical arc set and hash bits; the f64 log of the GPU is within 1 ulp, so the cost units may differ by one."""
    got = _build(case)
    ref, _, margin = sc.vis_csr(case)
    assert margin > 1e-9 and len(ref.col) > 500
    _check_structure(got, ref, case)
    check_equal(got['cost'] & 0xFFFF, ref.cost & 0xFFFF, case, 'identity hash bits of the cost')
    du = (got['cost'] >> 16) - (ref.cost >> 16)
    print(f'{case.name}: {int((du != 0).sum())} of {len(du)} arcs differ in their cost units (max |delta| {int(np.abs(du).max())})')
    if np.abs(du).max() > 1:
        e = int(np.nonzero(np.abs(du) > 1)[0][0])
        raise AssertionError(f'{case.route}: cost units differ by {int(du[e])} at arc {e}: {_where(ref, case, e)}')


# ------------------------------------------------------------------------------------------------- identity table
@pytest.mark.parametrize('quirk', [True, False], ids=['quirk', 'plain'])
@pytest.mark.parametrize('case', family('ided'), ids=repr)
def test_identity_table(case, quirk):
    table, wait = hp.ided_table(dev(case.track), dev(case.conf), dev(case.x), dev(case.y), dev(case.count), case.n_ids, quirk,
                                dev(case.id_row) if case.id_row is not None else None, case.n_rows)
    wait()
    ref = sc.ided_reference(case, quirk)
    got = np.array(table)
    assert got.shape == ref.shape
    a, b = got.view(np.uint64), np.ascontiguousarray(ref).view(np.uint64)
    if not np.array_equal(a, b):
        r, c = (int(v) for v in np.argwhere(a != b)[0])
        raise AssertionError(f'{case.route} (label quirk {quirk}): {int((a != b).sum())} cells differ, first in row {r}, column {c} '
                             f'(label slot {c // 3}, {("anchor_x", "anchor_y", "conf")[c % 3]}): kernel {got[r, c]!r}, reference {ref[r, c]!r}')


# ------------------------------------------------------------------------------------------------- detection metrics
@pytest.mark.parametrize('k_mask', [-1, 4], ids=['no_masks', 'masks_at_0.7'])
@pytest.mark.parametrize('case', family('metrics'), ids=repr)
def test_detection_confusion(case, k_mask):
    assert k_mask < 0 or case.thrs[k_mask] == 0.7
    args = [dev(a) for a in (case.conf, case.x, case.y, case.count, case.gx, case.gy, case.gcount)]
    out = hp.detection_confusion(*args, case.thrs, case.min_dist, k_mask)
    cm, fp, fn = sc.metrics_reference(case, k_mask)
    if k_mask < 0:
        assert isinstance(out, torch.Tensor)
        check_equal(host(out), cm, case, 'confusion [frame, (TP, FP, FN), threshold]')
        return
    check_equal(host(out[0]), cm, case, 'confusion [frame, (TP, FP, FN), threshold]')
    check_equal(host(out[1]), fp, case, 'FP mask [frame, detection]')
    check_equal(host(out[2]), fn, case, 'FN mask [frame, label]')


# ------------------------------------------------------------------------------------------------- box histograms
@pytest.mark.parametrize('case', family('hist'), ids=repr)
def test_box_histograms(case):
    hist, hsum = (host(t) for t in hp.box_histograms(dev(case.frames), dev(case.x), dev(case.y), dev(case.count), case.t_offset, case.box))
    r_hist, r_sum = sc.hist_reference(case)
    check_equal(hist.view(np.uint32), r_hist.view(np.uint32), case, 'histogram bits [frame, detection, bin]')
    check_equal(hsum.view(np.uint64), r_sum.view(np.uint64), case, 'bin sum bits [frame, detection]')


# ------------------------------------------------------------------------------------------------- preprocess
@pytest.mark.parametrize('case', family('prep'), ids=repr)
def test_preprocess(case):
    T, H, W = case.raw.shape
    raw = dev(case.raw.view(np.int16))
    mask = dev(case.mask.astype(np.uint8)) if case.mask is not None else None
    ref = sc.prep_reference(case)
    if case.out_slice:
        buf = torch.full((T + 2, H, W), float('nan'), dtype=torch.float32, device='cuda')
        out = hp.preprocess_u16(raw, mask, case.offset, case.clip, case.log, case.scale, out=buf[1:T + 1])
        assert out.data_ptr() == buf[1].data_ptr()
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[T + 1]).all()), f'{case.route}: wrote outside the out= slice'
    else:
        out = torch.full((T, H, W), float('nan'), dtype=torch.float32, device='cuda')          # NaN: what the kernel did not write shows
        hp.preprocess_u16(raw, mask, case.offset, case.clip, case.log, case.scale, out=out)
    got = host(out)
    unwritten = np.isnan(got)
    assert not unwritten.any(), f'{case.route}: {int(unwritten.sum())} pixels not written, first at (t, y, x) {tuple(int(v) for v in np.argwhere(unwritten)[0])}'
    check_equal(got == 0, ref == 0, case, 'sparsity pattern (t, y, x)')
    if case.log:
        a, b = got.view(np.int32).astype(np.int64), ref.view(np.int32).astype(np.int64)          # non-negative floats: bits order like values
        ulp = np.abs(a - b)
        print(f'prep {case.name}: max {int(ulp.max())} ulp, {int((ulp > 0).sum())} of {ulp.size} pixels differ')
        assert ulp.max() <= 2, f'{case.route}: {first_diff(ulp <= 2, np.ones(ulp.shape, bool))}'
    else:
        check_equal(got.view(np.uint32), ref.view(np.uint32), case, 'output bits (t, y, x)')
