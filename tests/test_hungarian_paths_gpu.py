"""Every dispatch path of the Hungarian association kernels (axtrack_amd/csrc/hungarian.hip) against the SciPy reference
of tests/hungarian_reference.py: the six pair-kernel variants (one to three register slots, nine, column state in LDS), with
and without the cost cache and with no cache at all, the three cost sources (closed form, given table, masked-grid table),
crowded gap-2 passes, frame ranges, and both chain numberings on hand-made links. tests/test_hungarian_cpu.py proves on
the CPU that each case lands in the path its name claims and forces real searches; here the kernels run them and
hungarian_reference.judge says what is wrong, if anything is: matching, admission, optimum per pair, trajectories, padding."""
import numpy as np
import pytest
import torch

import hungarian_reference as hr
from axtrack_amd import _lib, hotpath as hp, params

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _geometry():
    """dmax / units as AxonDetections hands them to the kernels (the one product input of these tests)."""
    from axtrack_amd.detections import transition_cost_table
    table, dmax = transition_cost_table(params.DEPLOYED)
    return dmax, np.where(np.isfinite(table), np.rint(table * 1e6), 0).astype(np.int64)


def _anchors(case):
    F, cap = len(case.counts), case.cap
    x = np.zeros((F, cap), np.int32)
    y = np.zeros((F, cap), np.int32)
    if case.kind == 'geo':
        for t, d in enumerate(case.dets):
            x[t, :len(d[1])] = d[1]
            y[t, :len(d[2])] = d[2]
    return dev(x), dev(y), dev(np.asarray(case.counts, np.int32))


def _run(case):
    """The case through hp.hungarian_assoc: (track i32 [F, cap], n_tracks)."""
    x, y, cnt = _anchors(case)
    if case.kind == 'ctab':
        ctab = dev(hr.costs_to_table(case.costs, case.counts, case.cap, gaps=case.max_gap))
        track, n = hp.hungarian_assoc(x, y, cnt, 1, 1, [0] * case.max_gap, np.zeros((case.max_gap, 2), np.int64), case.thr_units,
                                      ctab=ctab)
    else:
        dmax, units = _geometry()
        grid = hp.Grid(case.mask, False) if case.mask is not None else None
        track, n = hp.hungarian_assoc(x, y, cnt, case.H, case.W, dmax, units, case.thr_units, conn8=case.conn8, mask=grid)
    torch.cuda.synchronize()
    return track.cpu().numpy(), int(n.item())


def _judge(case, track, n):
    hr.judge(case.costs, case.counts, track, n, name=case.name, thr_units=case.thr_units, max_gap=case.max_gap, ref=case.reference)


@pytest.mark.parametrize('case', hr.battery_a(), ids=repr)
def test_open_grid(case):
    """Battery A: clustered, alternating, sparse and lattice scenes with the closed-form path lengths, 4- and 8-connected,
    at slot counts on both sides of every dispatch bound."""
    _judge(case, *_run(case))


@pytest.mark.parametrize('case', hr.battery_b(), ids=repr)
def test_given_cost_table(case):
    """Battery B: link costs handed over as a table (d_ctab of axt_hungarian_pairs): dense random, Machol-Wien, equal units,
    nothing admitted, one row per column -- and admitted links dearer than leaving the row unlinked."""
    _judge(case, *_run(case))


@pytest.mark.parametrize('case', hr.battery_c(), ids=repr)
def test_masked_grid(case):
    """Battery C: path lengths from the masked-grid searches (axt_hungarian_pairs with a grid), crowded."""
    _judge(case, *_run(case))


def _pairs_call(case, a, b, pred, work, cap=None):
    """axt_hungarian_pairs for the source frames [a, b) of a case; cap: another slot count than the case's (anchors re-laid)."""
    dmax, units = _geometry()
    x, y, cnt = _anchors(case)
    if cap is not None:
        pad = torch.zeros((len(case.counts), cap - case.cap), dtype=torch.int32, device='cuda')
        x, y = torch.cat([x, pad], 1).contiguous(), torch.cat([y, pad], 1).contiguous()
    h_dmax = np.ascontiguousarray(dmax, np.int32)
    d_units = dev(units)
    rc = _lib.load().axt_hungarian_pairs(x.data_ptr(), y.data_ptr(), cnt.data_ptr(), len(case.counts), cap or case.cap, None,
                                         case.H, case.W, hp.MAX_PX_ASSOC_DIST, int(case.conn8), 2, h_dmax.ctypes.data,
                                         d_units.data_ptr(), case.thr_units, a, b, pred.data_ptr(), work.data_ptr(), hp._stream(),
                                         None)
    torch.cuda.synchronize()
    return rc


def test_slot_count_beyond_the_limit_is_refused():
    """cap = 2049: an error code and a message, and neither the links nor the work space are touched."""
    case = next(c for c in hr.battery_a() if c.name == 'a64')
    F, cap = len(case.counts), 2049
    pred = torch.full((2 * F * cap,), 7, dtype=torch.int32, device='cuda')
    work = torch.full((2 * F * cap + F + 1,), 7, dtype=torch.int32, device='cuda')
    rc = _pairs_call(case, 0, F, pred, work, cap=cap)
    assert rc < 0 and b'2049' in _lib.load().axt_last_error()
    assert bool((pred == 7).all()) and bool((work == 7).all())
    with pytest.raises(_lib.AxtError):
        z = torch.zeros((F, cap), dtype=torch.int32, device='cuda')
        hp.hungarian_assoc(z, z, dev(np.asarray(case.counts, np.int32)), 300, 300, *_geometry(), case.thr_units)


@pytest.mark.parametrize('name', ['a192_three_slots', 'a576_nc9_deep'])
def test_frame_ranges_combine_to_the_whole(name):
    """The sharding contract in one process: the links of [0, k) and [k, F), combined with an element-wise maximum, equal
    the links of the full range at every split k, and number to the reference's trajectories."""
    case = next(c for c in hr.battery_a() if c.name == name)
    F, cap = len(case.counts), case.cap
    slots = F * cap
    lib = _lib.load()

    def links(a, b):
        pred = torch.full((2 * slots,), 7, dtype=torch.int32, device='cuda')
        work = torch.empty((2 * slots + F + 1,), dtype=torch.int32, device='cuda')
        assert _pairs_call(case, a, b, pred, work) == 0
        return pred

    whole = links(0, F)
    assert int((whole[:slots] >= 0).sum()) > 0 and int((whole[slots:] >= 0).sum()) > 0
    cnt = dev(np.asarray(case.counts, np.int32))
    for k in range(F + 1):
        both = torch.maximum(links(0, k), links(k, F))
        assert torch.equal(both, whole), f'{name}: split at {k}'
        work = torch.empty((2 * slots,), dtype=torch.int32, device='cuda')
        track = torch.empty((F, cap), dtype=torch.int32, device='cuda')
        n = torch.empty((1,), dtype=torch.int32, device='cuda')
        assert lib.axt_chain_tracks(cnt.data_ptr(), F, cap, both.data_ptr(), work.data_ptr(), track.data_ptr(), n.data_ptr(),
                                    hp._stream()) == 0
        torch.cuda.synchronize()
        _judge(case, track.cpu().numpy(), int(n.item()))


# (frames, slots per frame): frame counts on both sides of the powers of four, slot counts at 8192 (one workgroup) and 8193
# (several launches), around one 16 384-slot batch of the ranking and at several batches, most of them no multiple of 1024
CHAIN_SHAPES = [(1, 8192), (1, 8193), (1, 16383), (1, 40000), (2, 4096), (2, 4097), (4, 2048), (4, 10000), (5, 1639), (5, 3277),
                (16, 512), (16, 513), (16, 1024), (17, 482), (17, 963), (17, 964), (64, 128), (64, 625), (65, 127), (65, 615),
                (257, 31), (257, 32), (257, 63), (257, 64), (257, 156)]


@pytest.mark.parametrize('kind', ['spanning', 'single', 'roots', 'holes'])
@pytest.mark.parametrize('F,cap', CHAIN_SHAPES)
def test_chain_numbering_alone(F, cap, kind):
    """axt_chain_tracks on hand-made links, no solver: chains through every frame with gaps alternating 1 and 2, one single
    chain, roots only, empty frames; track table and track count equal the CPU walk's exactly."""
    count, pred1, pred2 = hr.chain_scene(F, cap, kind, seed=F + cap)
    want, n_want = hr.chain_walk(count, cap, pred1, pred2)
    slots = F * cap
    pred = dev(np.concatenate([pred1.reshape(-1), pred2.reshape(-1)]))
    work = torch.empty((2 * slots,), dtype=torch.int32, device='cuda')
    track = torch.full((F, cap), -7, dtype=torch.int32, device='cuda')
    n = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    d_count = dev(count)
    assert _lib.load().axt_chain_tracks(d_count.data_ptr(), F, cap, pred.data_ptr(), work.data_ptr(), track.data_ptr(),
                                        n.data_ptr(), hp._stream()) == 0
    torch.cuda.synchronize()
    assert int(n.item()) == n_want
    got = track.cpu().numpy()
    assert np.array_equal(got, want), f'first difference at slot {np.argwhere(got != want)[0]}'
