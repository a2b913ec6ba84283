"""The search step of the Hungarian pair kernels and the chain numbering (axtrack_amd/csrc/hungarian.hip) on the cases of
tests/hungarian_step_cases.py: keys that differ in one half of the packed word only, equal keys in different lanes, rows of lanes and register slots, the largest key, no candidate at all, a
column level with the dummy; frame counts on both sides of the 64-column slots and of the cost cache, gap-2 pairs with
rows and columns taken, empty frames; chains of gap-2 links alone and across an empty frame, at slot counts on both sides
of the bound between the two chain numberings and frame counts on both sides of the powers of four.
tests/test_hungarian_step_cpu.py proves on the CPU that each case is what its name says. Every pair case is judged by
hungarian_reference.judge against SciPy (the tied ones with the trajectories of the kernel's own tie rules), except the two
whose costs exceed the judge's exact f64 sums, which an enumeration in Python integers decides."""
import numpy as np
import pytest
import torch

import hungarian_reference as hr
import hungarian_step_cases as sc
from axtrack_amd import _lib, hotpath as hp

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _run(case):
    F, cap = len(case.counts), case.cap
    z = torch.zeros((F, cap), dtype=torch.int32, device='cuda')
    ctab = dev(hr.costs_to_table(case.costs, case.counts, cap, gaps=case.max_gap))
    track, n = hp.hungarian_assoc(z, z, dev(np.asarray(case.counts, np.int32)), 1, 1, [0] * case.max_gap,
                                  np.zeros((case.max_gap, 2), np.int64), case.thr_units, ctab=ctab)
    torch.cuda.synchronize()
    return track.cpu().numpy(), int(n.item())


@pytest.mark.parametrize('case', sc.pair_cases(), ids=repr)
def test_search_step(case):
    track, n = _run(case)
    if case.exact == 'enumeration':
        dummy = hr.dummy_costs(case.counts, case.thr_units)[0]
        _, (pick,) = sc.enumerated_optimum(case.costs[(0, 1)], dummy)
        linked = {j for j in pick if j >= 0}
        trajs = [[(0, i)] + ([(1, j)] if j >= 0 else []) for i, j in enumerate(pick)]
        trajs += [[(1, j)] for j in range(case.counts[1]) if j not in linked]
        assert n == len(trajs)
        assert np.array_equal(track, hr.track_table(trajs, case.counts, case.cap))
        return
    ref = sc.model_reference(case.costs, case.counts, case.thr_units, case.max_gap) if case.ties else case.reference
    hr.judge(case.costs, case.counts, track, n, name=case.name, thr_units=case.thr_units, max_gap=case.max_gap, ref=ref)


@pytest.mark.parametrize('kind', sc.CHAIN_KINDS)
@pytest.mark.parametrize('F,cap', sc.chain_shapes())
def test_chain_numbering(F, cap, kind):
    """axt_chain_tracks on hand-made links: track table and track count equal hungarian_reference.chain_walk's."""
    count, pred1, pred2 = sc.chain_scene(F, cap, kind, seed=F + cap)
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
    assert np.array_equal(got, want), f'{sc.chain_route(slots)}: first difference at slot {np.argwhere(got != want)[0]}'
