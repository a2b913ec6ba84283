"""The cached state of AxonDetections on the GPU: an object that is given new detections, or associated again under other
parameters, answers exactly like a fresh one. The expected value is always a fresh object's, never a stored number.

The scene: 6 detection frames of 160 x 192 noise (so every detection has its own appearance histogram), capacity 64, and two
seeded detection sets A and B of the same array shapes -- 3 to 6 detections per frame in descending confidence, each within
7 px of one of six anchors (three either side of x = 96; consecutive frames differ by at most 12 moves), every 70 px
appearance box inside the frame."""
import numpy as np
import pytest

from axtrack_amd import params

pytestmark = pytest.mark.gpu

H, W, F, CAP = 160, 192, 6, 64
TARGET = (80, 60)


def _wall_mask(gap=(74, 86)):
    """All ones but a vertical wall at x = 94..98 with one 12 px gap."""
    m = np.ones((H, W), bool)
    m[:, 94:99] = False
    m[gap[0]:gap[1], 94:99] = True
    return m


def _scene(seed):
    rng = np.random.default_rng(seed)
    spots = np.array([(x, y) for x in (52, 78, 114, 140) for y in (50, 80, 110)])          # six either side of the wall
    base = spots[np.r_[rng.permutation(6)[:3], 6 + rng.permutation(6)[:3]]] + rng.integers(-4, 5, (6, 2))
    conf, x, y = np.zeros((F, CAP), np.float32), np.zeros((F, CAP), np.int32), np.zeros((F, CAP), np.int32)
    count = np.zeros(F, np.int32)
    for f in range(F):
        n = count[f] = int(rng.integers(3, 7))
        pos = base[rng.permutation(6)[:n]] + rng.integers(-3, 4, (n, 2))
        conf[f, :n] = np.sort(rng.uniform(0.6, 0.99, n).astype(np.float32))[::-1]
        x[f, :n], y[f, :n] = pos[:, 0], pos[:, 1]
    assert x[x > 0].min() >= 40 and x.max() <= W - 40 and y[y > 0].min() >= 40 and y.max() <= H - 40
    return conf, x, y, count


A, B = _scene(1), _scene(2)


def test_the_two_scenes_differ_in_anchors_and_not_in_shape():
    assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(A, B))
    assert not np.array_equal(A[1], B[1]) and not np.array_equal(A[2], B[2])
    for s in (A, B):
        assert s[3].min() >= 3 and s[3].max() <= 6
        assert (s[1][s[0] > 0] < 94).any() and (s[1][s[0] > 0] > 98).any()                  # anchors on both sides of the wall


def _ad(assoc='mcf', vis=0, mask=None, **more):
    import torch
    import axtrack_amd
    frames = torch.rand((F + 4, H, W), generator=torch.Generator().manual_seed(7)) * 0.98 + 0.01
    tl = axtrack_amd.Timelapse(frames, name='state', mask=mask, device=torch.device('cuda', 0))
    P = dict(params.load_parameters(), ASSOCIATION=assoc, MCF_VIS_SIM_WEIGHT=vis, MCF_MIN_FLOW=1, MCF_MAX_FLOW=100000, **more)
    return axtrack_amd.AxonDetections(None, tl, P, None)


def _same_arrays(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def _assert_answers_like(ad, fresh):
    assert _same_arrays(ad.ided_arrays(), fresh.ided_arrays())
    assert ad.IDed_dets_all.equals(fresh.IDed_dets_all)
    assert ad.n_ids == fresh.n_ids and ad.n_ids > 0
    assert ad.mcf_total_cost == fresh.mcf_total_cost
    assert ad.get_target_distances().equals(fresh.get_target_distances())
    got, want = ad.get_trg_path(2), fresh.get_trg_path(2)
    assert list(got) == list(want) and len(want) > 0
    assert all(_same_arrays(got[k], want[k]) for k in want)
    got, want = ad.reconstruction_arrays(), fresh.reconstruction_arrays()
    assert list(got) == list(want) and len(want['len']) > 0
    assert all(np.array_equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize('masked', [False, True], ids=['open', 'wall'])
@pytest.mark.parametrize('vis', [0, 0.1])
@pytest.mark.parametrize('assoc', ['mcf', 'hungarian'])
def test_reused_object_equals_a_fresh_one(assoc, vis, masked):
    mask = _wall_mask() if masked else None
    ad = _ad(assoc, vis, mask)
    ad.set_detections(*A)
    ad.assign_ids()
    ad.set_target(TARGET)
    ad.get_target_distances(), ad.reconstruction_arrays(), ad.get_trg_path(2)
    ad.set_detections(*B)
    ad.assign_ids()
    fresh = _ad(assoc, vis, mask)
    fresh.set_detections(*B)
    fresh.assign_ids()
    fresh.set_target(TARGET)
    assert (fresh.mcf_total_cost is not None) == (assoc == 'mcf')
    _assert_answers_like(ad, fresh)


def test_association_variant_switch_drops_the_certificate():
    from helpers import check_flow_certificate
    ad = _ad('mcf', MCF_CERTIFICATE=True)
    ad.set_detections(*B)
    ad.assign_ids()
    cert = ad.mcf_certificate
    assert not cert['entry'].flags.writeable and not cert['exit'].flags.writeable
    proof = check_flow_certificate(cert['obs'], cert['entry'], cert['exit'], cert['row_ptr'], cert['col'], cert['cost'], cert['next'],
                                   cert['track'], cert['total_cost'], cert['potentials'], cert['min_flow'], cert['max_flow'])
    assert proof['trajectories'] == ad.n_ids > 0 and ad.mcf_total_cost == cert['total_cost']
    ad.P['ASSOCIATION'] = 'hungarian'
    ad.assign_ids()
    assert ad.mcf_certificate is None and ad.mcf_total_cost is None and ad.n_ids > 0


def test_search_reuses_the_appearance_histograms():
    ad = _ad('mcf', 0.1)
    ad.set_detections(*A)
    ad.assign_ids()
    hist = ad._hist
    assert hist is not None
    ad.assign_ids()
    assert ad._hist is hist                                           # the detections have not changed: not recomputed
    ad.set_detections(*B)
    assert ad._hist is None
    ad.assign_ids()
    assert ad._hist is not None and ad._hist is not hist


def test_time_varying_mask_arcs_through_one_chooser():
    m3 = np.stack([_wall_mask() if k < 5 else _wall_mask((30, 42)) for k in range(F + 4)])
    ad = _ad('mcf', mask=m3)
    assert ad.dataset.mask3d is not None and len(ad._mask_grids()[0]) == 2
    ad.set_detections(*B)
    for assoc in ('mcf', 'hungarian', 'mcf'):
        ad.P['ASSOCIATION'] = assoc
        ad.assign_ids()
        fresh = _ad(assoc, mask=m3)
        fresh.set_detections(*B)
        fresh.assign_ids()
        assert _same_arrays(ad.ided_arrays(), fresh.ided_arrays()) and ad.n_ids == fresh.n_ids > 0
        assert ad.mcf_total_cost == fresh.mcf_total_cost and ad.IDed_dets_all.equals(fresh.IDed_dets_all)
