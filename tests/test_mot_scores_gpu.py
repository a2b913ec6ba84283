"""The device tracking scorer (axt_mot_scores) against the CPU reference of tests/mot_reference.py --
counts, tallies and the event log, exactly, on the named cases and on the limit cases (every stated limit, both sides of
every route threshold) -- and AxonDetections.get_tracking_metrics / score_associations /
search_MCF_params(scoring='gpu') against axtrack_amd.mot_metrics on the tie-free scenes."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from axtrack_amd import hotpath as hp, mot_metrics as mm, params
import mot_reference as mr
from helpers import golden_dets
from mot_reference import assert_scores_equal

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(s, ks=None, events=True):
    tr = s['tracks'] if ks is None else s['tracks'][ks]
    out = hp.mot_scores(dev(tr), dev(s['x']), dev(s['y']), dev(s['count']), dev(s['gid']), dev(s['gx']), dev(s['gy']),
                        dev(s['gcount']), s['no'], s['nh'], s['max_dist'], events=events)
    return [o.cpu().numpy() for o in out]


def log_sets(kind, part, fp, k):
    f, i = np.nonzero(kind[k])
    ev = set(zip(f.tolist(), kind[k][f, i].tolist(), i.tolist(), part[k][f, i].tolist()))
    return ev, set(zip(*(v.tolist() for v in np.nonzero(fp[k]))))


@pytest.mark.parametrize('name', list(mr.named_cases()))
def test_named_case_equals_the_reference_exactly(name):
    s = mr.named_cases()[name]
    counts, tallies, kind, part, fp = run(s)
    assert counts.dtype == np.int64 and tallies.dtype == np.int32 and kind.dtype == np.uint8 and part.dtype == np.int32
    for k in range(s['tracks'].shape[0]):
        ref = mr.reference(s, k)
        assert counts[k].tolist() == ref['counts'].tolist(), (name, k, mm.MOT_COUNTS)
        assert tallies[k].tolist() == ref['tallies'].tolist()
        ev, fps = log_sets(kind, part, fp, k)
        assert ev == ref['events']
        assert fps == ref['fp']
        assert (part[k][kind[k] == 0] == -1).all() and (part[k][kind[k] == 3] == -1).all()


def test_a_batch_equals_single_calls_and_two_calls_give_identical_bits():
    s = mr.named_cases()['identities_65_k3']
    batch = run(s)
    again = run(s)
    for a, b in zip(batch, again):
        assert a.tobytes() == b.tobytes()
    for k in range(3):
        for a, b in zip(batch, run(s, [k])):
            assert a[k].tobytes() == b[0].tobytes()
    counts, tallies = run(s, events=False)                        # the log is optional
    assert counts.tobytes() == batch[0].tobytes() and tallies.tobytes() == batch[1].tobytes()


def test_tie_free_battery_equals_mot_metrics():
    for s, k in mr.tie_free_battery():
        counts, tallies = run(s, [k], events=False)
        assert_scores_equal(mm.scores_from_counts(counts[0], tallies[0]), mm.summarize(mr.host_events(s, k)[0]))


# ------------------------------------------------------------------ the limits and both sides of every route threshold
def assert_equals_the_reference(s, out, ks, ref_of, name):
    """Counts, tallies, event log and FP slots of the associations ks (rows 0.. of out) against the reference, exactly. A
    log that differs is first read as a matching: its cardinality and integer cost against the reference's optimum."""
    counts, tallies, kind, part, fp = out
    for row, k in enumerate(ks):
        ref = ref_of(k)
        ev, fps = log_sets(kind, part, fp, row)
        assert ev == ref['events'], (name, mr.explain_mismatch(s, k, ref, ev))
        assert fps == ref['fp'], (name, k)
        assert counts[row].tolist() == ref['counts'].tolist(), (name, k, mm.MOT_COUNTS)
        assert tallies[row].tolist() == ref['tallies'].tolist(), (name, k)
        assert (part[row][kind[row] == 0] == -1).all() and (part[row][kind[row] == 3] == -1).all()


@functools.lru_cache(maxsize=None)
def first_run(name):
    """One call per limit case, shared by the tests below and left unchanged by them."""
    return run(mr.limit_cases()[name].scene)


@pytest.mark.parametrize('name', list(mr.limit_cases()))
def test_limit_case_equals_the_reference_exactly(name):
    """Every call returns AXT_OK (hp.mot_scores raises otherwise): the launches with 65 504 and 65 688 bytes of dynamic
    LDS, with 94 208, and the identity matching with exactly 65 536 bytes and no attribute set."""
    s = mr.limit_cases()[name].scene
    K = s['tracks'].shape[0]
    assert_equals_the_reference(s, first_run(name), range(K), lambda k: mr.limit_reference(name, k), name)


@pytest.mark.parametrize('name', list(mr.limit_cases()))
def test_limit_case_twice_gives_the_same_bytes(name):
    for a, b in zip(first_run(name), run(mr.limit_cases()[name].scene)):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', ['many_associations', 'lds_edge_713'])
def test_a_batch_of_k_gives_the_bytes_of_k_single_calls(name):
    s = mr.limit_cases()[name].scene
    batch = first_run(name)
    for k in range(s['tracks'].shape[0]):
        for a, b in zip(batch, run(s, [k])):
            assert a[k].tobytes() == b[0].tobytes(), (name, k)


def test_without_the_event_log_the_counts_are_the_same_at_1024_x_1024():
    name = 'dense_1024x1024_md255'
    counts, tallies = run(mr.limit_cases()[name].scene, events=False)
    assert counts.tobytes() == first_run(name)[0].tobytes() and tallies.tobytes() == first_run(name)[1].tobytes()


# ------------------------------------------------------------------ AxonDetections
def _detections_object(dets, tmp_path, H=1024, W=1024):
    import axtrack_amd
    from axtrack_amd.detections import AxonDetections
    tl = axtrack_amd.Timelapse(np.zeros((len(dets) + 4, H, W), np.float32), name='synth')
    ad = AxonDetections(None, tl, params.load_parameters(), str(tmp_path))
    ad._set_detections_from_tables([pd.DataFrame({'conf': c, 'anchor_x': x, 'anchor_y': y}) for c, x, y in dets])
    return ad


@pytest.fixture()
def labelled(golden, tmp_path):
    """golden('detect_1024') with the association under the deployed parameters as labels (as
    test_mcf_parameter_search_rows_match_the_oracle sets it up)."""
    dets = golden_dets(golden('detect_1024'))
    ad = _detections_object(dets, tmp_path)
    ad.assign_ids()
    frame, tid, _, x, y = ad.ided_arrays()
    ad.set_groundtruth([(x[frame == t], y[frame == t], tid[frame == t]) for t in range(len(dets))])
    return ad


def _host_scores(ad):
    target = ad.get_frame_dets('groundtruth', None, libmot=True)
    pred = ad.get_frame_dets('IDed', None, libmot=True) if ad._solved else None
    return mm.summarize(mm.compare_to_groundtruth(target, pred, float(ad.nms_min_dist) ** 2))


def test_get_tracking_metrics_and_score_associations_equal_the_host_scores(labelled):
    ad = labelled
    tables = []
    for ec, ccm in ((ad.P['MCF_EDGE_COST_THR'], ad.P['MCF_CONF_CAPPING_METHOD']), (0.4, 'ceil'), (0.4, 'scale_to_max')):
        ad.P.update(MCF_EDGE_COST_THR=ec, MCF_CONF_CAPPING_METHOD=ccm)
        ad.assign_ids()
        want = _host_scores(ad)
        got, log = ad.get_tracking_metrics(events=True)
        assert_scores_equal(got, want)
        assert_scores_equal(ad.get_tracking_metrics(), want)
        F, cap = ad.d_x.shape
        assert log['kind'].shape == log['partner'].shape == (F, ad._gt_dev[0].shape[1]) and log['fp'].shape == (F, cap)
        assert (log['kind'] == 3).sum() == want.num_misses and log['fp'].sum() == want.num_false_positives
        tables.append((ad._track_dev().clone(), want))
    tables.append((torch.full_like(tables[0][0], -1), None))                 # nothing solved: the host path's pred = None
    res = ad.score_associations(torch.stack([t for t, _ in tables]))
    assert list(res.columns) == mm.MOTCHALLENGE_METRICS and len(res) == 4
    for (_, want), (_, row) in zip(tables[:3], res.iterrows()):
        assert_scores_equal(row, want)
    target = ad.get_frame_dets('groundtruth', None, libmot=True)
    assert_scores_equal(res.iloc[3], mm.summarize(mm.compare_to_groundtruth(target, None, 23.0 ** 2)))
    assert res.iloc[0].mota == 1 and res.iloc[0].idf1 == 1


def test_parameter_search_scored_on_the_device_equals_the_host_search(labelled, tmp_path):
    ad, P = labelled, params.load_parameters()
    grid = dict(edge_cost_thr_values=[0.4, P['MCF_EDGE_COST_THR']], entry_exit_cost_values=[0.9, P['MCF_ENTRY_EXIT_COST']],
                miss_rate_values=[P['MCF_MISS_RATE']], vis_sim_weight_values=[0], conf_capping_method_values=['ceil', 'scale_to_max'])
    host = ad.search_MCF_params(**grid)
    host_csv = (tmp_path / 'MCF_params_results.csv').read_bytes()
    assert ad.P == P
    got = ad.search_MCF_params(**grid, scoring='gpu', score_batch=3)          # 8 rows: batches of 3, 3 and 2
    assert ad.P == P
    pd.testing.assert_frame_equal(got, host, check_exact=True)
    assert (tmp_path / 'MCF_params_results.csv').read_bytes() == host_csv
    assert len(got) == 8 and 1 <= int((got.mota == 1).sum()) < 8
    with pytest.raises(ValueError):
        ad.search_MCF_params(**grid, scoring='device')


def test_errors(labelled, golden, tmp_path):
    dets = golden_dets(golden('detect_1024'))
    bare = _detections_object(dets, tmp_path)
    bare.assign_ids()
    with pytest.raises(ValueError, match='no labels'):
        bare.get_tracking_metrics()
    with pytest.raises(ValueError, match='no labels'):
        bare.score_associations(bare._track_dev()[None])
    ad = labelled
    ad._drop_association()
    with pytest.raises(AssertionError):
        ad.get_tracking_metrics()
    with pytest.raises(ValueError, match='shape'):
        ad.score_associations(torch.zeros((1, 2, 3), dtype=torch.int32, device='cuda'))
    ad._shard = object()
    with pytest.raises(NotImplementedError):
        ad.score_associations(torch.full_like(ad.d_x, -1)[None])
    ad._shard = None
    many = np.arange(1025)
    ad.set_groundtruth([(many, many, many)] + [(many[:1], many[:1], many[:1])] * (len(dets) - 1))
    with pytest.raises(ValueError, match='1025 labels'):
        ad.score_associations(torch.full_like(ad.d_x, -1)[None])
    # and the library itself refuses the shape
    with pytest.raises(Exception, match='gcap 1025'):
        hp.mot_scores_scratch_bytes(1, 4, 8, 1025, 3, 5)
