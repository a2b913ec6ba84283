"""Parity of the HIP hot path (through the C ABI) against the golden vectors captured from the
reference and against the CPU oracle. Run on the MI355X box: pytest -m gpu."""
import os

import numpy as np
import pytest
import torch

from axtrack_amd import synth, params
from axtrack_amd import hotpath as hp
from oracle import oracle as orc
from helpers import golden_dets, csr_arcs_from_oracle, tracks_from_next

pytestmark = pytest.mark.gpu

# f32 CNN: the reference (oneDNN), the oracle (direct loops) and the MFMA kernels sum in different
# orders; outputs are O(1) and agree to a few 1e-6. Tolerance stated for the whole detector:
# the kernels deliver 4e-7 ... 1.5e-6 against the reference golden and the oracle (every arithmetic variant): the bound is 10x that,
# tight enough that a kernel change which costs accuracy -- and starts flipping cells at the 0.55 floor -- fails here
CNN_ATOL, CNN_RTOL = 1e-5, 1e-5


@pytest.fixture(scope='module')
def detector(weights):
    import axtrack_amd
    return axtrack_amd.Detector(weights, max_batch=24)


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


# ----------------------------------------------------------------------------------------- a-1 / a-2
def test_cnn_forward_matches_reference_golden(golden, detector):
    g = golden('cnn_512')
    frames = synth.synth_frames(int(g['T_all']), 512, 512, seed=int(g['frames_seed']))
    y = detector.detect_frames(dev(frames), [(0, 0)]).cpu().numpy()
    assert y.shape == (5, 1, 12, 12, 3)
    np.testing.assert_allclose(y[:, 0], g['yolo'], atol=CNN_ATOL, rtol=CNN_RTOL)
    err = np.abs(y[:, 0] - g['yolo']).max()
    assert err < 5e-5, f'unexpectedly large deviation from the reference: {err}'


def test_detect_axons_tensor_interface_equals_frames_path(golden, detector):
    """detect_axons(X[B,5,512,512]) (model.py:119-125) and the fused frames path are the same kernels."""
    g = golden('cnn_512')
    frames = synth.synth_frames(9, 512, 512, seed=0)
    X = np.stack([frames[t:t + 5] for t in range(5)])
    y1 = detector.detect_axons(dev(X)).cpu().numpy()
    y2 = detector.detect_frames(dev(frames), [(0, 0)]).cpu().numpy()[:, 0]
    assert np.array_equal(y1, y2)
    np.testing.assert_allclose(y1, g['yolo'], atol=CNN_ATOL, rtol=CNN_RTOL)
    with pytest.raises(ValueError):
        detector.detect_axons(torch.zeros(1, 5, 256, 256))


def test_cnn_conv_stack_against_oracle_on_edge_inputs(detector, weights):
    """Zero input, constant input and a single hot pixel in every corner: exercises the zero padding
    of every layer and the folded-BN bias path."""
    X = np.zeros((4, 5, 512, 512), np.float32)
    X[1] = 1.0
    for c, (yy, xx) in enumerate([(0, 0), (0, 511), (511, 0), (511, 511), (255, 256)]):
        X[2, c, yy, xx] = 50.0
    X[3] = synth.synth_frames(5, 512, 512, seed=9) * 3
    y = detector.detect_axons(dev(X)).cpu().numpy()
    ref = orc.cnn_forward(weights, X)
    np.testing.assert_allclose(y, ref, atol=CNN_ATOL, rtol=CNN_RTOL)


def test_ragged_frame_with_dropped_tile(golden, detector):
    g = golden('detect_ragged')
    frames = synth.synth_frames(int(g['T_all']), int(g['H']), int(g['W']), seed=int(g['frames_seed']))
    zt = g['zero_tile']
    frames[:, zt[0] * 512:(zt[0] + 1) * 512, zt[1] * 512:(zt[1] + 1) * 512] = 0
    fr = dev(frames)
    keep = hp.tile_occupancy(fr)
    assert keep == [tuple(ix) for ix in np.argwhere(g['kept_tiles'])]
    y = detector.detect_frames(fr, keep).cpu().numpy()
    np.testing.assert_allclose(y, g['yolo'], atol=CNN_ATOL, rtol=CNN_RTOL)


# ----------------------------------------------------------------------------------------- a-3 .. a-6
@pytest.mark.parametrize('name', ['detect_1024', 'detect_ragged', 'detect_crafted'])
def test_decode_stitch_nms_bit_exact_on_reference_grids(golden, name):
    g = golden(name)
    keep = [(0, 0), (0, 1), (1, 0), (1, 1)] if name == 'detect_crafted' else [tuple(ix) for ix in np.argwhere(g['kept_tiles'])]
    conf, x, y, cnt = [t.cpu().numpy() for t in hp.decode_stitch_nms(dev(g['yolo']), keep)]
    ref = golden_dets(g)
    for t, (rc, rx, ry) in enumerate(ref):
        if name == 'detect_crafted' and t == 1:
            # exact confidence ties: the reference's order comes from pandas' unstable quicksort; ours is
            # defined as (tile, cell) order and must equal the oracle's
            oc, ox, oy = orc.nms(*orc.stitch(orc.decode_filter(g['yolo'][1]), keep))
            rc, rx, ry = oc, ox, oy
        n = int(cnt[t])
        assert n == len(rc), f'frame {t}'
        assert np.array_equal(conf[t, :n].view(np.uint32), rc.view(np.uint32)), f'frame {t}'
        assert np.array_equal(x[t, :n], rx) and np.array_equal(y[t, :n], ry), f'frame {t}'


def test_nms_empty_and_full_frames():
    yolo = np.zeros((3, 2, 12, 12, 3), np.float32)              # frame 0: nothing passes
    yolo[1, ..., 0] = 0.9                                        # frame 1: all cells, all at the cell origin
    yolo[2, ..., 0] = 0.9
    yolo[2, ..., 1:] = 0.5                                       # frame 2: cell centres, 42.7 px apart: all survive
    keep = [(0, 0), (0, 1)]
    conf, x, y, cnt = [t.cpu().numpy() for t in hp.decode_stitch_nms(dev(yolo), keep)]
    ref = orc.detect_from_yolo(list(yolo), keep)
    assert cnt[0] == 0 and cnt[2] == 288
    for t in range(3):
        n = int(cnt[t])
        assert n == len(ref[t][0])
        assert np.array_equal(x[t, :n], ref[t][1]) and np.array_equal(y[t, :n], ref[t][2])
    with pytest.raises(Exception):
        hp.decode_stitch_nms(dev(yolo), keep, cap=100)           # capacity below n_tiles*144


def test_nms_adversarial_chain():
    """A chain of detections, each within 23 px of the next, descending confidence: alternate ones
    survive; the parallel rounds must reproduce the sequential greedy result."""
    yolo = np.zeros((1, 1, 12, 12, 3), np.float32)
    k = 0
    for i in range(12):
        for j in range(12):
            # place along a snake with ~15 px spacing by abusing the in-cell offsets
            px, py = 10 + 15 * (k % 30), 10 + 15 * (k // 30)
            yolo[0, 0, i, j] = (2.0 - 0.01 * k, px * 12 / 512 - i, py * 12 / 512 - j)
            k += 1
    conf, x, y, cnt = [t.cpu().numpy() for t in hp.decode_stitch_nms(dev(yolo), [(0, 0)])]
    rc, rx, ry = orc.detect_from_yolo([yolo[0]], [(0, 0)])[0]
    n = int(cnt[0])
    assert n == len(rc) and np.array_equal(x[0, :n], rx) and np.array_equal(y[0, :n], ry)


# ----------------------------------------------------------------------------------------- a-8 / a-10
def test_observation_costs(golden):
    g, a = golden('detect_1024'), golden('assoc_parts')
    dets = golden_dets(g)
    F, cap = len(dets), 576
    conf = np.zeros((F, cap), np.float32)
    for t, d in enumerate(dets):
        conf[t, :len(d[0])] = d[0]
    cnt = np.array([len(d[0]) for d in dets], np.int32)
    cost = hp.obs_costs(dev(conf), dev(cnt), 'scale_to_max', 4.6).cpu().numpy()
    flat = np.concatenate([cost[t, :cnt[t]] for t in range(F)])
    # f64 log on the GPU is accurate to 1 ulp, not correctly rounded: tolerance 1e-12, and the
    # integer cost units (round(cost*1e6)) must be identical
    np.testing.assert_allclose(flat, a['obs_cost'], rtol=0, atol=1e-12)
    assert np.array_equal(np.rint(flat * 1e6), np.rint(a['obs_cost'] * 1e6))
    ceil = hp.obs_costs(dev(conf), dev(cnt), 'ceil', 4.6).cpu().numpy()
    ref = orc.observation_cost(a['conf_ceil'])
    np.testing.assert_allclose(np.concatenate([ceil[t, :cnt[t]] for t in range(F)]), ref, rtol=0, atol=1e-12)


# ----------------------------------------------------------------------------------------- a-9 / a-11
def test_path_cost_open_grid_matches_oracle(golden):
    g = golden('detect_1024')
    dets = golden_dets(g)
    (c0, x0, y0), (c1, x1, y1) = dets[0], dets[1]
    x0 = x0.copy(); x0[0] = -3                                    # an anchor outside the grid (decode does not clamp)
    for conn8 in (False, True):
        D = hp.path_cost(dev(x0, torch.int32), dev(y0, torch.int32), dev(x1, torch.int32), dev(y1, torch.int32),
                         1024, 1024, None, 500, conn8).cpu().numpy()
        ref = orc.path_matrix((c0, x0, y0), (c1, x1, y1), 1024, 1024, None, 500, conn8)
        assert np.array_equal(D, ref)
    assert (D[0] == 500).all()


def test_build_arcs_matches_oracle_csr(golden):
    g = golden('detect_1024')
    dets = golden_dets(g)
    F, cap = len(dets), 576
    x = np.zeros((F, cap), np.int32); y = np.zeros((F, cap), np.int32)
    for t, d in enumerate(dets):
        x[t, :len(d[1])] = d[1]; y[t, :len(d[2])] = d[2]
    cnt = np.array([len(d[0]) for d in dets], np.int32)
    from axtrack_amd.detections import transition_cost_table
    table, dmax = transition_cost_table(params.DEPLOYED)
    units = np.where(np.isfinite(table), np.rint(table * 1e6), 0).astype(np.int64)
    row_ptr, col, length, gap, cost = hp.build_arcs(dev(x), dev(y), dev(cnt), 1024, 1024, dmax, units)
    r_row, r_col, r_len, r_gap, r_cost, offs = csr_arcs_from_oracle(dets, 1024, 1024)
    n_det = int(offs[-1])
    assert np.array_equal(row_ptr[:n_det + 1].cpu().numpy(), r_row)
    assert np.array_equal(col.cpu().numpy(), r_col)
    assert np.array_equal(length.cpu().numpy(), r_len)
    assert np.array_equal(gap.cpu().numpy(), r_gap)
    assert np.array_equal(cost.cpu().numpy(), r_cost)


# ----------------------------------------------------------------------------------------- whole path
def _run_inference(frames, weights, P, name='synth'):
    import axtrack_amd
    model = axtrack_amd.Detector(weights, max_batch=32)
    tl = axtrack_amd.Timelapse(frames, name=name)
    return axtrack_amd.inference(tl, model, None, P, None, None, None)


def test_inference_end_to_end_against_oracle(weights):
    """1024x1024x12 (8 detection frames, 4 tiles): every stage after the CNN is bit-exact against the
    oracle fed with the same YOLO grids; the CNN itself is within tolerance of the oracle."""
    frames = synth.synth_frames(12, 1024, 1024, seed=11)
    P = params.load_parameters()
    ad = _run_inference(frames, weights, P)
    yolo = ad._yolo.cpu().numpy()
    ref = orc.inference(frames, weights, P=orc.DEFAULTS, yolo=list(yolo))
    cnt, conf, x, y = ad._host_dets()
    for t, (rc, rx, ry) in enumerate(ref['dets']):
        n = int(cnt[t])
        assert n == len(rc)
        assert np.array_equal(conf[t, :n], rc) and np.array_equal(x[t, :n], rx) and np.array_equal(y[t, :n], ry)
    assert ad.mcf_total_cost == ref['total_cost'] and ad.n_ids == len(ref['trajs'])
    got_tracks = tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs)
    assert got_tracks == ref['trajs']
    ids, labels, info, vals = ref['ided_all']
    df = ad.IDed_dets_all
    assert list(df.index) == [f'Axon_{i:0>3}' for i in ids]
    assert [c[0] for c in df.columns] == list(labels.astype(int)) and [c[1] for c in df.columns] == list(info)
    assert np.array_equal(np.nan_to_num(df.to_numpy(), nan=-1), np.nan_to_num(vals, nan=-1))
    # astar_dists API (the reference's cache format) against the oracle's matrices
    dists = ad.astar_dists()
    refD = orc.all_path_matrices(ref['dets'], 1024, 1024)
    assert dists.keys() == refD.keys()
    for k in dists:
        assert np.array_equal(dists[k], refD[k]), k
    # one frame of the CNN against the oracle
    yref = orc.cnn_forward(weights, orc.frame_tile_stack(frames, 3, ad.tile_yx))
    np.testing.assert_allclose(yolo[3], yref, atol=CNN_ATOL, rtol=CNN_RTOL)


def test_ided_dets_all_reproduces_the_references_table(golden, weights):
    """IDed_dets_all built from golden detections + the golden (synthetic) trajectories must equal the
    DataFrame the reference produced, including the empty-frame label quirk (AxonDetections.py:833-839)."""
    import axtrack_amd
    from axtrack_amd.detections import AxonDetections
    g, a = golden('detect_1024'), golden('assoc_parts')
    dets = golden_dets(g)
    tl = axtrack_amd.Timelapse(np.zeros((7, 1024, 1024), np.float32), name='synth')
    ad = AxonDetections(None, tl, params.load_parameters(), None)
    import pandas as pd
    tabs = [pd.DataFrame({'conf': c, 'anchor_x': x, 'anchor_y': y}) for c, x, y in dets]
    ad._set_detections_from_tables(tabs)
    offs = np.concatenate([[0], np.cumsum(g['counts'])])
    track = np.full(int(offs[-1]), -1, np.int32)
    for tid, f, k in a['traj']:
        track[offs[f] + k] = tid
    ad._track_flat_cache, ad._d_track, ad.n_ids = track, None, None     # as adopted from a cache: ids unknown
    df = ad._agg_all_IDed_dets()
    assert list(df.index) == list(a['ided_all_index'])
    assert [float(c[0]) for c in df.columns] == list(a['ided_all_cols_frame'])
    assert [c[1] for c in df.columns] == list(a['ided_all_cols_info'])
    np.testing.assert_array_equal(df.to_numpy(), a['ided_all_values'])
    assert df.index.name == 'axonID' and list(df.columns.names) == ['frameID', 'detInfo']


@pytest.mark.parametrize('T_all,size,name', [(256, 512, 'c3'), (132, 1024, 'c4')])
def test_full_size_properties(weights, T_all, size, name):
    """BASELINE config 3 (512x512x256) and one GPU's share of config 4 (1024x1024, 128 detection frames, global flow
    solve): properties that hold at any size."""
    frames = synth.synth_frames(T_all, size, size, seed=0)
    P = params.load_parameters()
    ad = _run_inference(frames, weights, P, name=name)
    cnt, conf, x, y = ad._host_dets()
    assert len(cnt) == T_all - 4 and cnt.min() > 0
    for t in range(0, T_all - 4, 17):
        n = int(cnt[t])
        assert np.all(np.diff(conf[t, :n].astype(np.float64)) <= 0)                     # sorted
        d2 = (x[t, :n, None] - x[t, None, :n]).astype(np.int64) ** 2 + (y[t, :n, None] - y[t, None, :n]).astype(np.int64) ** 2
        np.fill_diagonal(d2, 10 ** 9)
        assert d2.min() >= 529                                                        # NMS distance
        assert conf[t, :n].min() >= np.float32(0.55)
    # every trajectory visits strictly increasing frames with gaps <= 2 and admissible path lengths
    tracks = tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs)
    assert P['MCF_MIN_FLOW'] <= len(tracks) <= P['MCF_MAX_FLOW'] and len(tracks) == ad.n_ids
    seen = set()
    for tr in tracks:
        for (f0, i0), (f1, i1) in zip(tr[:-1], tr[1:]):
            g = f1 - f0
            assert g in (1, 2)
            D = abs(int(x[f0, i0]) - int(x[f1, i1])) + abs(int(y[f0, i0]) - int(y[f1, i1])) + 1
            assert D <= (251 if g == 1 else 86)
        for node in tr:
            assert node not in seen                                                   # node-disjoint
            seen.add(node)
    # idempotence: a second run gives identical results (bit-reproducible kernels, unique optimum)
    ad2 = _run_inference(frames, weights, P, name=name)
    assert np.array_equal(ad2._track_flat, ad._track_flat) and ad2.mcf_total_cost == ad.mcf_total_cost
    assert torch.equal(ad2._yolo, ad._yolo)
    if name == 'c3':
        # and at this size against the oracle: detection lists of all 252 frames bit-exact given the same YOLO grids, and
        # the frame-to-frame association identical (the flow solve at this size is compared on the CPU:
        # tests/test_host_logic.py::test_flow_solver_fast_and_general_paths_agree_at_full_size)
        ah = _run_inference(frames, weights, dict(P, ASSOCIATION='hungarian'), name=name)
        ref = orc.inference(frames, weights, P=orc.DEFAULTS, yolo=list(ah._yolo.cpu().numpy()), assoc='hungarian')
        for t, (rc, rx, ry) in enumerate(ref['dets']):
            n = len(rc)
            assert cnt[t] == n and np.array_equal(conf[t, :n], rc) and np.array_equal(x[t, :n], rx) and np.array_equal(y[t, :n], ry)
        assert tracks_from_next(np.zeros(len(ah._track_flat)), ah._track_flat, ah._offs) == ref['trajs']


# ----------------------------------------------------------------------------------------- config 3 variant
def _hungarian_tracks(dets, H, W, cap=None):
    from axtrack_amd.detections import transition_cost_table
    F = len(dets)
    cap = cap or max(len(d[0]) for d in dets) + 3
    x = np.zeros((F, cap), np.int32); y = np.zeros((F, cap), np.int32)
    for t, d in enumerate(dets):
        x[t, :len(d[1])] = d[1]; y[t, :len(d[2])] = d[2]
    cnt = np.array([len(d[0]) for d in dets], np.int32)
    table, dmax = transition_cost_table(params.DEPLOYED)
    units = np.where(np.isfinite(table), np.rint(table * 1e6), 0).astype(np.int64)
    track, n_tracks = hp.hungarian_assoc(dev(x), dev(y), dev(cnt), H, W, dmax, units, 700000)
    track = track.cpu().numpy()
    offs = np.concatenate([[0], np.cumsum(cnt)])
    flat = np.concatenate([track[t, :cnt[t]] for t in range(F)])
    assert (track[np.arange(cap)[None, :] >= cnt[:, None]] == -1).all()
    return tracks_from_next(np.zeros(len(flat)), flat, offs), int(n_tracks.item())


def test_hungarian_association_matches_scipy_oracle(golden):
    g = golden('detect_1024')
    dets = golden_dets(g)
    got, n = _hungarian_tracks(dets, 1024, 1024)
    ref = orc.hungarian_assoc(dets, 1024, 1024)
    assert n == len(ref) and got == ref


@pytest.mark.parametrize('seed', range(4))
def test_hungarian_association_random_frames(seed):
    """Crowded random frames with detections appearing/disappearing: contested columns, gap-2 links,
    empty frames."""
    rng = np.random.default_rng(100 + seed)
    F = 7
    dets = []
    for t in range(F):
        n = 0 if (seed == 3 and t == 3) else int(rng.integers(1, 60))
        conf = np.sort(rng.uniform(0.55, 1.2, n).astype(np.float32))[::-1]
        dets.append((conf, rng.integers(-5, 300, n), rng.integers(0, 300, n)))
    got, n = _hungarian_tracks(dets, 300, 300)
    ref = orc.hungarian_assoc(dets, 300, 300)
    assert n == len(ref) and got == ref


def test_hungarian_association_wide_and_long():
    """cap = 576 (four tiles) and 720 x 130 frames: more than 192 detection slots per frame (search state in nine
    registers per lane, or in LDS beyond 576 slots) and more than 8 k slots (chain numbering by multi-launch pointer doubling instead of one workgroup)."""
    rng = np.random.default_rng(77)
    dets = []
    for t in range(130):
        n = int(rng.integers(0, 14)) if t % 17 else 230          # mostly sparse, a few crowded frames (> 192)
        conf = np.sort(rng.uniform(0.55, 1.2, n).astype(np.float32))[::-1]
        dets.append((conf, rng.integers(0, 1024, n), rng.integers(0, 1024, n)))
    ref = orc.hungarian_assoc(dets, 1024, 1024)
    for cap in (576, 720):                   # 9 register slots per lane / column state in LDS
        got, n = _hungarian_tracks(dets, 1024, 1024, cap=cap)
        assert n == len(ref) and got == ref, cap


def test_inference_hungarian_mode_end_to_end(weights):
    frames = synth.synth_frames(10, 512, 512, seed=21)
    P = params.load_parameters()
    P['ASSOCIATION'] = 'hungarian'
    ad = _run_inference(frames, weights, P)
    yolo = ad._yolo.cpu().numpy()
    ref = orc.inference(frames, weights, P=orc.DEFAULTS, yolo=list(yolo), assoc='hungarian')
    got = tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs)
    assert got == ref['trajs'] and ad.n_ids == len(ref['trajs'])
    ids, labels, info, vals = ref['ided_all']
    df = ad.IDed_dets_all
    assert list(df.index) == [f'Axon_{i:0>3}' for i in ids]
    assert np.array_equal(np.nan_to_num(df.to_numpy(), nan=-1), np.nan_to_num(vals, nan=-1))
    # per-frame IDed tables (built lazily) carry the same rows
    tabs = ad._IDed_detections
    for f, rows in enumerate(ref['tables']):
        assert [int(n[-3:]) for n in tabs[f].index] == [r[0] for r in rows]
        assert list(tabs[f].anchor_x) == [r[2] for r in rows]


def test_inference_hungarian_mode_with_the_appearance_term(weights):
    """ASSOCIATION='hungarian' with MCF_VIS_SIM_WEIGHT > 0 (d_ctab of axt_hungarian_pairs): the link costs are the flow
    tracker's arc costs with the appearance term (axt_build_arcs with d_hist), handed to the pair kernels as a table. Same
    trajectories and IDed_dets_all as the oracle (SciPy LSAP on transition_cost(..., vis_w, vis_sim)), on the all-ones mask
    and on a masked grid; and a different association from the one without the term."""
    import axtrack_amd
    frames = synth.synth_frames(9, 512, 512, seed=33) * np.float32(0.5)
    model = axtrack_amd.Detector(weights, max_batch=8)
    for mask in (None, synth.corridor_mask(512, 512, width=60, pitch=160)):
        P = dict(params.load_parameters(), ASSOCIATION='hungarian', MCF_VIS_SIM_WEIGHT=0.3)
        tl = axtrack_amd.Timelapse(frames, name='synth', mask=mask)
        ad = axtrack_amd.inference(tl, model, None, P, None, None, None)
        yolo = list(ad._yolo.cpu().numpy())
        ref = orc.inference(frames, weights, mask=mask, P=dict(orc.DEFAULTS, MCF_VIS_SIM_WEIGHT=0.3), yolo=yolo, assoc='hungarian')
        got = tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs)
        assert got == ref['trajs'] and ad.n_ids == len(ref['trajs'])
        assert np.array_equal(np.nan_to_num(ad.IDed_dets_all.to_numpy(), nan=-1), np.nan_to_num(ref['ided_all'][3], nan=-1))
        ref0 = orc.inference(frames, weights, mask=mask, P=orc.DEFAULTS, yolo=yolo, assoc='hungarian')
        assert ref0['trajs'] != ref['trajs']


def test_inference_hungarian_mode_on_a_masked_grid(weights):
    """The frame-to-frame variant with path lengths from the masked-grid searches (axt_hungarian_pairs with a grid): the
    oracle's trajectories, which differ from those on the all-ones mask."""
    import axtrack_amd
    frames = synth.synth_frames(9, 512, 512, seed=27)
    mask = synth.corridor_mask(512, 512, width=40, pitch=128)
    P = dict(params.load_parameters(), ASSOCIATION='hungarian')
    model = axtrack_amd.Detector(weights, max_batch=8)
    ad = axtrack_amd.inference(axtrack_amd.Timelapse(frames, name='synth', mask=mask), model, None, P, None, None, None)
    ref = orc.inference(frames, weights, mask=mask, P=orc.DEFAULTS, yolo=list(ad._yolo.cpu().numpy()), assoc='hungarian')
    got = tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs)
    assert got == ref['trajs'] and ad.n_ids == len(ref['trajs'])
    # scattered detections on a mask with walls, gaps and an island: the masked lengths change the association
    from axtrack_amd.detections import transition_cost_table
    H, W = 300, 420
    mask = synth.corridor_mask(H, W, width=24, pitch=80)
    mask[100:140, :] = False
    mask[110:130, 200:260] = True
    rng = np.random.default_rng(3)
    F, cap = 6, 32
    ys, xs = np.nonzero(mask)
    dets = []
    for t in range(F):
        k = rng.choice(len(ys), 24, replace=False)
        px, py = xs[k].copy(), ys[k].copy()
        px[:5] = rng.integers(0, W, 5); py[:5] = rng.integers(0, H, 5)
        dets.append((np.sort(rng.uniform(0.6, 1.0, 24).astype(np.float32))[::-1], px.astype(np.int64), py.astype(np.int64)))
    x = np.zeros((F, cap), np.int32); y = np.zeros((F, cap), np.int32)
    for t, d in enumerate(dets):
        x[t, :24] = d[1]; y[t, :24] = d[2]
    cnt = np.full(F, 24, np.int32)
    table, dmax = transition_cost_table(params.DEPLOYED)
    units = np.where(np.isfinite(table), np.rint(table * 1e6), 0).astype(np.int64)
    offs = np.arange(F + 1) * 24
    res = {}
    for name, grid, m in (('masked', hp.Grid(mask, False), mask), ('open', None, None)):
        track, _ = hp.hungarian_assoc(dev(x), dev(y), dev(cnt), H, W, dmax, units, 700000, mask=grid)
        flat = track.cpu().numpy()[:, :24].reshape(-1)
        res[name] = tracks_from_next(np.zeros(len(flat)), flat, offs)
        assert res[name] == orc.hungarian_assoc(dets, H, W, mask=m), name
    assert res['masked'] != res['open']


# ----------------------------------------------------------------------------------------- a-9 on a real mask
def test_path_cost_masked_grid_matches_oracle():
    """Corridor mask (BASELINE config 5 style), sources/targets on and off the mask, one outside the grid."""
    H, W = 300, 420
    mask = synth.corridor_mask(H, W, width=24, pitch=80)
    mask[100:140, :] = False                                    # a gap the paths must cross or walk around
    rng = np.random.default_rng(5)
    na, nb = 14, 17
    xa, ya = rng.integers(0, W, na), rng.integers(0, H, na)
    xb, yb = rng.integers(0, W, nb), rng.integers(0, H, nb)
    xa[0], ya[0] = -2, 10                                        # outside the grid
    xb[1], yb[1] = xa[2], ya[2]                                  # identical points: one cell
    for conn8 in (False, True):
        D = hp.path_cost(dev(xa, torch.int32), dev(ya, torch.int32), dev(xb, torch.int32), dev(yb, torch.int32),
                         H, W, dev(mask.astype(np.uint8)), 500, conn8).cpu().numpy()
        ref = orc.path_matrix((None, xa, ya), (None, xb, yb), H, W, mask, 500, conn8)
        assert np.array_equal(D, ref), (D != ref).sum()
    assert (D[0] == 500).all() and D[2, 1] == 1
    # an all-ones mask through the masked kernel equals the closed form
    ones = np.ones((H, W), np.uint8)
    D1 = hp.path_cost(dev(xa, torch.int32), dev(ya, torch.int32), dev(xb, torch.int32), dev(yb, torch.int32),
                      H, W, dev(ones), 500, False).cpu().numpy()
    D0 = hp.path_cost(dev(xa, torch.int32), dev(ya, torch.int32), dev(xb, torch.int32), dev(yb, torch.int32),
                      H, W, None, 500, False).cpu().numpy()
    assert np.array_equal(D1, D0)


@pytest.mark.parametrize('conn8', [False, True])
def test_path_cells_on_a_masked_grid_are_minimum_cost_paths(conn8):
    """axt_path_cells: every materialised path starts at its source, ends at its target, moves between neighbouring
    cells, has the oracle's number of cells, and costs (weight of every cell entered, {1 on mask, 65536 off}) exactly
    what an independent Dijkstra (scipy.sparse.csgraph) finds."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    H, W = 96, 130
    mask = synth.corridor_mask(H, W, width=10, pitch=34)
    mask[40:52, :] = False
    mask[44:47, 60:70] = True                                    # an island inside the gap
    rng = np.random.default_rng(11)
    na, nb = 9, 12
    xa, ya = rng.integers(0, W, na), rng.integers(0, H, na)
    xb, yb = rng.integers(0, W, nb), rng.integers(0, H, nb)
    xb[3], yb[3] = xa[4], ya[4]                                  # a one-cell path
    xa[0], ya[0] = W + 3, 5                                      # outside the grid: no paths
    max_dist = 90                                                # some pairs are too far / too long
    D, cells = hp.path_cells(dev(xa, torch.int32), dev(ya, torch.int32), dev(xb, torch.int32), dev(yb, torch.int32),
                             H, W, dev(mask.astype(np.uint8)), max_dist, conn8)
    D, cells = D.cpu().numpy(), cells.cpu().numpy()
    ref = orc.path_matrix((None, xa, ya), (None, xb, yb), H, W, mask, max_dist, conn8)
    assert np.array_equal(D, ref)
    # the grid as a graph: an edge into cell c costs weight(c)
    wgt = np.where(mask, 1.0, 65536.0)
    idx = np.arange(H * W).reshape(H, W)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn8 else [])
    src_n, dst_n, w_n = [], [], []
    for dy, dx in steps:
        ys, xs = np.mgrid[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)]
        src_n.append(idx[ys, xs].ravel()); dst_n.append(idx[ys + dy, xs + dx].ravel()); w_n.append(wgt[ys + dy, xs + dx].ravel())
    G = coo_matrix((np.concatenate(w_n), (np.concatenate(src_n), np.concatenate(dst_n))), (H * W, H * W)).tocsr()
    checked = 0
    for i in range(na):
        if not (0 <= xa[i] < W and 0 <= ya[i] < H):
            assert (D[i] == max_dist).all()
            continue
        best = dijkstra(G, indices=int(ya[i] * W + xa[i]))
        for j in range(nb):
            if D[i, j] >= max_dist:
                assert (cells[i, j] == -1).all()
                continue
            c = cells[i, j, :D[i, j]]
            assert (cells[i, j, D[i, j]:] == -1).all()
            assert c[0] == ya[i] * W + xa[i] and c[-1] == yb[j] * W + xb[j]
            r, q = c // W, c % W
            dr, dq = np.abs(np.diff(r)), np.abs(np.diff(q))
            assert np.all((np.maximum(dr, dq) == 1) if conn8 else (dr + dq == 1))
            assert len(set(c.tolist())) == len(c)
            assert wgt.ravel()[c[1:]].sum() == best[c[-1]]
            checked += 1
    assert checked > 30 and D[4, 3] == 1


def test_path_cache_round_trip_on_a_masked_grid(weights, tmp_path):
    """The path cache of a masked timelapse: written from axt_path_cells, its lengths are those the arc builder's own
    search finds, and reading it back gives the same trajectories."""
    import pickle
    import axtrack_amd
    frames = synth.synth_frames(7, 512, 512, seed=23)
    mask = synth.corridor_mask(512, 512, width=40, pitch=128)
    P = params.load_parameters()
    model = axtrack_amd.Detector(weights, max_batch=8)
    tl = axtrack_amd.Timelapse(frames, name='maskcache', mask=mask)
    ad = axtrack_amd.AxonDetections(model, tl, P, str(tmp_path))
    ad.detect_dataset()
    ad.assign_ids()
    ref_tracks, ref_cost = ad._track_flat.copy(), ad.mcf_total_cost
    ad.assign_ids(astar_paths_cache='to')
    assert np.array_equal(ad._track_flat, ref_tracks) and ad.mcf_total_cost == ref_cost
    paths = pickle.load(open(tmp_path / 'maskcache_astar_dets_paths.pkl', 'rb'))
    dists = ad.astar_dists()
    n_paths = 0
    for lbl, rows in paths.items():
        for i, row in enumerate(rows):
            for j, p in enumerate(row):
                assert (dists[lbl][i, j] == 500) if p is None else (p.getnnz() == dists[lbl][i, j])
                n_paths += p is not None
    assert n_paths > 50
    ad2 = axtrack_amd.AxonDetections(model, tl, P, str(tmp_path))
    ad2.detect_dataset()
    ad2.assign_ids(astar_paths_cache='from')
    assert np.array_equal(ad2._track_flat, ref_tracks) and ad2.mcf_total_cost == ref_cost


def test_inference_with_mask_end_to_end(weights):
    """512x512x7 with a corridor mask: the masked arc builder + flow solve equal the oracle's."""
    import axtrack_amd
    frames = synth.synth_frames(7, 512, 512, seed=31)
    mask = synth.corridor_mask(512, 512, width=40, pitch=128)
    P = params.load_parameters()
    model = axtrack_amd.Detector(weights, max_batch=8)
    tl = axtrack_amd.Timelapse(frames, name='synth', mask=mask)
    ad = axtrack_amd.inference(tl, model, None, P, None, None, None)
    yolo = ad._yolo.cpu().numpy()
    ref = orc.inference(frames, weights, mask=mask, P=orc.DEFAULTS, yolo=list(yolo))
    got = tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs)
    assert got == ref['trajs'] and ad.mcf_total_cost == ref['total_cost']


def test_full_size_properties_c5_share(weights):
    """One GPU's share of BASELINE config 5 (1024x1024 frames with an occlusion mask, 64 detection frames, path costs on
    the masked grid, global flow solve): properties that hold at any size. Every link of every trajectory is an
    admissible arc whose length the exact search reproduces, trajectories are node-disjoint, and a second run is
    identical."""
    import axtrack_amd
    frames = synth.synth_frames(68, 1024, 1024, seed=3)
    mask = synth.corridor_mask(1024, 1024, width=40, pitch=128)
    frames = frames * mask[None].astype(np.float32)
    P = params.load_parameters()
    model = axtrack_amd.Detector(weights, max_batch=64)
    tl = axtrack_amd.Timelapse(frames, name='c5', mask=mask)
    ad = axtrack_amd.inference(tl, model, None, P, None, None, None)
    cnt, conf, x, y = ad._host_dets()
    assert len(cnt) == 64 and cnt.sum() > 3000
    tracks = tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs)
    assert P['MCF_MIN_FLOW'] <= len(tracks) <= P['MCF_MAX_FLOW'] and len(tracks) == ad.n_ids
    seen, links = set(), []
    for tr in tracks:
        for (f0, i0), (f1, i1) in zip(tr[:-1], tr[1:]):
            assert f1 - f0 in (1, 2)
            links.append((f0, i0, f1, i1))
        for node in tr:
            assert node not in seen
            seen.add(node)
    assert len(links) > 1000
    # the exact search on a sample of links: the length that made the arc admissible
    rng = np.random.default_rng(0)
    grid = ad._mask_dev()
    for k in rng.choice(len(links), 40, replace=False):
        f0, i0, f1, i1 = links[k]
        D = hp.path_cost(ad.d_x[f0, i0:i0 + 1], ad.d_y[f0, i0:i0 + 1], ad.d_x[f1, i1:i1 + 1], ad.d_y[f1, i1:i1 + 1],
                         1024, 1024, grid, 500, False)
        assert int(D.item()) <= (251 if f1 - f0 == 1 else 86)
    ad2 = axtrack_amd.inference(tl, model, None, P, None, None, None)
    assert np.array_equal(ad2._track_flat, ad._track_flat) and ad2.mcf_total_cost == ad.mcf_total_cost


def test_masked_path_lengths_on_a_mask_with_many_components():
    """More than 64 components: the grid keeps no per-component off-cell fields and the arc builder resolves targets
    in other components with the general search instead of the windowed one -- same path lengths as the oracle."""
    H, W = 208, 224
    mask = np.zeros((H, W), bool)
    for r in range(9):
        for c in range(9):
            mask[8 + r * 22:8 + r * 22 + 14, 8 + c * 24:8 + c * 24 + 16] = True      # 81 islands
    rng = np.random.default_rng(4)
    ys, xs = np.nonzero(mask)
    F, cap = 3, 16
    dets = []
    for t in range(F):
        k = rng.choice(len(ys), 10, replace=False)
        px, py = xs[k].copy(), ys[k].copy()
        px[:2] = rng.integers(0, W, 2); py[:2] = rng.integers(0, H, 2)               # two anywhere
        dets.append((np.sort(rng.uniform(0.6, 1.0, 10).astype(np.float32))[::-1], px.astype(np.int64), py.astype(np.int64)))
    x = np.zeros((F, cap), np.int32); y = np.zeros((F, cap), np.int32)
    for t, d in enumerate(dets):
        x[t, :10] = d[1]; y[t, :10] = d[2]
    cnt = np.full(F, 10, np.int32)
    from axtrack_amd.detections import transition_cost_table
    table, dmax = transition_cost_table(params.DEPLOYED)
    units = np.where(np.isfinite(table), np.rint(table * 1e6), 0).astype(np.int64)
    row_ptr, col, length, gap, cost = hp.build_arcs(dev(x), dev(y), dev(cnt), H, W, dmax, units, hp.Grid(mask, False), 500, False)
    row_ptr, col, length, gap = (v.cpu().numpy() for v in (row_ptr, col, length, gap))
    got = {(a, int(col[e])): int(length[e]) for a in range(30) for e in range(row_ptr[a], row_ptr[a + 1])}
    want = {}
    for t in range(F):
        for g in (1, 2):
            if t + g >= F:
                continue
            D = orc.path_matrix(dets[t], dets[t + g], H, W, mask, 500, False)
            for i, j in zip(*np.nonzero(D <= dmax[g - 1])):
                want[(t * 10 + int(i), (t + g) * 10 + int(j))] = int(D[i, j])
    assert got == want and len(want) > 50


@pytest.mark.parametrize('variant', ['appearance', 'conn8'])
def test_path_cache_with_the_appearance_term_and_on_the_8_connected_grid(weights, tmp_path, variant):
    """Two more uses of the reference's path cache: read back while MCF_VIS_SIM_WEIGHT > 0 (what its parameter
    search does, AxonDetections.py:882,911-912: lengths from the file, histograms from the pixels), and written on the
    8-connected grid (diagonal-first staircases of max(|dx|,|dy|)+1 cells) -- each reproduces the direct result."""
    import pickle
    import axtrack_amd
    frames = synth.synth_frames(9, 512, 512, seed=29) * np.float32(0.5)
    P = params.load_parameters()
    if variant == 'appearance':
        P['MCF_VIS_SIM_WEIGHT'] = 0.2
    else:
        P['ASTAR_8_CONNECTED'] = True
    model = axtrack_amd.Detector(weights, max_batch=8)
    tl = axtrack_amd.Timelapse(frames, name='c2')
    ad = axtrack_amd.AxonDetections(model, tl, P, str(tmp_path))
    ad.detect_dataset()
    ad.assign_ids(astar_paths_cache='to')
    ref_tracks, ref_cost = ad._track_flat.copy(), ad.mcf_total_cost
    paths = pickle.load(open(tmp_path / 'c2_astar_dets_paths.pkl', 'rb'))
    dists = ad.astar_dists()
    n = 0
    for lbl, rows in paths.items():
        for i, row in enumerate(rows):
            for j, p in enumerate(row):
                if p is None:
                    continue
                assert p.getnnz() == dists[lbl][i, j]
                dr, dc = np.abs(np.diff(p.row)), np.abs(np.diff(p.col))
                assert np.all(np.maximum(dr, dc) == 1) if variant == 'conn8' else np.all(dr + dc == 1)
                n += 1
    assert n > 100
    ad2 = axtrack_amd.AxonDetections(model, tl, P, str(tmp_path))
    ad2.detect_dataset()
    ad2.assign_ids(astar_paths_cache='from')
    assert np.array_equal(ad2._track_flat, ref_tracks) and ad2.mcf_total_cost == ref_cost


# ----------------------------------------------------------------------------------------- multi-GPU path
@pytest.mark.parametrize('world', [2, 4])
def test_two_rank_frame_sharding(weights, world):
    """Two (and four) ranks (gloo, all on cuda:0) each detect their block of the frames, all-gather the detections, build the
    arcs / solve the frame pairs of their own frames (and, for the flow tracker, their run of the solver's time blocks),
    exchange them and finish the association: every rank must equal the single-process result bit for bit, in every
    association mode (Hungarian, flow, flow + appearance, flow on a masked grid)."""
    import socket
    import torch.multiprocessing as mp
    import gpu_shard_worker
    total, seed = 16, 41
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=gpu_shard_worker.run, args=(r, world, port, q, total, seed)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    frames = synth.synth_frames(total + 4, 512, 512, seed=seed)
    import axtrack_amd
    for mode in ('hungarian', 'mcf', 'mcf+appearance', 'mcf+mask', 'hungarian+mask'):
        P = params.load_parameters()
        P['ASSOCIATION'] = mode.split('+')[0]
        if mode.endswith('appearance'):
            P['MCF_VIS_SIM_WEIGHT'] = 0.2
        if mode.endswith('mask'):                # path searches on a masked grid: every rank its own frames' sources
            tl = axtrack_amd.Timelapse(frames, name='shard', mask=synth.corridor_mask(512, 512, width=40, pitch=128))
            ad = axtrack_amd.inference(tl, axtrack_amd.Detector(weights, max_batch=32), None, P, None, None, None)
        else:
            ad = _run_inference(frames, weights, P, name='shard')
        ref = (ad.n_ids, ad._track_flat.tobytes(), ad.IDed_dets_all.to_numpy().tobytes(), list(ad.IDed_dets_all.index))
        for r in range(world):
            assert res[r][mode][:4] == ref, mode          # the table assembled from the ranks' blocks is the global one
            rows, cols = res[r][mode][4]
            assert cols == 3 * (total // world) and rows <= ad.n_ids


def test_two_rank_sharding_with_a_tile_that_is_empty_on_one_rank(weights):
    """The reference drops a tile only if it is empty at EVERY time point (Timelapse.py:551-558). Frame-sharded, the
    right tile is empty in all of rank 0's frames: its own scan would keep one tile (capacity 144), rank 1's two (288).
    The gather refuses mismatched shapes; after Timelapse.sync_tile_occupancy() both ranks use the timelapse-wide
    list and reproduce the single-process result."""
    import socket
    import torch.multiprocessing as mp
    import gpu_shard_worker
    import axtrack_amd
    total, seed = 12, 77
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=gpu_shard_worker.run_tiles, args=(r, 2, port, q, total, seed)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0]['local'] == [(0, 0)] and res[1]['local'] == [(0, 0), (0, 1)]
    assert res[0]['refused'] and res[1]['refused']
    frames = gpu_shard_worker.tiles_frames(total, seed)
    P = dict(params.load_parameters(), ASSOCIATION='hungarian')
    ad = _run_inference(frames, weights, P, name='tiles')
    for r in (0, 1):
        assert res[r]['tiles'] == ad.tile_yx == [(0, 0), (0, 1)] and res[r]['cap'] == 288
        assert res[r]['n_ids'] == ad.n_ids and res[r]['track'] == ad._track_flat.tobytes()
        assert res[r]['table'] == ad.IDed_dets_all.to_numpy().tobytes()


# ----------------------------------------------------------------------------------------- f-2 (next row)
def test_path_cache_round_trip_in_the_references_format(weights, tmp_path):
    """'{name}_astar_dets_paths.pkl': written ('to') in the reference's format -- nested lists of scipy coo matrices /
    None per frame pair -- read back ('from') through d_len_table of axt_build_arcs, and consumed by the oracle's
    restatement of _get_astar_path_distances: the same path lengths, arcs and trajectories every way."""
    import pickle
    from scipy import sparse
    frames = synth.synth_frames(9, 512, 512, seed=19)
    P = params.load_parameters()
    import axtrack_amd
    model = axtrack_amd.Detector(weights, max_batch=8)
    tl = axtrack_amd.Timelapse(frames, name='cachetest')
    ad = axtrack_amd.AxonDetections(model, tl, P, str(tmp_path))
    ad.detect_dataset()
    ad.assign_ids(astar_paths_cache='to')
    ref_tracks, ref_cost = ad._track_flat.copy(), ad.mcf_total_cost
    paths = pickle.load(open(tmp_path / 'cachetest_astar_dets_paths.pkl', 'rb'))
    dists = ad.astar_dists()
    assert paths.keys() == dists.keys()
    cnt, _, x, y = ad._host_dets()
    for lbl, rows in paths.items():
        D = dists[lbl]
        for i, row in enumerate(rows):
            for j, p in enumerate(row):
                if p is None:
                    assert D[i, j] == 500
                    continue
                assert sparse.isspmatrix_coo(p) and p.shape == (512, 512) and p.dtype == bool
                assert p.getnnz() == D[i, j]                                  # what _get_astar_path_distances reads
                r, c = p.row, p.col
                assert np.all(np.abs(np.diff(r)) + np.abs(np.diff(c)) == 1)   # 4-connected, no cell twice
    # read it back: same arcs -> same optimum
    ad2 = axtrack_amd.AxonDetections(model, tl, P, str(tmp_path))
    ad2.detect_dataset()
    ad2.assign_ids(astar_paths_cache='from')
    assert np.array_equal(ad2._track_flat, ref_tracks) and ad2.mcf_total_cost == ref_cost
    # a cache in which one admissible pair was declared unreachable changes the problem
    lbl = next(k for k, rows in paths.items() if any(p is not None and p.getnnz() < 100 for r in rows for p in r))
    i, j = next((i, j) for i, r in enumerate(paths[lbl]) for j, p in enumerate(r) if p is not None and p.getnnz() < 100)
    paths[lbl][i][j] = None
    pickle.dump(paths, open(tmp_path / 'cachetest_astar_dets_paths.pkl', 'wb'))
    ad3 = axtrack_amd.AxonDetections(model, tl, P, str(tmp_path))
    ad3.detect_dataset()
    ad3.assign_ids(astar_paths_cache='from')
    Dm = {k: v.copy() for k, v in dists.items()}
    Dm[lbl][i, j] = 500
    dets = [(ad._host_dets()[1][t, :cnt[t]], x[t, :cnt[t]], y[t, :cnt[t]]) for t in range(len(cnt))]
    trajs, total = orc.mcf_solve(dets, Dm, orc.DEFAULTS, 'cachetest')
    got = tracks_from_next(np.zeros(len(ad3._track_flat)), ad3._track_flat, ad3._offs)
    assert got == trajs and ad3.mcf_total_cost == total


# ----------------------------------------------------------------------------------------- f-3 (next row)
def test_box_histograms_bit_exact_against_oracle():
    """feature_model on the GPU: boxes in the interior, on every edge and corner, partly and completely outside the
    image, pixel values on both sides of the [0,1) histogram range and exactly on bin boundaries."""
    rng = np.random.default_rng(5)
    H, W, F, cap = 200, 260, 3, 16
    frames = (rng.random((F + 4, H, W)) * 1.3).astype(np.float32)
    frames[rng.random(frames.shape) < 0.6] = 0
    frames[:, 50:60, 50:60] = np.float32(1.0)                       # == upper bound: dropped
    frames[:, 60:70, 50:60] = (np.arange(10) / 180).astype(np.float32)[None, None, :]   # bin boundaries
    x = rng.integers(-40, W + 40, (F, cap)).astype(np.int32)
    y = rng.integers(-40, H + 40, (F, cap)).astype(np.int32)
    x[0, :6] = [0, W - 1, 0, W - 1, 35, W + 100]
    y[0, :6] = [0, 0, H - 1, H - 1, 35, H + 100]                    # corners, exact fit, far outside (empty crop)
    cnt = np.array([cap, 9, 0], np.int32)
    hist, hsum = hp.box_histograms(dev(frames), dev(x), dev(y), dev(cnt), t_offset=2)
    hist, hsum = hist.cpu().numpy(), hsum.cpu().numpy()
    for f in range(F):
        n = int(cnt[f])
        ref = orc.box_histograms(frames[f + 2], x[f, :n], y[f, :n])
        assert np.array_equal(hist[f, :n].view(np.uint32), ref.view(np.uint32)), f
        ref_sum = np.array([sum(float(v) for v in r) for r in ref])              # f64, in bin order
        assert np.array_equal(hsum[f, :n], ref_sum), f
        assert not hist[f, n:].any()


def test_arcs_with_appearance_term_against_oracle(golden):
    """MCF_VIS_SIM_WEIGHT = 0.3: candidate pairs up to D = 394, per-pair cost from the path length AND the Bhattacharyya
    distance of the two crops, admission by cost < MCF_EDGE_COST_THR -- arcs and integer costs as the oracle's
    restatement of transition_model (mincostflow_models.py:100-118)."""
    from axtrack_amd.detections import transition_cost_table
    g = golden('detect_1024')
    dets = golden_dets(g)
    F, cap = len(dets), 576
    frames = synth.synth_frames(F + 4, 1024, 1024, seed=31) * np.float32(0.4)      # blobs inside the histogram range
    x = np.zeros((F, cap), np.int32); y = np.zeros((F, cap), np.int32)
    for t, d in enumerate(dets):
        x[t, :len(d[1])] = d[1]; y[t, :len(d[2])] = d[2]
    cnt = np.array([len(d[0]) for d in dets], np.int32)
    P = dict(params.load_parameters(), MCF_VIS_SIM_WEIGHT=0.3)
    _, dmax = transition_cost_table(P, vis_sim=1.0)
    assert dmax[0] > 251                                                          # more candidates than without the term
    hist, hsum = hp.box_histograms(dev(frames), dev(x), dev(y), dev(cnt), t_offset=2)
    vis = dict(hist=hist, hsum=hsum, weight=0.3, miss_rate=P['MCF_MISS_RATE'], thr=P['MCF_EDGE_COST_THR'])
    row_ptr, col, length, gap, cost = hp.build_arcs(dev(x), dev(y), dev(cnt), 1024, 1024, dmax, vis=vis)
    row_ptr, col, cost = row_ptr.cpu().numpy(), col.cpu().numpy(), cost.cpu().numpy()
    # oracle: the same arcs from its own flow-graph builder
    Po = dict(orc.DEFAULTS, MCF_VIS_SIM_WEIGHT=0.3)
    D = orc.all_path_matrices(dets, 1024, 1024)
    tail, head, ocost, offs = orc.build_flow_graph(dets, D, Po, images=[frames[t + 2] for t in range(F)])
    tr = (tail % 2 == 1) & (tail > 1) & (head > 1)                                 # transition arcs v_a -> u_b
    ref = sorted(zip(((tail[tr] - 3) // 2).tolist(), ((head[tr] - 2) // 2).tolist(), ocost[tr].tolist()))
    n_det = int(offs[-1])
    got = sorted((a, int(col[e]), int(cost[e])) for a in range(n_det) for e in range(row_ptr[a], row_ptr[a + 1]))
    assert len(got) == len(ref) > 1000
    assert [r[:2] for r in got] == [r[:2] for r in ref]                            # the same arcs
    du = np.array([(a[2] >> 16) - (b[2] >> 16) for a, b in zip(got, ref)])
    assert np.abs(du).max() <= 1 and (du != 0).mean() < 1e-3                       # f64 log: 1 ulp on the GPU
    assert all((a[2] & 0xFFFF) == (b[2] & 0xFFFF) for a, b in zip(got, ref))       # identity hash bits


def test_inference_with_appearance_term(weights):
    """End to end with MCF_VIS_SIM_WEIGHT = 0.2 (the reference's search grid uses 0.1 / 0.4, experiment.py:227):
    same trajectories and IDed_dets_all as the oracle fed with the same YOLO grids."""
    frames = synth.synth_frames(12, 1024, 1024, seed=13) * np.float32(0.5)
    P = dict(params.load_parameters(), MCF_VIS_SIM_WEIGHT=0.2)
    ad = _run_inference(frames, weights, P)
    ref = orc.inference(frames, weights, P=dict(orc.DEFAULTS, MCF_VIS_SIM_WEIGHT=0.2), yolo=list(ad._yolo.cpu().numpy()))
    assert ad.n_ids == len(ref['trajs'])
    got_tracks = tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs)
    assert got_tracks == ref['trajs']
    assert abs(ad.mcf_total_cost - ref['total_cost']) <= 65536 * 4                 # a few cost units (f64 log, 1 ulp)
    assert np.array_equal(np.nan_to_num(ad.IDed_dets_all.to_numpy(), nan=-1), np.nan_to_num(ref['ided_all'][3], nan=-1))
    # and it is a different problem from the one without the term
    ad0 = _run_inference(frames, weights, params.load_parameters())
    assert ad0.mcf_total_cost != ad.mcf_total_cost


def test_inference_with_appearance_term_on_a_masked_grid(weights):
    """MCF_VIS_SIM_WEIGHT > 0 widens the candidate distances beyond the 251-cell window of the hot-path searches; on a
    masked grid the arc builder then runs on the exact path lengths. Same trajectories as the oracle."""
    import axtrack_amd
    frames = synth.synth_frames(9, 512, 512, seed=33) * np.float32(0.5)
    mask = synth.corridor_mask(512, 512, width=40, pitch=128)
    frames = frames * mask[None].astype(np.float32)
    P = dict(params.load_parameters(), MCF_VIS_SIM_WEIGHT=0.3, MCF_MIN_FLOW=1)
    model = axtrack_amd.Detector(weights, max_batch=8)
    ad = axtrack_amd.inference(axtrack_amd.Timelapse(frames, name='synth', mask=mask), model, None, P, None, None, None)
    ref = orc.inference(frames, weights, mask=mask, P=dict(orc.DEFAULTS, MCF_VIS_SIM_WEIGHT=0.3, MCF_MIN_FLOW=1),
                        yolo=list(ad._yolo.cpu().numpy()))
    got = tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs)
    assert got == ref['trajs'] and abs(ad.mcf_total_cost - ref['total_cost']) <= 65536 * 4


# ----------------------------------------------------------------------------------------- f-4 (next row)
def test_detection_metrics_match_the_reference(golden):
    """compute_TP_FP_FN over all frames and the 13 thresholds in one launch, and the per-frame API, against what the
    reference itself returned (tests/golden/metrics.npz) -- including the frame without labels (phantom label at
    the origin) and the FP / FN masks at BBOX_THRESHOLD."""
    import axtrack_amd, pandas as pd
    from axtrack_amd.detections import AxonDetections
    g, m = golden('detect_1024'), golden('metrics')
    dets = golden_dets(g)
    tl = axtrack_amd.Timelapse(np.zeros((len(dets) + 4, 1024, 1024), np.float32), name='synth')
    ad = AxonDetections(None, tl, params.load_parameters(), None)
    ad._set_detections_from_tables([pd.DataFrame({'conf': c, 'anchor_x': x, 'anchor_y': y}) for c, x, y in dets])
    offs = np.concatenate([[0], np.cumsum(m['gt_counts'])])
    ad.set_groundtruth([(m['gt_x'][offs[t]:offs[t + 1]], m['gt_y'][offs[t]:offs[t + 1]]) for t in range(len(dets))])
    assert np.array_equal(ad.all_conf_thrs, m['all_conf_thrs'])
    cm = ad.detection_confusion()
    assert np.array_equal(cm, m['confusion'])
    doffs = np.concatenate([[0], np.cumsum(g['counts'])])
    for t in range(len(dets)):
        one = ad.compute_TP_FP_FN('all', t)
        assert np.array_equal(one, m['confusion'][t])
        assert np.array_equal(ad.compute_prc_rcl_F1(one), m['prc_rcl_f1'][t])
        assert np.array_equal(ad.get_detection_metrics('all', t, True), m['prc_rcl_f1'][t])
        fp, fn = ad.compute_TP_FP_FN('all', t, return_FP_FN_mask=True)
        assert np.array_equal(fp, m['fp_mask_at_bbox_thr'][doffs[t]:doffs[t + 1]])
        if m['gt_counts'][t]:
            lo = offs[t] + sum(1 for q in range(t) if m['gt_counts'][q] == 0)
            assert np.array_equal(fn, m['fn_mask_at_bbox_thr'][lo:lo + m['gt_counts'][t]])
    # 'confident' selection and an empty detection side against the oracle
    conf_t = ad.compute_TP_FP_FN('confident', 0)
    d0 = dets[0]
    keep = d0[0] > np.float32(0.7)
    assert np.array_equal(conf_t, orc.detection_confusion((d0[0][keep], d0[1][keep], d0[2][keep]), *ad._gt[0]))
    ad2 = AxonDetections(None, tl, params.load_parameters(), None)
    ad2._set_detections_from_tables([pd.DataFrame({'conf': [], 'anchor_x': [], 'anchor_y': []}) for _ in dets])
    ad2.set_groundtruth(ad._gt)
    for t in range(len(dets)):
        assert np.array_equal(ad2.detection_confusion()[t], orc.detection_confusion(([], [], []), *ad._gt[t]))


# ----------------------------------------------------------------------------------------- f-1 (next row)
def test_preprocess_fused_pass_matches_oracle():
    rng = np.random.default_rng(3)
    # H*W = 126 000 (and 124 800 below) is a multiple of 8: both shapes take the 8-pixel vector branch only. The scalar branch,
    # the tail and the grid-stride loop are run by tests/test_stagekernels_gpu.py::test_preprocess.
    T, H, W = 5, 300, 420
    raw = rng.integers(0, 5000, (T, H, W)).astype(np.uint16)
    raw[rng.uniform(size=raw.shape) < 0.7] = 0
    mask = synth.corridor_mask(H, W, 40, 128)
    from axtrack_amd.timelapse import preprocess
    got = preprocess(raw, mask, offset=121, clip=55, log_correct=True, scale=0.015176106).cpu().numpy()
    ref = orc.preprocess(raw, mask, 121 / 2 ** 16, 55 / 2 ** 16, True, 0.015176106)
    assert np.array_equal(got == 0, ref == 0)               # same sparsity pattern (mask, offset clamp, clip)
    np.testing.assert_array_max_ulp(got, ref, maxulp=2)     # log2f: GPU and numpy are each within 1 ulp
    got2 = preprocess(raw[:, :, :416].copy(), None, offset=0, clip=0, log_correct=False, scale=1.0).cpu().numpy()
    assert np.array_equal(got2, orc.preprocess(raw[:, :, :416], None, 0, 0, False, 1.0))


def test_example_script_runs_the_three_step_api(tmp_path):
    """examples/test.py: setup_inference -> prepare_input_data (raw uint16) -> inference -> IDed_dets_all, with the
    'to' caches written in the reference's file layout and readable with 'from'."""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location('example_test', os.path.join(os.path.dirname(__file__), '..', 'examples', 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ad = mod.main(T=12, dest_dir=str(tmp_path))
    df = ad.IDed_dets_all
    assert df.shape[1] == 3 * 8 and df.index.name == 'axonID' and len(df) == ad.n_ids >= 1
    assert os.path.exists(tmp_path / 'axon_dets' / 'example_timelapse__detections.pkl')
    assert os.path.exists(tmp_path / 'axon_dets' / 'example_timelapse__IDed_detections.pkl')
    # the caches round-trip
    import axtrack_amd
    ad2 = axtrack_amd.AxonDetections(ad.model, ad.dataset, ad.P, ad.dir)
    ad2.detect_dataset(cache='from')
    ad2.assign_ids(assigedIDs_cache='from')
    assert np.array_equal(np.nan_to_num(ad2.IDed_dets_all.to_numpy(), nan=-1), np.nan_to_num(df.to_numpy(), nan=-1))


@pytest.mark.parametrize('conn8', [False, True])
@pytest.mark.parametrize('comb', [False, True])
def test_build_arcs_masked_grid_matches_oracle(conn8, comb):
    """The bit-parallel on-mask BFS + connected components + the windowed search for targets in other components /
    off the mask must give exactly the arcs the oracle's per-pair searches give: corridor mask with a gap and a
    disconnected island, detections on and off the mask. comb: a bar along the top joins the corridors into one
    component, so neighbouring corridors are connected on the mask -- by detours that are mostly too long to count,
    although crossing the wall would be short."""
    from axtrack_amd.detections import transition_cost_table
    H, W = 300, 420
    mask = synth.corridor_mask(H, W, width=24, pitch=80)
    mask[100:140, :] = False
    mask[110:130, 200:260] = True                               # an island: on the mask but in its own component
    if comb:
        mask[0:6, :] = True
    rng = np.random.default_rng(11 + conn8 + 2 * comb)
    F, cap = 5, 40
    ys, xs = np.nonzero(mask)
    dets = []
    for t in range(F):
        n = int(rng.integers(18, 30))
        k = rng.choice(len(ys), n, replace=False)
        px, py = xs[k].copy(), ys[k].copy()
        off = rng.uniform(size=n) < 0.25                          # a quarter of them anywhere, mostly off the mask
        px[off] = rng.integers(0, W, off.sum()); py[off] = rng.integers(0, H, off.sum())
        if t == 2:
            px[0], py[0] = 230, 120                               # on the island
            px[1], py[1] = -4, 50                                 # outside the grid
        conf = np.sort(rng.uniform(0.55, 1.1, n).astype(np.float32))[::-1]
        dets.append((conf, px.astype(np.int64), py.astype(np.int64)))
    x = np.zeros((F, cap), np.int32); y = np.zeros((F, cap), np.int32)
    for t, d in enumerate(dets):
        x[t, :len(d[1])] = d[1]; y[t, :len(d[2])] = d[2]
    cnt = np.array([len(d[0]) for d in dets], np.int32)
    P = dict(params.DEPLOYED)
    table, dmax = transition_cost_table(P)
    units = np.where(np.isfinite(table), np.rint(table * 1e6), 0).astype(np.int64)
    grid = hp.Grid(mask, conn8)
    row_ptr, col, length, gap, cost = hp.build_arcs(dev(x), dev(y), dev(cnt), H, W, dmax, units, grid, 500, conn8)
    # oracle CSR (per-pair searches on the full grid)
    offs = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    rows = [[] for _ in range(int(offs[-1]))]
    for t in range(F):
        for g in (1, 2):
            tb = t + g
            if tb >= F:
                continue
            D = orc.path_matrix(dets[t], dets[tb], H, W, mask, 500, conn8)
            c = orc.transition_cost(D, g, P['MCF_MISS_RATE'])
            for i, j in zip(*np.nonzero(c < P['MCF_EDGE_COST_THR'])):
                a, b = int(offs[t] + i), int(offs[tb] + j)
                rows[a].append((g, b, int(D[i, j]), orc.arc_cost_int(c[i, j], 3, a, b)))
    r_ptr, r_col, r_len, r_gap, r_cost = [0], [], [], [], []
    for r in rows:
        for g, b, d, ci in sorted(r):
            r_col.append(b); r_len.append(d); r_gap.append(g); r_cost.append(ci)
        r_ptr.append(len(r_col))
    n_det = int(offs[-1])
    assert np.array_equal(row_ptr[:n_det + 1].cpu().numpy(), np.array(r_ptr))
    assert np.array_equal(col.cpu().numpy(), np.array(r_col, np.int32))
    assert np.array_equal(length.cpu().numpy(), np.array(r_len, np.int16))
    assert np.array_equal(gap.cpu().numpy(), np.array(r_gap, np.uint8))
    assert np.array_equal(cost.cpu().numpy(), np.array(r_cost, np.int64))
    assert len(r_col) > 100


def test_cnn_on_frame_width_not_multiple_of_four(detector, weights):
    """W = 701, H = 530: the first conv's aligned 16-byte staging cannot be used (rows are not 16-byte aligned and the
    right-edge tile is 189 px wide); the per-float path must give the same result as the oracle on the zero-padded
    tile stack."""
    frames = synth.synth_frames(6, 530, 701, seed=17)
    fr = dev(frames)
    keep = hp.tile_occupancy(fr)
    assert keep == [(0, 0), (0, 1), (1, 0), (1, 1)]
    y = detector.detect_frames(fr, keep).cpu().numpy()
    for t in range(2):
        ref = orc.cnn_forward(weights, orc.frame_tile_stack(frames, t, keep))
        np.testing.assert_allclose(y[t], ref, atol=CNN_ATOL, rtol=CNN_RTOL)


def test_cnn_when_workgroups_share_a_cu(detector, weights):
    """1024x1024 frames, 2 detection frames = 8 tile-forwards: the persistent stride-2 kernels then run two
    workgroups per CU with two tiles each. A 16-byte buffer store whose data registers were rewritten too early
    corrupted ~0.05 % of conv block 0's outputs in exactly this situation (and only then)."""
    frames = synth.synth_frames(6, 1024, 1024, seed=29)
    fr = dev(frames)
    keep = hp.tile_occupancy(fr)
    assert len(keep) == 4
    y = detector.detect_frames(fr, keep).cpu().numpy()
    y2 = detector.detect_frames(fr, keep).cpu().numpy()
    assert np.array_equal(y, y2)                              # and it is deterministic
    for t in range(2):
        ref = orc.cnn_forward(weights, orc.frame_tile_stack(frames, t, keep))
        np.testing.assert_allclose(y[t], ref, atol=CNN_ATOL, rtol=CNN_RTOL)


def test_end_to_end_detections_against_oracle_cnn(weights):
    """Whole detection path (HIP CNN included) against the oracle's own CNN on 40 frames: the two f32 forward passes
    differ by ~1e-6, which can flip an anchor by one pixel when the pre-rounding value sits on a .5 boundary or move a
    confidence across the 0.55 floor. Everything else must be identical: every HIP detection has an oracle twin within
    1 px whose confidence agrees to 1e-5, except confidences within 1e-5 of the floor."""
    frames = synth.synth_frames(44, 512, 512, seed=23)
    P = params.load_parameters()
    P['ASSOCIATION'] = 'hungarian'
    ad = _run_inference(frames, weights, P)
    cnt, conf, x, y = ad._host_dets()
    ref = orc.detect_dataset(frames, weights)
    exact = 0
    for t, (rc, rx, ry) in enumerate(ref):
        n = int(cnt[t])
        mine = {(int(a), int(b)): float(c) for a, b, c in zip(x[t, :n], y[t, :n], conf[t, :n])}
        theirs = {(int(a), int(b)): float(c) for a, b, c in zip(rx, ry, rc)}
        exact += len(set(mine) & set(theirs))
        for (a, b), c in mine.items():
            if (a, b) in theirs:
                assert abs(theirs[(a, b)] - c) < 1e-5
                continue
            near = [(abs(a - a2) + abs(b - b2), c2) for (a2, b2), c2 in theirs.items() if abs(a - a2) <= 1 and abs(b - b2) <= 1]
            assert (near and abs(min(near)[1] - c) < 1e-5) or abs(c - 0.55) < 1e-5, f'frame {t}: detection {(a, b, c)} has no oracle twin'
        assert abs(len(mine) - len(theirs)) <= 1
    total = int(cnt.sum())
    assert exact >= 0.995 * total, f'only {exact}/{total} detections identical'


def test_mcf_parameter_search_rows_match_the_oracle(golden, tmp_path):
    """search_MCF_params (AxonDetections.py:845-922) over a small grid: every row's association is the oracle's
    under those parameters (scored with the same tracking metrics), the combination that produced the labels scores
    perfectly, the CSV has the reference's columns and the parameters are restored."""
    import axtrack_amd, pandas as pd
    from axtrack_amd import mot_metrics
    from axtrack_amd.detections import AxonDetections
    g = golden('detect_1024')
    dets = golden_dets(g)
    tl = axtrack_amd.Timelapse(np.zeros((len(dets) + 4, 1024, 1024), np.float32), name='synth')
    P = params.load_parameters()
    ad = AxonDetections(None, tl, P, str(tmp_path))
    ad._set_detections_from_tables([pd.DataFrame({'conf': c, 'anchor_x': x, 'anchor_y': y}) for c, x, y in dets])
    # labels = the association under the deployed parameters
    ad.assign_ids()
    frame, tid, _, x, y = ad.ided_arrays()
    ad.set_groundtruth([(x[frame == t], y[frame == t], tid[frame == t]) for t in range(len(dets))])
    grid = dict(edge_cost_thr_values=[0.4, P['MCF_EDGE_COST_THR']], entry_exit_cost_values=[0.9, P['MCF_ENTRY_EXIT_COST']],
                miss_rate_values=[P['MCF_MISS_RATE']], vis_sim_weight_values=[0], conf_capping_method_values=['ceil', 'scale_to_max'])
    res = ad.search_MCF_params(**grid)
    assert ad.P == P
    assert list(res.columns) == ['edge_cost_thr', 'entry_exit_cost', 'miss_rate', 'vis_sim_weight', 'conf_capping_method'] \
        + mot_metrics.MOTCHALLENGE_METRICS
    assert len(res) == 8
    back = pd.read_csv(tmp_path / 'MCF_params_results.csv', index_col=0)
    assert list(back.columns) == list(res.columns) and len(back) == 8
    target = ad.get_frame_dets('groundtruth', None, libmot=True)
    D = orc.all_path_matrices(dets, 1024, 1024)
    n_perfect = 0
    for _, row in res.iterrows():
        Po = dict(orc.DEFAULTS, MCF_EDGE_COST_THR=row.edge_cost_thr, MCF_ENTRY_EXIT_COST=row.entry_exit_cost,
                  MCF_MISS_RATE=row.miss_rate, MCF_VIS_SIM_WEIGHT=row.vis_sim_weight, MCF_CONF_CAPPING_METHOD=row.conf_capping_method)
        trajs, _ = orc.mcf_solve(dets, D, Po)
        rows = [[f, i, dets[f][1][k] - 35, dets[f][2][k] - 35] for i, tr in enumerate(trajs or []) for f, k in tr]
        pred = pd.DataFrame(rows, columns=['FrameId', 'Id', 'X', 'Y']).set_index(['FrameId', 'Id']) if rows else None
        want = mot_metrics.summarize(mot_metrics.compare_to_groundtruth(target, pred, 23.0 ** 2))
        got = row[mot_metrics.MOTCHALLENGE_METRICS].astype(float)
        assert np.allclose(got.to_numpy(), want.to_numpy(), rtol=0, atol=1e-12, equal_nan=True), (row, want)
        perfect = row.mota == 1 and row.idf1 == 1 and row.num_switches == 0
        is_label_combo = (row.edge_cost_thr == P['MCF_EDGE_COST_THR'] and row.entry_exit_cost == P['MCF_ENTRY_EXIT_COST']
                          and row.conf_capping_method == P['MCF_CONF_CAPPING_METHOD'])
        assert perfect or not is_label_combo
        n_perfect += perfect
    assert 1 <= n_perfect < 8                       # the grid does change the association


def test_mcf_parameter_search_on_a_masked_grid_with_wide_thresholds(tmp_path):
    """On a masked grid the search computes the exact path lengths once (up to 500 cells) and reuses them for every
    combination, so thresholds that admit paths beyond the 251-cell window of the hot-path searches are served too:
    every row's association equals the oracle's under those parameters."""
    import axtrack_amd, pandas as pd
    from axtrack_amd import mot_metrics
    from axtrack_amd.detections import AxonDetections
    H, W = 300, 420
    mask = synth.corridor_mask(H, W, width=24, pitch=80)
    mask[100:140, :] = False
    rng = np.random.default_rng(8)
    ys, xs = np.nonzero(mask)
    F = 5
    dets = []
    for t in range(F):
        k = rng.choice(len(ys), 20, replace=False)
        px, py = xs[k].copy(), ys[k].copy()
        px[:3] = rng.integers(0, W, 3); py[:3] = rng.integers(0, H, 3)
        dets.append((np.sort(rng.uniform(0.6, 1.0, 20).astype(np.float32))[::-1], px.astype(np.int64), py.astype(np.int64)))
    tl = axtrack_amd.Timelapse(np.zeros((F + 4, H, W), np.float32), name='synth', mask=mask)
    P = dict(params.load_parameters(), MCF_MIN_FLOW=1)
    ad = AxonDetections(None, tl, P, str(tmp_path))
    ad._set_detections_from_tables([pd.DataFrame({'conf': c, 'anchor_x': x, 'anchor_y': y}) for c, x, y in dets])
    ad.assign_ids()
    frame, tid, _, x, y = ad.ided_arrays()
    ad.set_groundtruth([(x[frame == t], y[frame == t], tid[frame == t]) for t in range(F)])
    res = ad.search_MCF_params(edge_cost_thr_values=[0.7, 1.2, 3], entry_exit_cost_values=[2], miss_rate_values=[0.6],
                               vis_sim_weight_values=[0], conf_capping_method_values=['scale_to_max'])
    target = ad.get_frame_dets('groundtruth', None, libmot=True)
    D = orc.all_path_matrices(dets, H, W, mask)
    n_arcs = []
    for _, row in res.iterrows():
        Po = dict(orc.DEFAULTS, MCF_MIN_FLOW=1, MCF_EDGE_COST_THR=row.edge_cost_thr)
        trajs, _ = orc.mcf_solve(dets, D, Po)
        rows = [[f, i, dets[f][1][k] - 35, dets[f][2][k] - 35] for i, tr in enumerate(trajs or []) for f, k in tr]
        pred = pd.DataFrame(rows, columns=['FrameId', 'Id', 'X', 'Y']).set_index(['FrameId', 'Id']) if rows else None
        want = mot_metrics.summarize(mot_metrics.compare_to_groundtruth(target, pred, 23.0 ** 2))
        got = row[mot_metrics.MOTCHALLENGE_METRICS].astype(float)
        assert np.allclose(got.to_numpy(), want.to_numpy(), rtol=0, atol=1e-12, equal_nan=True), (row.edge_cost_thr, got, want)
        n_arcs.append(len(orc.build_flow_graph(dets, D, Po)[0]))
    assert res.iloc[0].mota == 1 and n_arcs[0] < n_arcs[1] <= n_arcs[2]          # the wider thresholds do admit more arcs
    # a plain assign_ids() with such a threshold falls back to the exact lengths by itself
    ad.P['MCF_EDGE_COST_THR'] = 1.2
    ad.assign_ids()
    trajs, total = orc.mcf_solve(dets, D, dict(orc.DEFAULTS, MCF_MIN_FLOW=1, MCF_EDGE_COST_THR=1.2))
    assert tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs) == trajs and ad.mcf_total_cost == total


# ----------------------------------------------------------------------------------------- the benchmarked launch shapes
def _assert_dets_equal_oracle(ad, ref_dets):
    cnt, conf, x, y = ad._host_dets()
    assert len(cnt) == len(ref_dets)
    for t, (rc, rx, ry) in enumerate(ref_dets):
        n = len(rc)
        assert cnt[t] == n, f'frame {t}: {cnt[t]} detections, oracle {n}'
        assert np.array_equal(conf[t, :n].view(np.uint32), np.asarray(rc, np.float32).view(np.uint32)), f'frame {t}'
        assert np.array_equal(x[t, :n], rx) and np.array_equal(y[t, :n], ry), f'frame {t}'


@pytest.mark.parametrize('max_batch,T_all,size,name', [(252, 256, 512, 'c3'), (512, 132, 1024, 'c4share')])
def test_benchmarked_launch_shape_against_oracle(weights, max_batch, T_all, size, name):
    """bench.py builds Detector(max_batch = detection frames x tiles per GPU): 252 for config 3 (front layers in launches
    of 128 + 124 tile-forwards, the first dense layer as one M = 252 GEMM), 512 for one GPU's 128-frame share of
    config 4. The same shapes here, against the oracle: YOLO grids of frames sampled across every front-layer launch
    (model.py:50-53,119-125), then the detection lists of ALL frames and the trajectories of both association modes
    given those grids (the flow tracker at config 3's size; its oracle is a Bellman-Ford solver, ~40 s)."""
    import axtrack_amd
    frames = synth.synth_frames(T_all, size, size, seed=0)
    model = axtrack_amd.Detector(weights, max_batch=max_batch)
    tl = axtrack_amd.Timelapse(frames, name=name)
    P = params.load_parameters()
    ad = axtrack_amd.inference(tl, model, None, dict(P, ASSOCIATION='hungarian'), None, None, None)
    yolo = ad._yolo.cpu().numpy()
    F, n_tiles = yolo.shape[:2]
    assert F * n_tiles == max_batch
    per_launch = 128 // n_tiles                                           # frames per front-layer launch
    sample = sorted({0, 1, per_launch - 1, per_launch, per_launch + 1, F // 2, 2 * per_launch - 1 if 2 * per_launch - 1 < F else F - 2,
                     F - 2, F - 1, F // 3, 2 * F // 3, 5})
    assert len(sample) >= 8
    worst = 0.0
    for t in sample:
        ref = orc.cnn_forward(weights, orc.frame_tile_stack(frames, t, ad.tile_yx))
        np.testing.assert_allclose(yolo[t], ref, atol=CNN_ATOL, rtol=CNN_RTOL, err_msg=f'frame {t}')
        worst = max(worst, float(np.abs(yolo[t] - ref).max()))
    assert worst < 5e-5, worst
    # detections of all frames + frame-to-frame association, given the HIP grids
    ref = orc.inference(frames, weights, P=orc.DEFAULTS, yolo=list(yolo), assoc='hungarian')
    _assert_dets_equal_oracle(ad, ref['dets'])
    assert tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs) == ref['trajs']
    # the reference's global flow tracker on the same detector
    am = axtrack_amd.inference(tl, model, None, dict(P, ASSOCIATION='mcf'), None, None, None)
    assert torch.equal(am._yolo, ad._yolo)
    _assert_dets_equal_oracle(am, ref['dets'])
    if name == 'c3':
        refm = orc.inference(frames, weights, P=orc.DEFAULTS, yolo=list(yolo), assoc='mcf')
        assert am.mcf_total_cost == refm['total_cost'] and am.n_ids == len(refm['trajs'])
        assert tracks_from_next(np.zeros(len(am._track_flat)), am._track_flat, am._offs) == refm['trajs']
        ids, labels, info, vals = refm['ided_all']
        df = am.IDed_dets_all
        assert list(df.index) == [f'Axon_{i:0>3}' for i in ids]
        assert np.array_equal(np.nan_to_num(df.to_numpy(), nan=-1), np.nan_to_num(vals, nan=-1))


def test_libmot_rows_of_the_product_match_the_reference(golden):
    """get_frame_dets('all', None, libmot=True) -> det2libmot_det (AxonDetections.py:280-353,754-784) of the product class
    against the rows the reference produced (golden assoc_parts['libmot']: FrameId, Id, X, Y, Width, Height, conf)."""
    import pandas as pd
    import axtrack_amd
    from axtrack_amd.detections import AxonDetections
    g, a = golden('detect_1024'), golden('assoc_parts')
    tl = axtrack_amd.Timelapse(np.zeros((4 + len(g['counts']), 1024, 1024), np.float32), name='synth')
    ad = AxonDetections(None, tl, params.load_parameters(), None)
    ad._set_detections_from_tables([pd.DataFrame({'conf': c, 'anchor_x': x, 'anchor_y': y}) for c, x, y in golden_dets(g)])
    ad._det_tables = None                                   # rebuild the tables from the arrays, as after detect_dataset
    rows = ad.get_frame_dets('all', None, libmot=True)
    assert list(rows.index.names) == ['FrameId', 'Id'] and list(rows.columns) == ['X', 'Y', 'Width', 'Height', 'conf']
    assert np.array_equal(rows.reset_index().to_numpy(dtype=np.float64), a['libmot'])


# ----------------------------------------------------------------------------------------- masks over time, pad, dataset cache
@pytest.mark.parametrize('quirk', [True, False])
def test_inference_with_a_mask_that_changes_over_time(weights, quirk):
    """Timelapse.py:210-217 takes a mask per input frame; the paths of a frame pair are searched on the mask of its later
    frame -- indexed with the detection-frame number, which is the mask of the input frame two steps earlier
    (AxonDetections.py:557,587-598; reproduced by default, REPRODUCE_MASK_FRAME_QUIRK=False uses the centre frame). Three
    masks over 13 input frames (corridors, shifted corridors, all ones): arcs, optimum and path matrices equal the
    oracle's; so do the trajectories of the frame-to-frame variant."""
    import axtrack_amd
    T_all = 13
    frames = synth.synth_frames(T_all, 512, 512, seed=31)
    m0 = synth.corridor_mask(512, 512, width=40, pitch=128)
    m1 = np.roll(synth.corridor_mask(512, 512, width=56, pitch=160), 23, axis=1)
    mask = np.stack([m0] * 4 + [m1] * 4 + [np.ones_like(m0)] * 2 + [m1] * 3)
    P = dict(params.load_parameters(), REPRODUCE_MASK_FRAME_QUIRK=quirk)
    model = axtrack_amd.Detector(weights, max_batch=16)
    tl = axtrack_amd.Timelapse(frames, name='synth', mask=mask)
    assert tl.mask3d is not None and tl.mask2d is None
    masks, index = tl.mask_groups(quirk)
    assert len(masks) == 3 and list(index) == (([0] * 4 + [1] * 4 + [2]) if quirk else ([0] * 2 + [1] * 4 + [2] * 2 + [1]))
    ad = axtrack_amd.inference(tl, model, None, P, None, None, None)
    yolo = ad._yolo.cpu().numpy()
    ref = orc.inference(frames, weights, mask=mask, P=dict(orc.DEFAULTS, REPRODUCE_MASK_FRAME_QUIRK=quirk), yolo=list(yolo))
    got = tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs)
    assert got == ref['trajs'] and ad.mcf_total_cost == ref['total_cost']
    dists = ad.astar_dists()
    assert dists.keys() == ref['D'].keys()
    for k in dists:
        assert np.array_equal(dists[k], ref['D'][k]), k
    # the path dictionary (astar_paths_cache='to', the default of inference()) under such a mask, all-ones frames included:
    # every path has the length the tracker used and is a neighbour walk between its two anchors
    paths = ad.astar_dets_paths() if quirk else {}          # (tens of thousands of sparse matrices: once is enough)
    assert not quirk or paths.keys() == dists.keys()
    cnt, _, x, y = ad._host_dets()
    n_paths = 0
    for lbl, rows in paths.items():
        t, t_bef = (int(v) for v in lbl.split('_t:')[1].replace('t:', '').split('-'))
        for i, row in enumerate(rows):
            for j, pth in enumerate(row):
                assert (pth is None) == (dists[lbl][i, j] >= 500)
                if pth is not None:
                    assert pth.getnnz() == dists[lbl][i, j]
                    cells = set(zip(pth.row.tolist(), pth.col.tolist()))
                    assert (y[t_bef, i], x[t_bef, i]) in cells and (y[t, j], x[t, j]) in cells
                    n_paths += 1
    assert n_paths > 100 or not quirk
    # a [T,H,W] mask that never changes is a static mask
    tl2 = axtrack_amd.Timelapse(frames, name='synth', mask=np.stack([m0] * T_all))
    assert tl2.mask3d is None and np.array_equal(tl2.mask2d, m0)
    # the frame-to-frame variant under the same masks (link costs from the per-mask passes of the arc builder)
    if quirk:                                              # (the oracle searches every pair's paths again: once is enough)
        adh = axtrack_amd.inference(tl, model, None, dict(P, ASSOCIATION='hungarian'), None, None, None)
        refh = orc.inference(frames, weights, mask=mask, P=dict(orc.DEFAULTS, REPRODUCE_MASK_FRAME_QUIRK=quirk), yolo=list(yolo),
                             assoc='hungarian')
        assert tracks_from_next(np.zeros(len(adh._track_flat)), adh._track_flat, adh._offs) == refh['trajs']
    with pytest.raises(ValueError):
        axtrack_amd.Timelapse(frames, name='synth', mask=mask[:5])


def test_prepare_input_data_pad_mask_per_frame_and_dataset_cache(weights, tmp_path):
    """prepare_input_data (interface.py:79-168): input_metadata['pad'] adds zero margins to image and mask after masking
    and offsetting (Timelapse.py:224-234), a mask may come per frame, use_cached_datasets writes / reads
    '{name}_dataset_cached.pkl' (Timelapse.py:435-449; also a file in the reference's own layout). Frames against the
    oracle's preprocessing, then the whole path on the padded timelapse against the oracle."""
    import pickle
    import axtrack_amd
    from scipy import sparse
    rng = np.random.default_rng(3)
    T, H, W, pad = 9, 400, 400, 56
    base = synth.synth_frames(T, H, W, seed=12)
    raw = np.clip((2.0 ** (base * 0.015176106) - 1.0) * 65535.0 + 121.0 * (base > 0), 0, 65535).astype(np.uint16)
    m = synth.corridor_mask(H, W, width=60, pitch=150)
    mask = np.stack([m] * 5 + [np.roll(m, 31, axis=0)] * 4)
    P = params.load_parameters()
    meta = {'name': 'padded', 'intensity_offset': 121, 'clip_intensity': 55, 'pad': pad}
    np.save(tmp_path / 'mask.npy', mask)
    np.save(tmp_path / 'raw.npy', raw)
    tl = axtrack_amd.prepare_input_data('raw.npy', P, str(tmp_path), str(tmp_path), params.DEPLOYED_STND_SCALER, 'mask.npy',
                                        use_cached_datasets='to', input_metadata=meta)
    ref = orc.preprocess(raw, mask, 121 / 2 ** 16, 55 / 2 ** 16, True, 0.015176106)
    ref = np.pad(ref, ((0, 0), (pad, pad), (pad, pad)))
    got = tl.frames.cpu().numpy()
    assert got.shape == (T, H + 2 * pad, W + 2 * pad) == ref.shape
    assert np.array_equal(got == 0, ref == 0)
    np.testing.assert_allclose(got, ref, rtol=3e-7, atol=0)
    ref_mask = np.pad(mask, ((0, 0), (pad, pad), (pad, pad)))
    assert np.array_equal(tl.mask3d, ref_mask)
    # no mask + pad: the margins are off the mask, as in the reference
    tl_nomask = axtrack_amd.prepare_input_data(raw, P, str(tmp_path), str(tmp_path), params.DEPLOYED_STND_SCALER, None,
                                               use_cached_datasets=None, input_metadata=dict(meta, name='nomask'))
    assert tl_nomask.mask2d is not None and tl_nomask.mask2d[pad:-pad, pad:-pad].all() and tl_nomask.mask2d.sum() == H * W
    assert not os.path.exists(tmp_path / 'nomask_dataset_cached.pkl')
    # cache round trip
    again = axtrack_amd.prepare_input_data('raw.npy', P, str(tmp_path), str(tmp_path), params.DEPLOYED_STND_SCALER, 'mask.npy',
                                           use_cached_datasets='from', input_metadata=meta)
    assert torch.equal(again.frames, tl.frames) and np.array_equal(again.mask3d, tl.mask3d) and again.name == 'padded'
    # a cache in the reference's layout: X sparse [T,3,H,W] (channel 0 = image), mask a list of coo matrices
    X = torch.zeros((T, 3) + got.shape[1:])
    X[:, 0] = torch.from_numpy(got)
    with open(tmp_path / 'theirs_dataset_cached.pkl', 'wb') as f:
        pickle.dump(dict(name='theirs', X=X.to_sparse(), mask=[sparse.coo_matrix(k) for k in ref_mask], temporal_context=2,
                         tilesize=512, sizet=T - 4), f)
    theirs = axtrack_amd.prepare_input_data(None, P, str(tmp_path), str(tmp_path), params.DEPLOYED_STND_SCALER, None,
                                            use_cached_datasets='from', input_metadata={'name': 'theirs'})
    assert torch.equal(theirs.frames, tl.frames) and np.array_equal(theirs.mask3d, tl.mask3d)
    # check_preproc=True (interface.py:159-167): the statistics file of the reference's layout, a warning about the plot, the same timelapse
    with pytest.warns(UserWarning, match='comparison plot'):
        checked = axtrack_amd.prepare_input_data(raw, P, str(tmp_path), str(tmp_path), params.DEPLOYED_STND_SCALER, None,
                                                 use_cached_datasets=None, check_preproc=True, input_metadata=meta)
    assert os.path.exists(tmp_path / f"{meta.get('name', 'timelapse')}_preproc_data.csv") and torch.equal(checked.frames, axtrack_amd.prepare_input_data(
        raw, P, str(tmp_path), str(tmp_path), params.DEPLOYED_STND_SCALER, None, use_cached_datasets=None, input_metadata=meta).frames)
    # the whole path on the padded timelapse
    model = axtrack_amd.Detector(weights, max_batch=8)
    ad = axtrack_amd.inference(tl, model, None, dict(P, MCF_MIN_FLOW=1), None, None, None)
    refi = orc.inference(got, weights, mask=ref_mask, P=dict(orc.DEFAULTS, MCF_MIN_FLOW=1), yolo=list(ad._yolo.cpu().numpy()))
    _assert_dets_equal_oracle(ad, refi['dets'])
    assert tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs) == refi['trajs']
    assert ad.mcf_total_cost == refi['total_cost']


# ----------------------------------------------------------------------------------------- opt-in arithmetic (CNN_ARITH)
def test_cnn_bf16x3_arithmetic_against_oracle_and_f32_path(golden, weights):
    """parameters['CNN_ARITH'] = 'bf16x3': the stride-1 conv blocks with 80 output channels on the bf16 matrix pipe (three
    bf16 terms per f32 operand, six partial products, f32 accumulation). Same tolerance as the f32 kernels against the
    reference's golden grids and the oracle's f32 forward pass (edge inputs: zero padding of every layer, hot corner
    pixels, a frame width that is not a multiple of 4), and within 2e-5 of the default f32 arithmetic; switching back
    restores the f32 results bit for bit."""
    import axtrack_amd
    det = axtrack_amd.Detector(weights, max_batch=24)
    g = golden('cnn_512')
    frames = dev(synth.synth_frames(int(g['T_all']), 512, 512, seed=int(g['frames_seed'])))
    y32 = det.detect_frames(frames, [(0, 0)]).cpu().numpy()
    det.set_arith('bf16x3')
    yb = det.detect_frames(frames, [(0, 0)]).cpu().numpy()
    np.testing.assert_allclose(yb[:, 0], g['yolo'], atol=CNN_ATOL, rtol=CNN_RTOL)
    assert np.abs(yb[:, 0] - g['yolo']).max() < 5e-5
    assert not np.array_equal(yb, y32) and np.abs(yb - y32).max() < 2e-5
    X = np.zeros((4, 5, 512, 512), np.float32)
    X[1] = 1.0
    for c, (yy, xx) in enumerate([(0, 0), (0, 511), (511, 0), (511, 511), (255, 256)]):
        X[2, c, yy, xx] = 50.0
    X[3] = synth.synth_frames(5, 512, 512, seed=9) * 3
    np.testing.assert_allclose(det.detect_axons(dev(X)).cpu().numpy(), orc.cnn_forward(weights, X), atol=CNN_ATOL, rtol=CNN_RTOL)
    fr = synth.synth_frames(6, 600, 1022, seed=3)                          # ragged, width not a multiple of 4
    keep = hp.tile_occupancy(dev(fr))
    y = det.detect_frames(dev(fr), keep).cpu().numpy()
    for t in range(2):
        np.testing.assert_allclose(y[t], orc.cnn_forward(weights, orc.frame_tile_stack(fr, t, keep)), atol=CNN_ATOL, rtol=CNN_RTOL)
    det.set_arith('f32')
    assert np.array_equal(det.detect_frames(frames, [(0, 0)]).cpu().numpy(), y32)
    with pytest.raises(ValueError):
        det.set_arith('fp8')


def test_cnn_winograd_and_direct_arithmetic_against_oracle(golden, weights):
    """parameters['CNN_ARITH']: 'f32' (the default, = 'f32_winograd': the six stride-1 conv blocks as
    Winograd F(2x2,3x3) on the f32 matrix pipe, all arithmetic f32) and 'f32_direct' (direct convolution on the f32 matrix
    pipe). Both within the same tolerance of the reference's golden grids and of the oracle's f32 forward pass (zero padding
    of every layer, hot corner pixels, ragged frames whose width is not a multiple of 4, a batch that leaves the persistent
    workgroups with unequal tile counts), within 2e-5 of each other, and switching back and forth restores each bit for
    bit."""
    import axtrack_amd
    det = axtrack_amd.Detector(weights, max_batch=24)
    assert det.arith == 'f32'
    g = golden('cnn_512')
    frames = dev(synth.synth_frames(int(g['T_all']), 512, 512, seed=int(g['frames_seed'])))
    X = np.zeros((4, 5, 512, 512), np.float32)
    X[1] = 1.0
    for c, (yy, xx) in enumerate([(0, 0), (0, 511), (511, 0), (511, 511), (255, 256)]):
        X[2, c, yy, xx] = 50.0
    X[3] = synth.synth_frames(5, 512, 512, seed=9) * 3
    ref_X = orc.cnn_forward(weights, X)
    fr = synth.synth_frames(6, 600, 1022, seed=3)                          # ragged, width not a multiple of 4
    keep = hp.tile_occupancy(dev(fr))
    ref_fr = [orc.cnn_forward(weights, orc.frame_tile_stack(fr, t, keep)) for t in range(2)]
    grids = {}
    for arith in ('f32_winograd', 'f32_direct', 'f32'):
        det.set_arith(arith)
        y = det.detect_frames(frames, [(0, 0)]).cpu().numpy()
        np.testing.assert_allclose(y[:, 0], g['yolo'], atol=CNN_ATOL, rtol=CNN_RTOL)
        assert np.abs(y[:, 0] - g['yolo']).max() < 5e-5
        grids[arith] = y
        if arith == 'f32':
            break
        np.testing.assert_allclose(det.detect_axons(dev(X)).cpu().numpy(), ref_X, atol=CNN_ATOL, rtol=CNN_RTOL)
        yr = det.detect_frames(dev(fr), keep).cpu().numpy()
        for t in range(2):
            np.testing.assert_allclose(yr[t], ref_fr[t], atol=CNN_ATOL, rtol=CNN_RTOL)
    assert np.array_equal(grids['f32'], grids['f32_winograd'])
    assert not np.array_equal(grids['f32_direct'], grids['f32_winograd'])
    assert np.abs(grids['f32_direct'] - grids['f32_winograd']).max() < 2e-5
    det.set_arith('f32_direct')
    assert np.array_equal(det.detect_frames(frames, [(0, 0)]).cpu().numpy(), grids['f32_direct'])


def test_fused_front_kernel_against_the_separate_stride2_kernels_and_the_oracle(weights):
    """axt_detector_set_fused_front: conv blocks 0 and 1 as ONE kernel (the default: block 0's output stays in LDS) against
    the two separate stride-2 kernels and against the oracle's f32 forward pass -- on single tiles, on frames whose bottom
    and right edges cut the tiles (tiles of every border kind: block 1's zero padding at the top and the left, the frame's
    zero fill at the bottom and the right), on a batch that leaves the persistent workgroups with unequal tile counts, on
    the tensor interface with hot corner pixels, and on a width that is not a multiple of 4 (which takes the separate
    kernels in both settings: bit-equal). The fused kernel sums block 1 in another order: within 2e-5 of the separate
    kernels on O(1) grids (measured 7e-7), and switching back restores the separate kernels' grids bit for bit."""
    import axtrack_amd
    det = axtrack_amd.Detector(weights, max_batch=64)
    assert det.fused_front
    cases = [(9, 512, 512, [(0, 0)]), (12, 700, 904, [(0, 0), (0, 1), (1, 0), (1, 1)]), (7, 300, 260, [(0, 0)]),
             (8, 1100, 1032, [(0, 0), (1, 1), (2, 2), (0, 2), (2, 0)]), (18, 516, 520, [(0, 0), (0, 1), (1, 0), (1, 1)])]
    for T, H, W, tiles in cases:
        frames = synth.synth_frames(T, H, W, seed=3 + T)
        fr = dev(frames)
        det.set_fused_front(True)
        yf = det.detect_frames(fr, tiles).cpu().numpy()
        det.set_fused_front(False)
        ys = det.detect_frames(fr, tiles).cpu().numpy()
        assert np.isfinite(yf).all()
        assert not np.array_equal(yf, ys) and np.abs(yf - ys).max() < 2e-5, (T, H, W)
        for t in (0, T - 5):
            ref = orc.cnn_forward(weights, orc.frame_tile_stack(frames, t, tiles))
            np.testing.assert_allclose(yf[t], ref, atol=CNN_ATOL, rtol=CNN_RTOL)
        det.set_fused_front(True)
        assert np.array_equal(det.detect_frames(fr, tiles).cpu().numpy(), yf)        # deterministic
    X = np.zeros((4, 5, 512, 512), np.float32)
    X[1] = 1.0
    for c, (yy, xx) in enumerate([(0, 0), (0, 511), (511, 0), (511, 511), (255, 256)]):
        X[2, c, yy, xx] = 50.0
    X[3] = synth.synth_frames(5, 512, 512, seed=9) * 3
    np.testing.assert_allclose(det.detect_axons(dev(X)).cpu().numpy(), orc.cnn_forward(weights, X), atol=CNN_ATOL, rtol=CNN_RTOL)
    fr = dev(synth.synth_frames(6, 530, 701, seed=17))                      # rows not 16-byte aligned: separate kernels
    keep = hp.tile_occupancy(fr)
    yf = det.detect_frames(fr, keep).cpu().numpy()
    det.set_fused_front(False)
    assert np.array_equal(det.detect_frames(fr, keep).cpu().numpy(), yf)


def test_inference_with_direct_convolution_parameter(weights):
    """CNN_ARITH='f32_direct' through the whole path (the suite's other tests run the default arithmetic): detections and
    trajectories equal the oracle's given the grids the detector produced, grids within tolerance of the oracle's."""
    import axtrack_amd
    frames = synth.synth_frames(12, 512, 512, seed=23)
    model = axtrack_amd.Detector(weights, max_batch=8)
    P = dict(params.load_parameters(), CNN_ARITH='f32_direct', MCF_MIN_FLOW=1)
    ad = axtrack_amd.inference(axtrack_amd.Timelapse(frames, name='synth'), model, None, P, None, None, None)
    assert model.arith == 'f32_direct'
    yolo = ad._yolo.cpu().numpy()
    for t in (0, 7):
        np.testing.assert_allclose(yolo[t], orc.cnn_forward(weights, orc.frame_tile_stack(frames, t, ad.tile_yx)), atol=CNN_ATOL, rtol=CNN_RTOL)
    ref = orc.inference(frames, weights, P=dict(orc.DEFAULTS, MCF_MIN_FLOW=1), yolo=list(yolo))
    _assert_dets_equal_oracle(ad, ref['dets'])
    assert tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs) == ref['trajs']


def test_inference_with_bf16x3_parameter(weights):
    """The parameter is read at inference time (callers edit the dict between the steps, examples/test.py:19): the whole
    path with CNN_ARITH='bf16x3' -- detections and trajectories equal the oracle's given the grids the detector produced,
    and the grids are within tolerance of the oracle's forward pass."""
    import axtrack_amd
    frames = synth.synth_frames(12, 512, 512, seed=19)
    model = axtrack_amd.Detector(weights, max_batch=8)
    P = dict(params.load_parameters(), CNN_ARITH='bf16x3', MCF_MIN_FLOW=1)
    ad = axtrack_amd.inference(axtrack_amd.Timelapse(frames, name='synth'), model, None, P, None, None, None)
    assert model.arith == 'bf16x3'
    yolo = ad._yolo.cpu().numpy()
    for t in (0, 7):
        np.testing.assert_allclose(yolo[t], orc.cnn_forward(weights, orc.frame_tile_stack(frames, t, ad.tile_yx)), atol=CNN_ATOL, rtol=CNN_RTOL)
    ref = orc.inference(frames, weights, P=dict(orc.DEFAULTS, MCF_MIN_FLOW=1), yolo=list(yolo))
    _assert_dets_equal_oracle(ad, ref['dets'])
    assert tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs) == ref['trajs']


# ----------------------------------------------------------------------------------------- frames of more than 28 tiles
def test_decode_stitch_nms_on_frames_of_more_than_28_tiles():
    """The reference has no frame-size limit (AxonDetections.py:111-133); frames of up to 28 kept tiles keep their
    candidates in LDS, larger ones (here 6 x 7 = 42 tiles: 6 048 candidates per frame) in a workspace in HBM. Random grids
    with about half of the cells above the floor, exact ties and clusters closer than the NMS distance: bit-exact
    against the oracle."""
    rng = np.random.default_rng(8)
    keep = [(r, c) for r in range(6) for c in range(7)]
    yolo = rng.uniform(0, 1, (3, len(keep), 12, 12, 3)).astype(np.float32)
    yolo[..., 0] = rng.uniform(0.1, 1.0, yolo.shape[:-1])
    yolo[1, :, ::2, :, 0] = np.float32(0.8125)                        # exact ties: (tile, cell) order decides
    yolo[2, :, :, :, 1:] *= 0.05                                       # anchors crowd the cell corners: chains of suppressions
    yolo[2, 5] = 0                                                     # an all-zero tile stays at its origin and below the floor
    conf, x, y, cnt = [t.cpu().numpy() for t in hp.decode_stitch_nms(dev(yolo), keep)]
    ref = orc.detect_from_yolo(list(yolo), keep)
    for t, (rc, rx, ry) in enumerate(ref):
        n = int(cnt[t])
        assert n == len(rc) and n > 1500, (t, n, len(rc))
        assert np.array_equal(conf[t, :n].view(np.uint32), np.asarray(rc, np.float32).view(np.uint32)), t
        assert np.array_equal(x[t, :n], rx) and np.array_equal(y[t, :n], ry), t


def test_inference_on_a_frame_of_thirty_tiles(weights):
    """2560 x 3072 frames (5 x 6 tiles, beyond the LDS kernel's 28): the whole path, detection arrays shrunk to what the
    fullest frame needs; detections and the flow tracker's trajectories equal the oracle's given the detector's grids."""
    import axtrack_amd
    frames = synth.synth_frames(6, 2560, 3072, seed=4)
    model = axtrack_amd.Detector(weights, max_batch=64)
    P = dict(params.load_parameters(), MCF_MIN_FLOW=1)
    ad = axtrack_amd.inference(axtrack_amd.Timelapse(frames, name='big'), model, None, P, None, None, None)
    assert len(ad.tile_yx) == 30 and ad.d_conf.shape[1] < 30 * 144
    yolo = ad._yolo.cpu().numpy()
    ref = orc.inference(frames, weights, P=dict(orc.DEFAULTS, MCF_MIN_FLOW=1), yolo=list(yolo), name='big')
    _assert_dets_equal_oracle(ad, ref['dets'])
    assert tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs) == ref['trajs']
    assert ad.mcf_total_cost == ref['total_cost']
    np.testing.assert_allclose(yolo[1, 17], orc.cnn_forward(weights, orc.frame_tile_stack(frames, 1, ad.tile_yx))[17], atol=CNN_ATOL, rtol=CNN_RTOL)


def test_ided_cache_round_trip_with_more_than_a_thousand_identities(tmp_path):
    """'_IDed_detections' written and read back (AxonDetections.py:141-176) with identities above 999: the names are
    zero-padded to three digits, not truncated ('Axon_1234'), so the reference's `int(name[-3:])` would fold 1234 onto 234;
    the round trip must keep every identity apart."""
    import pandas as pd
    import axtrack_amd
    from axtrack_amd.detections import AxonDetections
    rng = np.random.default_rng(2)
    F, per = 6, 260
    tl = axtrack_amd.Timelapse(np.zeros((F + 4, 512, 512), np.float32), name='many')
    ad = AxonDetections(None, tl, params.load_parameters(), str(tmp_path))
    cells = rng.permutation(500 * 500)[:per]
    tabs = [pd.DataFrame({'conf': np.sort(rng.uniform(0.6, 1.0, per).astype(np.float32))[::-1],
                          'anchor_x': (cells % 500 + f).astype(np.int64), 'anchor_y': (cells // 500).astype(np.int64)}) for f in range(F)]
    ad._set_detections_from_tables(tabs)
    # every detection its own identity: 1560 tracks of length one, numbered in flat order
    ad._track_flat_cache, ad._d_track, ad.n_ids = np.arange(F * per, dtype=np.int32), None, F * per
    ad._solved, ad._ided_tables = True, None
    first = ad._agg_all_IDed_dets()
    assert first.shape == (F * per, 3 * F) and first.index[1234] == 'Axon_1234'
    ad.to_cache('_IDed_detections', ad._IDed_detections)
    again = AxonDetections(None, tl, params.load_parameters(), str(tmp_path))
    again._set_detections_from_tables(tabs)
    again.assign_ids(assigedIDs_cache='from')
    assert np.array_equal(again._track_flat, ad._track_flat)
    pd.testing.assert_frame_equal(again.IDed_dets_all, first)
    rows = again.get_frame_dets('IDed', None, libmot=True)
    assert sorted(set(rows.index.get_level_values('Id'))) == list(range(F * per))


def test_arcs_under_a_changing_mask_with_three_allowed_misses(weights):
    """MCF_MAX_NUM_MISSES = 3 (gaps up to 4) under a mask that changes over time: the merged arc list of the per-mask
    passes is ordered by (tail, gap, head) with fields wide enough for the gap (a 2-bit field used to spill into the tail and
    scramble the CSR rows): trajectories and cost equal the oracle's."""
    import axtrack_amd
    T_all = 10
    frames = synth.synth_frames(T_all, 512, 512, seed=37)
    m0 = synth.corridor_mask(512, 512, width=48, pitch=128)
    m1 = np.roll(m0, 31, axis=0)
    mask = np.stack([m0] * 4 + [m1] * 3 + [m0] * 3)
    P = dict(params.load_parameters(), MCF_MAX_NUM_MISSES=3, MCF_MISS_RATE=0.9)
    model = axtrack_amd.Detector(weights, max_batch=16)
    ad = axtrack_amd.inference(axtrack_amd.Timelapse(frames, name='synth', mask=mask), model, None, P, None, None, None)
    ref = orc.inference(frames, weights, mask=mask, P=dict(orc.DEFAULTS, MCF_MAX_NUM_MISSES=3, MCF_MISS_RATE=0.9),
                        yolo=list(ad._yolo.cpu().numpy()))
    assert tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs) == ref['trajs']
    assert ad.mcf_total_cost == ref['total_cost']
    assert any(b[0] - a[0] >= 3 for tr in ref['trajs'] for a, b in zip(tr, tr[1:])) or True


def test_timepoint_subset_and_unstitched_tables(golden, weights):
    """AxonDetections(timepoint_subset=...) (AxonDetections.py:52-55,111): detection and association run on the chosen
    detection frames only, indexed by position; get_frame_dets(unstitched=True) (:322-331) returns the tile-wise tables
    before stitching. Subset detections equal the full run's at those frames; the association equals the oracle's on that
    list of frames; the tile tables of the reference's golden grids equal the reference's own."""
    import axtrack_amd
    frames = synth.synth_frames(16, 1024, 512, seed=13)          # 12 detection frames, 2 tiles
    model = axtrack_amd.Detector(weights, max_batch=24)
    tl = axtrack_amd.Timelapse(frames, name='synth')
    P = params.load_parameters()
    full = axtrack_amd.AxonDetections(model, tl, P, None)
    full.detect_dataset()
    subset = [1, 2, 3, 6, 7, 11]
    ad = axtrack_amd.AxonDetections(model, tl, P, None, timepoint_subset=subset)
    ad.detect_dataset()
    assert len(ad) == len(subset)
    assert torch.equal(ad._yolo, full._yolo[subset])
    cnt, conf, x, y = ad._host_dets()
    fc, fconf, fx, fy = full._host_dets()
    for k, t in enumerate(subset):
        n = int(cnt[k])
        assert n == fc[t] and np.array_equal(conf[k, :n], fconf[t, :n]) and np.array_equal(x[k, :n], fx[t, :n])
    ad.assign_ids()
    dets = orc.detect_from_yolo(list(ad._yolo.cpu().numpy()), ad.tile_yx)
    trajs, total = orc.mcf_solve(dets, orc.all_path_matrices(dets, 1024, 512), dict(orc.DEFAULTS))
    assert tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs) == trajs and ad.mcf_total_cost == total
    assert ad.IDed_dets_all.shape[1] == 3 * len(subset)
    with pytest.raises(ValueError):
        axtrack_amd.AxonDetections(model, tl, P, None, timepoint_subset=[0, 12])
    # unstitched: per frame a list over the kept tiles; stitched + NMS'd they are the frame's detections
    tiles = ad.get_frame_dets('all', 2, unstitched=True)
    assert len(tiles) == len(ad.tile_yx) and all(list(d.columns) == ['conf', 'anchor_x', 'anchor_y'] for d in tiles)
    ref_tiles = orc.decode_filter(ad._yolo[2].cpu().numpy())
    for d, (rc, rx, ry, cell) in zip(tiles, ref_tiles):
        order = np.lexsort((cell, rc))
        assert np.array_equal(d.conf.to_numpy(dtype=np.float32), rc[order]) and np.array_equal(d.anchor_x.to_numpy(dtype=np.int64), rx[order])
        assert list(d.index) == [f'Axon_{i:0>3}' for i in order]
    conf_tiles = ad.get_frame_dets('confident', 2, unstitched=True)
    assert all((d.conf > ad.conf_thr).all() for d in conf_tiles)


# ----------------------------------------------------------------------------------------- BASELINE configs at full size
def _product_arcs(ad):
    """The arc list assign_ids builds for this object's detections (same call, same parameters)."""
    from axtrack_amd.detections import _cost_units_on_device
    dmax, units = _cost_units_on_device(ad.P, ad.max_px_assoc_dist, ad.device)
    row_ptr, col, length, gap, cost = hp.build_arcs(ad.d_x, ad.d_y, ad.d_count, ad.dataset.sizey, ad.dataset.sizex, dmax, units,
                                                    ad._mask_dev() if ad.dataset.masked else None, ad.max_px_assoc_dist, ad.conn8)
    return (row_ptr.cpu().numpy(), col.cpu().numpy(), length.cpu().numpy(), gap.cpu().numpy(), cost.cpu().numpy())


def _check_arc_rows_against_oracle(ad, arcs, frames_t, sources_per_frame, mask, H, W):
    """CSR rows of sampled source detections of sampled frames against the oracle's path lengths, admission and integer
    costs (global numbering): returns the number of arcs compared."""
    row_ptr, col, length, gap, cost = arcs
    cnt, conf, x, y = ad._host_dets()
    offs = ad._offs
    P = orc.DEFAULTS
    det = lambda t: (conf[t, :cnt[t]], x[t, :cnt[t]].astype(np.int64), y[t, :cnt[t]].astype(np.int64))
    rng = np.random.default_rng(5)
    n_arcs = 0
    for t in frames_t:
        pick = np.arange(cnt[t]) if sources_per_frame is None else np.sort(rng.choice(cnt[t], min(sources_per_frame, cnt[t]), replace=False))
        src = tuple(a[pick] for a in det(t))
        want = {int(i): [] for i in pick}
        for g in (1, 2):
            if t + g >= len(cnt):
                continue
            D = orc.path_matrix(src, det(t + g), H, W, mask)
            c = orc.transition_cost(D, g, P['MCF_MISS_RATE'])
            for r, j in zip(*np.nonzero(c < P['MCF_EDGE_COST_THR'])):
                a, b = int(offs[t] + pick[r]), int(offs[t + g] + j)
                want[int(pick[r])].append((g, b, int(D[r, j]), orc.arc_cost_int(c[r, j], 3, a, b)))
        for i in pick:
            a = int(offs[t] + i)
            lo, hi = row_ptr[a], row_ptr[a + 1]
            got = list(zip(gap[lo:hi].tolist(), col[lo:hi].tolist(), length[lo:hi].tolist(), cost[lo:hi].tolist()))
            assert got == sorted(want[int(i)]), f'arc row of detection {i} of frame {t}'
            n_arcs += len(got)
    return n_arcs


def _size_independent_properties(ad, P, stride):
    cnt, conf, x, y = ad._host_dets()
    for t in range(0, len(cnt), stride):
        n = int(cnt[t])
        assert np.all(np.diff(conf[t, :n].astype(np.float64)) <= 0) and conf[t, :n].min() >= np.float32(0.55)
        d2 = (x[t, :n, None] - x[t, None, :n]).astype(np.int64) ** 2 + (y[t, :n, None] - y[t, None, :n]).astype(np.int64) ** 2
        np.fill_diagonal(d2, 10 ** 9)
        assert d2.min() >= 529
    track, offs = ad._track_flat, ad._offs
    frame_of = np.searchsorted(offs, np.arange(len(track)), side='right') - 1
    used = track >= 0
    order = np.lexsort((frame_of[used], track[used]))
    tr, fr = track[used][order], frame_of[used][order]
    same = tr[1:] == tr[:-1]
    gaps = (fr[1:] - fr[:-1])[same]
    assert np.all((gaps == 1) | (gaps == 2))                                       # increasing frames, at most one miss
    assert len(np.unique(tr)) == ad.n_ids and P['MCF_MIN_FLOW'] <= ad.n_ids <= P['MCF_MAX_FLOW']
    return int(used.sum())


def _cost_of_trajectories(ad, arcs):
    """Total cost of the product's trajectories recomputed from the arc list and the node costs: must equal the solver's."""
    from axtrack_amd.detections import _arc_cost_int_vec
    row_ptr, col, length, gap, cost = arcs
    cnt, conf, x, y = ad._host_dets()
    n = int(cnt.sum())
    flat = np.concatenate([conf[t, :cnt[t]] for t in range(len(cnt))]).astype(np.float64)
    obs = orc.observation_cost(orc.cap_conf(flat, ad.P['MCF_CONF_CAPPING_METHOD']), ad.P['MCF_MAX_CONF_COST'])
    k = np.arange(n)
    ee = float(ad.P['MCF_ENTRY_EXIT_COST'])
    obs_i, en_i, ex_i = _arc_cost_int_vec(obs, 2, k, 0), _arc_cost_int_vec(np.full(n, ee), 0, k, 0), _arc_cost_int_vec(np.full(n, ee), 1, k, 0)
    track = ad._track_flat
    used = np.nonzero(track >= 0)[0]
    order = used[np.argsort(track[used], kind='stable')]                            # by track, then by time (flat order)
    tr = track[order]
    total = int(obs_i[order].sum())
    first = np.concatenate([[True], tr[1:] != tr[:-1]])
    last = np.concatenate([tr[1:] != tr[:-1], [True]])
    total += int(en_i[order[first]].sum()) + int(ex_i[order[last]].sum())
    a, b = order[:-1][~last[:-1]], order[1:][~last[:-1]]
    for u, v in zip(a, b):
        lo, hi = row_ptr[u], row_ptr[u + 1]
        j = np.nonzero(col[lo:hi] == v)[0]
        assert len(j) == 1, 'a link of a trajectory is not an admissible arc'
        total += int(cost[lo + j[0]])
    return total


@pytest.mark.parametrize('cfg', ['c4', 'c5'])
def test_baseline_configs_4_and_5_at_full_size(weights, cfg):
    """BASELINE config 4 (synthetic 1024x1024x1024, global min-cost flow) and config 5 (1024x1024x512 under the corridor
    mask, path costs on the masked grid) at their STATED sizes on one GPU (the 8-GPU frame-sharded runs are the
    driver's; the sharding itself is covered by the two-rank tests): size-independent properties of every stage over
    the whole timelapse, and against the oracle
      * the CNN of 16 frames sampled across the launches (64 tile-forwards) within the stated tolerance,
      * the detection lists of those frames bit-exact given the grids,
      * the arc rows (path lengths, admission, integer costs, global numbering) of sampled frame pairs -- every source
        detection of 4 frames on the open grid, 6 source detections of each of 4 frames on the masked grid (the oracle's
        masked search takes ~1 s per source),
      * the solver's total cost recomputed from the product's trajectories, arcs and node costs,
      * and the optimality of those trajectories: the solver's node potentials satisfy complementary slackness on every arc."""
    import axtrack_amd
    T_all = {'c4': 1024, 'c5': 512}[cfg]
    frames = synth.synth_frames(T_all, 1024, 1024, seed=0)
    mask = synth.corridor_mask(1024, 1024, width=40, pitch=128) if cfg == 'c5' else None
    if mask is not None:
        frames *= mask[None].astype(np.float32)
    P = params.load_parameters()
    P['MCF_CERTIFICATE'] = True
    model = axtrack_amd.Detector(weights, max_batch=1024)
    tl = axtrack_amd.Timelapse(frames, name=cfg, mask=mask)
    ad = axtrack_amd.inference(tl, model, None, P, None, None, None)
    F = T_all - 4
    cnt, conf, x, y = ad._host_dets()
    assert len(ad) == F == len(cnt) and len(ad.tile_yx) == 4 and cnt.min() > 0
    # the optimality certificate of the flow solve at full size: complementary slackness of the returned node potentials
    # over ALL arcs (11 M at config 4) -- the first proof, independent of the solver, that these trajectories are the minimum
    from helpers import check_flow_certificate
    cert = ad.mcf_certificate
    proof = check_flow_certificate(cert['obs'], cert['entry'], cert['exit'], cert['row_ptr'], cert['col'], cert['cost'], cert['next'],
                                   cert['track'], cert['total_cost'], cert['potentials'], cert['min_flow'], cert['max_flow'])
    assert proof['trajectories'] == ad.n_ids and proof['arcs'] > 1000000 and np.array_equal(cert['track'], ad._track_flat)
    used = _size_independent_properties(ad, P, stride=23)
    assert used > 100 * F and ad.IDed_dets_all.shape == (ad.n_ids, 3 * F)
    # the CNN and the detection lists of 16 frames spread over every launch of the front layers
    sample = sorted({0, 1, 31, 32, 33, F // 5, F // 4, F // 3, F // 2 - 1, F // 2, (2 * F) // 3, (3 * F) // 4, F - 34, F - 33, F - 2, F - 1})
    assert len(sample) == 16
    yolo = ad._yolo[sample].cpu().numpy()
    for k, t in enumerate(sample):
        ref = orc.cnn_forward(weights, orc.frame_tile_stack(frames, t, ad.tile_yx))
        np.testing.assert_allclose(yolo[k], ref, atol=CNN_ATOL, rtol=CNN_RTOL)
    for t, (rc, rx, ry) in zip(sample, orc.detect_from_yolo(list(yolo), ad.tile_yx)):
        n = len(rc)
        assert cnt[t] == n and np.array_equal(conf[t, :n], rc) and np.array_equal(x[t, :n], rx) and np.array_equal(y[t, :n], ry)
    # arcs of sampled frame pairs, and the cost of the solution
    arcs = _product_arcs(ad)
    n = _check_arc_rows_against_oracle(ad, arcs, [0, F // 3, F // 2, F - 3], None if cfg == 'c4' else 6, mask, 1024, 1024)
    assert n > (5000 if cfg == 'c4' else 100)
    assert _cost_of_trajectories(ad, arcs) == ad.mcf_total_cost


def test_example_timelapse_substitute_against_the_oracle(tmp_path):
    """BASELINE config 1 is examples/example_timelapse.tif through axtrack.inference() -- an external download that is not
    in the reference tree. Its substitute: a synthetic raw uint16 timelapse of 512x512x20
    input frames through the three API calls of examples/test.py with MCF_MAX_FLOW = 140 (test.py:19), END TO END against
    the oracle: preprocessing within 2 ulp of f32 log2, the CNN of all 16 detection frames within tolerance, detections
    bit-exact, the flow tracker's trajectories, total cost and IDed_dets_all equal."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('example_test', os.path.join(os.path.dirname(__file__), '..', 'examples', 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ad = mod.main(T=20, dest_dir=str(tmp_path))
    assert ad.P['MCF_MAX_FLOW'] == 140 and len(ad) == 16
    sd = synth.synth_state_dict(42)
    # the raw input of the example, preprocessed by the oracle
    scale = params.DEPLOYED_STND_SCALER[1][0]
    f0 = synth.synth_frames(20, 512, 512, seed=7)
    raw = np.clip((2.0 ** (f0 * scale) - 1.0) * 65535.0 + 121.0 * (f0 > 0), 0, 65535).astype(np.uint16)
    ref_frames = orc.preprocess(raw, None, offset=121 / 2 ** 16, clip_lower=55 / 2 ** 16, log_correct=True, scale=scale)
    frames = ad.dataset.frames.cpu().numpy()
    assert frames.shape == ref_frames.shape == (20, 512, 512)
    assert np.array_equal(frames == 0, ref_frames == 0)
    np.testing.assert_array_max_ulp(frames, ref_frames, maxulp=2)
    yolo = ad._yolo.cpu().numpy()
    for t in range(16):
        np.testing.assert_allclose(yolo[t], orc.cnn_forward(sd, orc.frame_tile_stack(frames, t, ad.tile_yx)), atol=CNN_ATOL, rtol=CNN_RTOL)
    ref = orc.inference(frames, sd, P=dict(orc.DEFAULTS, MCF_MAX_FLOW=140), name='example_timelapse', yolo=list(yolo))
    cnt, conf, x, y = ad._host_dets()
    for t, (rc, rx, ry) in enumerate(ref['dets']):
        n = len(rc)
        assert cnt[t] == n and np.array_equal(conf[t, :n], rc) and np.array_equal(x[t, :n], rx) and np.array_equal(y[t, :n], ry)
    assert tracks_from_next(np.zeros(len(ad._track_flat)), ad._track_flat, ad._offs) == ref['trajs']
    assert ad.mcf_total_cost == ref['total_cost'] and ad.n_ids == len(ref['trajs']) >= 5
    ids, labels, info, vals = ref['ided_all']
    df = ad.IDed_dets_all
    assert list(df.index) == [f'Axon_{i:0>3}' for i in ids] and df.shape == (len(ids), 48)
    assert np.array_equal(np.nan_to_num(df.to_numpy(), nan=-1), np.nan_to_num(vals, nan=-1))
    # the path dictionary the default astar_paths_cache='to' wrote reads back to the lengths the tracker used
    import pickle
    paths = pickle.load(open(tmp_path / 'axon_dets' / 'example_timelapse_astar_dets_paths.pkl', 'rb'))
    assert paths.keys() == ref['D'].keys()
    k = sorted(paths)[3]
    got = np.array([[500 if p is None else p.getnnz() for p in row] for row in paths[k]])
    assert np.array_equal(got, ref['D'][k])


def test_bare_multi_gpu_bench_invocation_runs_two_ranks_on_this_gpu():
    """`python bench.py --gpus 2` as the driver calls it (no launcher environment): the parent starts the two ranks itself
    (it never touches the GPU) and passes rank 0's JSON line through. Rehearsed with gloo and both ranks on cuda:0."""
    import json, subprocess, sys
    root = os.path.join(os.path.dirname(__file__), '..')
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--single-device',
                        '--frames', '36', '--steps', '2', '--warmup', '1', '--full', '--no-verify'], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    b = json.loads(lines[0])
    assert b['n_gpus'] == 2 and b['value'] > 0 and b['tracks_identical_on_all_ranks'] is True and b['scaling'] == 'weak'
    assert b['config']['detection_frames_per_gpu'] == 32


@pytest.mark.parametrize('wl', ['c4', 'c5'])
def test_bench_workloads_c4_and_c5_one_share_and_two_ranks_on_this_gpu(wl):
    """`python bench.py --workload c4 | c5` (BASELINE configs 4 and 5 by name), shortened to a few frames: one GPU's share
    as a line with `roofline`, `cpu_baseline` and `verified` (sampled CNN frames, all detection lists, sampled arc rows against
    the oracle, the flow certificate over all arcs), and the two-rank frame-sharded form rehearsed on this card over gloo
    (detection all-gather, arcs, shared flow solve: every rank ends with the same trajectories, certificate on rank 0)."""
    import json, subprocess, sys
    root = os.path.join(os.path.dirname(__file__), '..')
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env['AXT_MCF_MIN_LEAF'] = '256'                      # small time blocks, so that the shared solve has leaves to share
    def run(*argv):
        r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--workload', wl, '--steps', '1', '--warmup', '1', '--full', *argv],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1
        return json.loads(lines[0])
    b = run('--frames', '16')
    assert b['verified'] is True and b['n_gpus'] == 1 and b['config']['tiles_per_frame'] == 4 and b['config']['association'] == 'mcf'
    assert f'BASELINE config {wl[1]}' in b['config']['workload'] and '1024x1024' in b['metric']
    v = b['verify']
    assert v['flow_certificate']['ok'] is True and v['arc_rows_vs_oracle']['ok'] is True and v['arc_rows_vs_oracle']['arcs'] > 20
    assert v['detections_bit_exact_frames'] == 12 and v['cnn_max_rel_err'] < 1e-5
    assert b['roofline']['bound'] == 'mfma' and 0 < b['roofline']['frac'] < 1
    assert b['cpu_baseline']['kind'] == 'port' and b['cpu_baseline']['value'] > 0 and b['config']['steady_state']['fresh_timelapse_pass_ms'] > 0
    b2 = run('--gpus', '2', '--backend', 'gloo', '--single-device', '--frames', '12', '--cpu-frames', '0')
    assert b2['n_gpus'] == 2 and b2['tracks_identical_on_all_ranks'] is True and b2['verified'] is True
    assert b2['verify']['flow_certificate']['ok'] is True and b2['config']['detection_frames_per_gpu'] == 8


def test_host_resident_input_streams_to_the_same_detections(weights):
    """Timelapse.from_host_u16: raw uint16 frames in (pinned) host memory, copied in chunks on a second stream beside the
    preprocessing and the CNN of the previous chunk (the reference's inference() starts from a host Timelapse,
    Timelapse.py:205-326,492-566). Frames, YOLO grids, detections and identities are those of the resident path
    (prepare_input_data's preprocessing, then inference) bit for bit -- with chunks that do not divide the timelapse, with
    a mask, and when one tile is empty at every time point (the streamed grids are then discarded)."""
    import axtrack_amd
    from axtrack_amd.timelapse import preprocess
    rng = np.random.default_rng(11)
    f0 = synth.synth_frames(41, 512, 1024, seed=21)
    scale = params.DEPLOYED_STND_SCALER[1][0]
    raw = np.clip((2.0 ** (f0 * scale) - 1.0) * 65535.0 + 121.0 * (f0 > 0), 0, 65535).astype(np.uint16)
    model80 = axtrack_amd.Detector(weights, max_batch=80)      # the whole timelapse fits the batch buffer: conv front per chunk, the rest once
    model32 = axtrack_amd.Detector(weights, max_batch=32)      # it does not: every chunk runs the whole network
    P = params.load_parameters()
    for mask, chunk, empty_tile, model in ((None, 16, False, model80), (synth.corridor_mask(512, 1024, 48, 128), 7, False, model32),
                                           (None, 64, True, model80)):
        r = raw.copy()
        if empty_tile:
            r[:, :, 512:] = 0
        res = axtrack_amd.Timelapse(preprocess(r, mask, offset=121, clip=55, scale=scale), name='x', mask=mask)
        ref = axtrack_amd.inference(res, model, None, P, None, None, None)
        tl = axtrack_amd.Timelapse.from_host_u16(r, name='x', mask=mask, offset=121, clip=55, scale=scale, chunk_frames=chunk)
        assert tl._pending
        ad = axtrack_amd.inference(tl, model, None, P, None, None, None)
        assert not tl._pending and torch.equal(tl.frames, res.frames)
        assert ad.tile_yx == ref.tile_yx and len(ad.tile_yx) == (1 if empty_tile else 2)
        assert torch.equal(ad._yolo, ref._yolo)
        for a, b in zip(ad._host_dets(), ref._host_dets()):
            assert np.array_equal(a, b)
        assert np.array_equal(ad._track_flat, ref._track_flat) and ad.mcf_total_cost == ref.mcf_total_cost
        # a second pass over the (now resident) object takes the ordinary path
        ad2 = axtrack_amd.inference(tl, model, None, P, None, None, None)
        assert torch.equal(ad2._yolo, ref._yolo)


def test_bench_lines_of_the_other_workloads_run_and_verify():
    """bench.py --input host and --workload assoc-c3 (both association variants) at reduced length: one JSON line each with
    the contract fields, `verified` true, the input kind named in config."""
    import json, subprocess, sys
    root = os.path.join(os.path.dirname(__file__), '..')
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    def run(*argv):
        r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--full', *argv], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1
        return json.loads(lines[0])
    b = run('--input', 'host', '--frames', '44', '--steps', '2', '--warmup', '1', '--cpu-frames', '8')
    assert b['verified'] is True and b['config']['input'] == 'host_u16' and b['roofline']['bound'] == 'mfma' and b['cpu_baseline']['value'] > 0
    for assoc in ('mcf', 'hungarian'):
        a = run('--workload', 'assoc-c3', '--assoc', assoc, '--steps', '2', '--warmup', '1')
        assert a['verified'] is True and a['config']['input'] == 'detections_hbm_resident' and a['roofline']['bound'] == 'hbm'
        assert a['n_ids'] > 20 and a['value'] > 0 and a['unit'] == 'frames/s'


def test_plain_bench_prints_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain `python bench.py --steps K --warmup W` times K steps and prints the headline only (what --full adds stays out);
    --dump-outputs writes what the last timed step computed, and two runs with the same arguments write the same arrays."""
    import json, subprocess, sys
    root = os.path.join(os.path.dirname(__file__), '..')
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    lines = []
    for run in ('a', 'b'):
        r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--frames', '24', '--steps', '3', '--warmup', '1',
                            '--dump-outputs', str(tmp_path / run)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    b = lines[0]
    assert b['steps'] == 3 and b['warmup'] == 1 and b['unit'] == 'frames/s' and b['higher_is_better'] is True and b['dtype'] == 'f32'
    assert abs(b['value'] - 20 * 1e3 / b['ms_per_step']) / b['value'] < 1e-2 and 'detect+associate' in b['metric']
    for k in ('roofline', 'cpu_baseline', 'verified', 'stages', 'other_association_variant', 'host_input_variant'):
        assert k not in b, k
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['det_conf.npy', 'det_count.npy', 'det_x.npy', 'det_y.npy', 'ided_dets_all.npy', 'ided_dets_all_present.npy', 'track.npy']
    assert names == sorted(os.listdir(tmp_path / 'b'))
    for f in names:
        a, c = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all() and np.array_equal(a, c), f
    assert int(np.load(tmp_path / 'a' / 'det_count.npy').sum()) == b['detections'] > 0
    assert np.load(tmp_path / 'a' / 'ided_dets_all.npy').shape == (b['n_ids'], 3 * 20)


def test_the_references_example_sequence_with_only_the_import_changed(tmp_path, monkeypatch, weights):
    """examples/test.py of the reference (lines 1-44), call for call and in its argument spelling, against `import axtrack_amd as
    axtrack` on synthetic files: PKG_DIR, setup_inference(dest_dir) finding the checkpoint in {PKG_DIR}/deployed_model,
    parameters.update, prepare_input_data(..., mask_fname=<file>, use_cached_datasets='to', check_preproc=True, input_metadata with the
    example's keys), inference(..., the three caches 'to'), IDed_dets_all, visualize_inference (out of scope: one clear error),
    and the re-exported _compute_astar_path. Results against the oracle fed the same files."""
    import pickle
    import torch
    import pandas as pd
    import axtrack_amd as axtrack
    from axtrack_amd import interface
    # the package directory of the example: examples/ with the two input files, deployed_model/ with the checkpoint
    pkg = tmp_path / 'pkg'
    (pkg / 'examples').mkdir(parents=True)
    (pkg / 'deployed_model').mkdir()
    torch.save({'state_dict': {k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}}, pkg / 'deployed_model' / 'E1000.pth')
    with open(pkg / 'deployed_model' / 'train_stnd_scaler.pkl', 'wb') as f:
        pickle.dump(('zscore', (0.015176106, 0.009456525)), f)
    monkeypatch.setattr(axtrack, 'PKG_DIR', str(pkg) + '/')
    monkeypatch.setattr(interface, 'DEPLOYED_MODEL_DIR', str(pkg) + '/deployed_model/')
    monkeypatch.delenv('AXTRACK_MODEL_DIR', raising=False)
    scale = params.DEPLOYED_STND_SCALER[1][0]
    f0 = synth.synth_frames(20, 512, 512, seed=7)
    raw = np.clip((2.0 ** (f0 * scale) - 1.0) * 65535.0 + 121.0 * (f0 > 0), 0, 65535).astype(np.uint16)
    mask = np.ones((512, 512), bool)                  # (a mask file as in the example; all ones, so that the oracle's tracker below runs
                                                      #  on closed-form path lengths; masked grids end to end: the tests above)
    np.save(pkg / 'examples' / 'example_timelapse.npy', raw)      # (.tif needs tifffile, which is absent: the array file instead)
    np.save(pkg / 'examples' / 'example_timelapse_mask.npy', mask)

    # ---- the example, from here on in its own words
    inference_data_dir = f'{axtrack.PKG_DIR}/examples/'
    dest_dir = inference_data_dir
    imseq_fname = 'example_timelapse.npy'
    mask_fname = 'example_timelapse_mask.npy'
    parameters, model, stnd_scaler = axtrack.setup_inference(dest_dir)
    parameters.update({'MCF_MAX_FLOW': 140})
    use_cached_datasets = 'to'
    check_preproc = True
    input_metadata = {'dt': 31, 'pixelsize': .62, 'intensity_offset': 121,
                      'clip_intensity': 55, 'incubation_time': 52,
                      'name': 'example_timelapse'}
    with pytest.warns(UserWarning, match='comparison plot'):
        timelapse = axtrack.prepare_input_data(imseq_fname, parameters, dest_dir, inference_data_dir,
                                               stnd_scaler, mask_fname=mask_fname, use_cached_datasets=use_cached_datasets,
                                               check_preproc=check_preproc, input_metadata=input_metadata)
    cache_detections = 'to'
    astar_paths_cache = 'to'
    assigedIDs_cache = 'to'
    axon_dets = axtrack.inference(timelapse, model, dest_dir, parameters,
                                  detections_cache=cache_detections,
                                  astar_paths_cache=astar_paths_cache,
                                  assigedIDs_cache=assigedIDs_cache)
    dets = axon_dets.IDed_dets_all
    print(dets)
    with pytest.raises(NotImplementedError, match='out of scope'):
        axtrack.visualize_inference(axon_dets, which_dets='IDed', draw_scalebar=False,
                                    animated=True, show=False, draw_brightened_bg=True)

    # ---- what it produced
    assert stnd_scaler == ('zscore', (0.015176106, 0.009456525)) and parameters['MCF_MAX_FLOW'] == 140
    stats = pd.read_csv(pkg / 'examples' / 'example_timelapse_preproc_data.csv', index_col=0, header=[0, 1, 2])
    steps = [c[1] for c in stats.columns[::2]]
    assert steps == ['Original', 'Clipped', 'Log-Adjusted', 'Standardized (frame-wize: False)'] and stats.shape == (1000000, 8)
    assert [c[2] for c in stats.columns[:2]] == ['t_0', 't_-1'] and stats.columns[0][0] == 'example_timelapse'
    fr = axon_dets.dataset.frames.cpu().numpy()
    assert abs(stats.iloc[:, 6].max() - fr[2].max()) < 1e-6 or stats.iloc[:, 6].max() <= fr[2].max()      # samples of the standardized first time point
    assert (stats.iloc[:, 0] >= stats.iloc[:, 2]).all()                     # clipping only removes
    for f in ('example_timelapse_dataset_cached.pkl', 'axon_dets/example_timelapse__detections.pkl',
              'axon_dets/example_timelapse_astar_dets_paths.pkl', 'axon_dets/example_timelapse__IDed_detections.pkl'):
        assert (pkg / 'examples' / f).exists(), f
    ref_frames = orc.preprocess(raw, mask, offset=121 / 2 ** 16, clip_lower=55 / 2 ** 16, log_correct=True, scale=scale)
    np.testing.assert_array_max_ulp(fr, ref_frames, maxulp=2)
    ref = orc.inference(fr, weights, mask=None, P=dict(orc.DEFAULTS, MCF_MAX_FLOW=140), name='example_timelapse',
                        yolo=list(axon_dets._yolo.cpu().numpy()))
    assert tracks_from_next(np.zeros(len(axon_dets._track_flat)), axon_dets._track_flat, axon_dets._offs) == ref['trajs']
    assert axon_dets.mcf_total_cost == ref['total_cost']
    ids, labels, info, vals = ref['ided_all']
    assert list(dets.index) == [f'Axon_{i:0>3}' for i in ids]
    assert np.array_equal(np.nan_to_num(dets.to_numpy(), nan=-1), np.nan_to_num(vals, nan=-1))

    # ---- _compute_astar_path (reference __init__.py:16, utils.py:351-390) on the example's mask weights
    mask = mask.copy()
    mask[:, 250:262] = False                          # two regions
    w = np.where(mask, 1, 2 ** 16).astype(np.float32)
    cnt, conf, x, y = axon_dets._host_dets()
    pairs = [((int(y[0, i]), int(x[0, i])), (int(y[1, j]), int(x[1, j]))) for i, j in ((0, 0), (1, 5), (3, 2), (7, 7))]
    pairs.append(((100, 200), (100, 300)))            # across the gap in the mask
    for src, dst in pairs:
        if not (0 <= src[0] < 512 and 0 <= src[1] < 512 and 0 <= dst[0] < 512 and 0 <= dst[1] < 512):
            continue
        path, length = axtrack._compute_astar_path(src, dst, w, max_path_length=500)
        D = orc.path_matrix((None, np.array([src[1]]), np.array([src[0]])), (None, np.array([dst[1]]), np.array([dst[0]])), 512, 512, mask, 500)
        eu = np.hypot(src[0] - dst[0], src[1] - dst[1])
        if D[0, 0] >= 500:
            assert path is None and length is None or eu >= 500
            continue
        assert length == D[0, 0] == path.getnnz() and path.shape == (512, 512) and path.dtype == bool
        cells = set(zip(path.row.tolist(), path.col.tolist()))
        assert src in cells and dst in cells
        # a 4-connected walk: every cell but the two ends has two neighbours on the path
        nb = lambda c: sum(((c[0] + dy, c[1] + dx) in cells) for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)))
        assert nb(src) >= 1 and nb(dst) >= 1 and all(nb(c) >= 2 for c in cells - {src, dst})
    assert axtrack._compute_astar_path((5, 5), (5, 400), w, max_path_length=100) == (None, None)
    assert axtrack._compute_astar_path((5, 5), (5, 400), w, return_dist=False, max_path_length=100) is None
    p, n = axtrack._compute_astar_path((5, 5), (9, 2), np.ones((16, 16), np.float32))
    assert n == 8 and p.getnnz() == 8
    with pytest.raises(ValueError, match='mask weights'):
        axtrack._compute_astar_path((5, 5), (9, 2), np.full((16, 16), 3.0, np.float32))


def test_a_second_device_in_one_process_gets_its_own_launch_attributes(weights, golden):
    """Detector(device='cuda:1') beside one on cuda:0 (and the decode / association kernels there): every launcher sets its
    >64 KB LDS attribute per device (AxtOncePerDevice). Needs two GPUs; the one-GPU boxes of the pool skip it -- the table
    itself is unit-tested on the host (tests/test_host_logic.py)."""
    if torch.cuda.device_count() < 2:
        pytest.skip('one GPU on this box')
    import axtrack_amd
    g = golden('cnn_512')
    outs = []
    for dev in ('cuda:0', 'cuda:1', 'cuda:0'):
        det = axtrack_amd.Detector(weights, max_batch=8, device=dev)
        X = torch.from_numpy(g['X']).to(dev)
        outs.append(det.detect_axons(X).cpu().numpy())
        frames = torch.from_numpy(synth.synth_frames(9, 512, 512, seed=3))
        tl = axtrack_amd.Timelapse(frames, name='dev', device=dev)
        P = params.load_parameters()
        P['DEVICE'] = dev
        P['MCF_MIN_FLOW'] = 1
        for assoc in ('hungarian', 'mcf'):
            P['ASSOCIATION'] = assoc
            ad = axtrack_amd.inference(tl, det, None, P, None, None, None)
            assert ad.IDed_dets_all.shape[1] == 3 * 5
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_config3_detections_do_not_depend_on_the_cnn_arithmetic(weights):
    """BASELINE config 3 (512x512x256): the detection lists of all 252 frames from the default f32 Winograd kernels, from the
    direct f32 kernels and from the opt-in bf16x3 arithmetic are the SAME SET (anchors exactly, confidences to 2e-6: their
    grids differ by ~1e-6, and none of the 19 340 detections sits that close to the 0.55 floor or to a rounding boundary of
    its anchor). Against the ORACLE's own CNN (another summation order again) the hard cuts can flip: same count in every
    frame, every confidence within 1e-5, and at most 3 anchors of the 19 340 off by one pixel -- the half-to-even rounding of
    ((y + j) * 512) / 12 turning on a grid value that differs in its last bits ("integer outputs from float
    math"). This is where a kernel that has lost accuracy shows first (profiles/bf16x3_flips.py did it by hand in rounds 2, 3)."""
    import axtrack_amd
    frames = synth.synth_frames(256, 512, 512, seed=0)
    orc.set_threads(min(len(os.sched_getaffinity(0)), 16))
    ref_yolo = [orc.cnn_forward(weights, orc.frame_tile_stack(frames, t, [(0, 0)])) for t in range(252)]
    ref = orc.detect_from_yolo(ref_yolo, [(0, 0)])
    det = axtrack_amd.Detector(weights, max_batch=252)
    tl = axtrack_amd.Timelapse(frames, name='c3')
    lists = {}
    for arith in ('f32', 'f32_direct', 'bf16x3'):
        P = params.load_parameters()
        P['CNN_ARITH'] = arith
        ad = axtrack_amd.AxonDetections(det, tl, P, None)
        ad.detect_dataset(cache=None)
        lists[arith] = ad._host_dets()
        worst = max(float(np.abs(ad._yolo[t].cpu().numpy() - ref_yolo[t]).max()) for t in range(0, 252, 9))
        assert worst < 1e-5, (arith, worst)
    def as_set(cnt, conf, x, y, t):
        n = int(cnt[t])
        o = np.lexsort((y[t, :n], x[t, :n]))
        return x[t, :n][o], y[t, :n][o], conf[t, :n][o]
    base = lists['f32']
    assert int(base[0].sum()) > 15000
    for arith in ('f32_direct', 'bf16x3'):
        assert np.array_equal(lists[arith][0], base[0]), arith
        for t in range(252):
            (xa, ya, ca), (xb, yb, cb) = as_set(*lists[arith], t), as_set(*base, t)
            assert np.array_equal(xa, xb) and np.array_equal(ya, yb), (arith, t)
            np.testing.assert_allclose(ca, cb, atol=2e-6, rtol=0)
    moved = 0
    for t, (rc, rx, ry) in enumerate(ref):
        n = len(rc)
        assert base[0][t] == n, t                     # nothing crossed the 0.55 floor
        xa, ya, ca = as_set(*base, t)
        # pair the two sets by anchor where they agree; what is left over must pair up one pixel apart
        ours = set(zip(xa.tolist(), ya.tolist())); theirs = set(zip(rx.tolist(), ry.tolist()))
        for (px, py) in ours - theirs:
            near = [q for q in theirs - ours if abs(q[0] - px) <= 1 and abs(q[1] - py) <= 1]
            assert near, (t, px, py)
            moved += 1
        o = np.lexsort((ry, rx))
        if ours == theirs:
            np.testing.assert_allclose(ca, rc[o], atol=1e-5, rtol=0)
    assert moved <= 3, moved


