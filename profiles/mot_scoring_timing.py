"""Time the tracking scores of one association on the device against the host path they replace in
search_MCF_params, in one process on one GPU, on a synthetic scene of config-3 size (252 frames, about 40
labels and detections per frame):

  (a) the host path of one combination     get_frame_dets('IDed', None, libmot=True) from the association's arrays,
                                           mot_metrics.compare_to_groundtruth, mot_metrics.summarize (the label table is
                                           built once outside, as the search does)
  (b) get_tracking_metrics()               axt_mot_scores with K = 1, the scores as a pd.Series
  (c) score_associations, K = 64           64 different track tables of the scene in one call; reported per association
  (d) assign_ids()                         the solve that precedes every scoring in the search, for scale

Medians of `--runs` timed runs (wall clock around a device synchronisation) after `--warmup` untimed ones. The yardstick
is (a), taken in the same run. Prints one JSON line.

    python profiles/mot_scoring_timing.py [--frames 252] [--objects 40] [--batch 64] [--runs 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import axtrack_amd  # noqa: E402
from axtrack_amd import mot_metrics, params  # noqa: E402
from axtrack_amd.detections import AxonDetections  # noqa: E402


def median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def scene(F, n, seed=1, size=512):
    """n growth cones on a grid, drifting a few pixels per frame; 8 % of the detections missing, two strays per frame.
    -> per-frame detection tables, per-frame labels (x, y, identity)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    step = (size - 80) // side
    pos = np.stack([(np.arange(n) % side) * step + 40, (np.arange(n) // side) * step + 40], 1)[None] \
        + np.clip(np.cumsum(rng.integers(-2, 3, (F, n, 2)), 0), -step // 3, step // 3)
    tables, labels = [], []
    for f in range(F):
        keep = rng.random(n) >= 0.08
        xy = np.concatenate([pos[f, keep] + rng.integers(-3, 4, (int(keep.sum()), 2)), rng.integers(0, size, (2, 2))])
        conf = rng.uniform(0.75, 0.99, len(xy)).astype(np.float32)
        tables.append(pd.DataFrame({'conf': conf, 'anchor_x': xy[:, 0], 'anchor_y': xy[:, 1]}))
        labels.append((pos[f, :, 0], pos[f, :, 1], np.arange(n)))
    return tables, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=252)
    ap.add_argument('--objects', type=int, default=40)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    F, n, K = args.frames, args.objects, args.batch
    tables, labels = scene(F, n)
    tl = axtrack_amd.Timelapse(np.zeros((F + 4, 512, 512), np.float32), name='synth')
    ad = AxonDetections(None, tl, params.load_parameters(), tempfile.mkdtemp())
    ad._set_detections_from_tables(tables)
    ad.set_groundtruth(labels)
    ad.assign_ids()
    assert ad._solved
    target = ad.get_frame_dets('groundtruth', None, libmot=True)
    max_d2 = float(ad.nms_min_dist) ** 2

    def host():
        ad._ided_tables, ad._track_flat_cache = None, None       # as after every assign_ids() of the search
        pred = ad.get_frame_dets('IDed', None, libmot=True)
        return mot_metrics.summarize(mot_metrics.compare_to_groundtruth(target, pred, max_d2))

    def one():
        return ad.get_tracking_metrics()

    # K different associations: from a frame of its own on, every table exchanges the identities by a permutation of its own
    base = ad._track_dev()
    n_ids = int(base.max().item()) + 1
    g = torch.Generator().manual_seed(2)
    many = base[None].repeat(K, 1, 1)
    for k in range(1, K):
        perm = torch.arange(n_ids)
        sel = torch.randperm(n_ids, generator=g)[:max(2, n_ids // 8)]
        perm[sel] = sel.roll(1)
        f0 = int(torch.randint(1, F, (1,), generator=g))
        part = many[k, f0:]
        many[k, f0:] = torch.where(part >= 0, perm.to(base.device)[part.clamp(min=0).long()].to(torch.int32), part)

    def batch():
        return ad.score_associations(many)

    res = {'frames': F, 'objects': n, 'track_identities': n_ids, 'batch': K, 'runs': args.runs, 'warmup': args.warmup}
    res['a_host_ms'] = median_ms(host, args.runs, args.warmup)
    res['b_get_tracking_metrics_ms'] = median_ms(one, args.runs, args.warmup)
    res['c_score_associations_ms'] = median_ms(batch, args.runs, args.warmup)
    res['c_per_association_ms'] = res['c_score_associations_ms'] / K
    res['d_assign_ids_ms'] = median_ms(ad.assign_ids, args.runs, args.warmup)
    # the two routes give the same scores -- checked once, outside the timings
    a, b, c = host(), one(), batch()
    res['scores_equal'] = bool(np.allclose(a.to_numpy(float), b.to_numpy(float), rtol=0, atol=1e-12, equal_nan=True)
                               and np.allclose(a.to_numpy(float), c.iloc[0].to_numpy(float), rtol=0, atol=1e-12, equal_nan=True))
    res['distinct_rows_in_batch'] = int(len(c.drop_duplicates()))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
