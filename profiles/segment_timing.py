#!/usr/bin/env python3
"""Timings of the mask preparation -> profiles/segment_timing.json and a markdown table on stdout.

  python profiles/segment_timing.py [out.json]

Every stage (axt_segment_edges, _histogram, _close, _flood) and the whole pipeline (segment.segment_mask: upload, the
four stages, the two read-backs of 256 counts and of min / max, download) at 1024 x 1024 and 4096 x 4096 on the synthetic
transmission image of config 5's corridor mask, and the flood alone on the serpentine of tests/target_reference.py, with
the rounds that did work. Device events around the call, median of 5 after a warm-up (the method of target_timing.py);
the pipeline is wall clock around a synchronised call, since it includes host work. There is no earlier implementation:
the yardstick is tests/segment_reference.py (SciPy and numpy, f64) on the host, wall clock, once, in the same run."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from axtrack_amd import synth, hotpath as hp, segment as seg   # noqa: E402
import segment_reference as sr                                 # noqa: E402
import target_reference as tr                                  # noqa: E402

REPS = 5


def event_ms(fn, reps=REPS):
    """Median / min / max of device-event times of fn() after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), max_ms=float(max(out)))


def wall_ms(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), max_ms=float(max(out)))


def host_ms(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def one_size(res, n):
    planted = synth.corridor_mask(n, n)
    img = synth.transmission_image(planted, seed=0)
    d_img = torch.from_numpy(img.view(np.int16)).cuda()
    r = {}
    # the yardstick, stage by stage
    P64, t_p = host_ms(lambda: sr.edge_magnitude(img))
    G64, t_g = host_ms(lambda: sr.smooth(P64, 1.0))
    mn64, mx64 = float(G64.min()), float(G64.max())
    h64, t_h = host_ms(lambda: np.histogram(G64, 256, range=(mn64, mx64))[0])
    thr64 = seg.otsu_threshold_from_hist(h64, mn64, mx64)
    C64, t_c = host_ms(lambda: sr.closing(P64 > thr64, 4))
    seed = sr.seed_of(planted, C64)
    F64, t_f = host_ms(lambda: sr.flood(C64, seed, 2))
    # the package
    P, G, mm = hp.segment_edges(d_img, 1.0)
    mn, mx = (float(v) for v in mm.cpu().numpy())
    hist = hp.segment_histogram(G, mn, mx)
    thr = seg.otsu_threshold_from_hist(hist.cpu().numpy(), mn, mx)
    C = hp.segment_close(P, thr, 4)
    F, rounds = hp.segment_flood(C, seed[0], seed[1], True, return_rounds=True)
    assert np.array_equal(F.cpu().numpy().astype(bool), sr.flood(C.cpu().numpy(), seed, 2))
    r['edges'] = dict(event_ms(lambda: hp.segment_edges(d_img, 1.0)), scipy_ms=t_p + t_g)
    r['edges_sigma_2.5'] = event_ms(lambda: hp.segment_edges(d_img, 2.5))
    r['histogram'] = dict(event_ms(lambda: hp.segment_histogram(G, mn, mx)), scipy_ms=t_h)
    r['close'] = dict(event_ms(lambda: hp.segment_close(P, thr, 4)), scipy_ms=t_c)
    r['flood_corridor'] = dict(event_ms(lambda: hp.segment_flood(C, seed[0], seed[1], True)), scipy_ms=t_f, rounds=int(rounds),
                               cells=int(F.sum()))
    r['pipeline'] = dict(wall_ms(lambda: seg.segment_mask(img, seed)), scipy_ms=t_p + t_g + t_h + t_c + t_f)
    r['iou'] = sr.iou(seg.segment_mask(img, seed), planted)
    r['pixels_differing_from_f64'] = float((seg.segment_mask(img, seed) != F64).mean())
    serp = tr.serpentine_mask(n, n, 24, 48)
    d_serp = torch.from_numpy(serp.view(np.uint8)).cuda()
    for conn8 in (False, True):
        S, rounds = hp.segment_flood(d_serp, 0, 0, conn8, return_rounds=True)
        ref, t_s = host_ms(lambda: sr.flood(serp, (0, 0), 2 if conn8 else 1))
        assert np.array_equal(S.cpu().numpy().astype(bool), ref)
        r[f'flood_serpentine_conn{8 if conn8 else 4}'] = dict(event_ms(lambda: hp.segment_flood(d_serp, 0, 0, conn8)), scipy_ms=t_s,
                                                              rounds=int(rounds), cells=int(ref.sum()))
    res[f'{n}x{n}'] = r


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'segment_timing.json')
    if not torch.cuda.is_available():
        raise SystemExit('segment_timing.py needs the GPU: there is no CPU path to time')
    res = dict(device=torch.cuda.get_device_name(0), reps=REPS, flood_tile=hp.segment_tile_size())
    for n in (1024, 4096):
        one_size(res, n)
    with open(out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print('| size | stage | GPU ms (median of 5) | min | max | SciPy f64 ms | rounds |')
    print('|---|---|---|---|---|---|---|')
    for size, r in res.items():
        if not isinstance(r, dict):
            continue
        for k, v in r.items():
            if isinstance(v, dict):
                print(f"| {size} | {k} | {v['median_ms']:.3f} | {v['min_ms']:.3f} | {v['max_ms']:.3f} | "
                      f"{v.get('scipy_ms', float('nan')):.1f} | {v.get('rounds', '')} |")
        print(f"{size}: IoU {r['iou']:.4f}, {r['pixels_differing_from_f64']:.2e} of the pixels differ from the f64 pipeline")


if __name__ == '__main__':
    main()
