#!/usr/bin/env python3
"""Timings of the target screens -> profiles/target_timing.json and a markdown table on stdout.

  python profiles/target_timing.py [out.json]

Field: axt_target_field for a single-cell target near a corner on the two 1024 x 1024 masks (config 5's corridor mask and
the serpentine of tests/target_reference.py), both connectivities, with the round count; the yardstick in the same run is
the package's only other whole-grid search, hotpath.path_cost with ONE source and max_dist = 32767 (the largest the entry
point takes: on a 1024 x 1024 grid the gate never applies to the search, which always covers the whole grid; the gate
only filters the answer). Device events around the call, median of 5 after a warm-up. Then sampling and path extraction
for one config-5 share (64 frames), get_target_distances() end to end, and render_frames with and without the target
layer at config 3's size (host binning included: wall clock around a synchronised call)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from axtrack_amd import synth, params, hotpath as hp          # noqa: E402
import axtrack_amd                                             # noqa: E402
import target_reference as tr                                  # noqa: E402

REPS = 5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


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


def fields(res):
    H = W = 1024
    ty, tx = 5, 5
    sy, sx = H - 6, W - 6                       # the yardstick's single source: the far corner
    for name, mask in (('corridor', synth.corridor_mask(H, W)), ('serpentine', tr.serpentine_mask(H, W, 24, 48))):
        for conn8 in (False, True):
            grid = hp.Grid(mask, conn8)
            cells = dev([ty * W + tx])
            rounds = hp.target_field(cells, H, W, grid, conn8, return_rounds=True)[2]
            new = event_ms(lambda: hp.target_field(cells, H, W, grid, conn8))
            xa, ya, xb, yb = dev([sx]), dev([sy]), dev([tx]), dev([ty])
            old = event_ms(lambda: hp.path_cost(xa, ya, xb, yb, H, W, grid, 32767, conn8))
            t = time.perf_counter()
            ref = tr.field(mask, [ty * W + tx], conn8)
            scipy_ms = (time.perf_counter() - t) * 1e3
            moves = hp.target_field(cells, H, W, grid, conn8)[1]
            assert np.array_equal(moves.cpu().numpy(), ref[1])
            D = int(hp.path_cost(xa, ya, xb, yb, H, W, grid, 32767, conn8).cpu()[0, 0])
            assert D == min(int(ref[1][sy, sx]) + 1, 32767)
            res[f'field_{name}_conn{8 if conn8 else 4}'] = dict(
                target_field=new, rounds=int(rounds), tile=int(hp._lib.load().axt_target_tile_size()),
                path_cost_one_source=old, ratio=old['median_ms'] / new['median_ms'], scipy_reference_ms=scipy_ms,
                longest_moves=int(ref[1].max()))


def screens(res):
    H = W = 1024
    F = 64
    mask = synth.corridor_mask(H, W)
    d = synth.synth_detections(F, H, W, n_alive=300, seed=0)
    tl = axtrack_amd.Timelapse(torch.zeros((F + 4, H, W)), name='c5', mask=mask, device=torch.device('cuda', 0),
                               pixelsize=0.62, dt=31)
    P = params.load_parameters()
    P['MCF_MIN_FLOW'], P['MCF_MAX_FLOW'] = 1, 100000
    ad = axtrack_amd.AxonDetections(None, tl, P, None)
    ad.set_detections(*(torch.from_numpy(d[k]).cuda() for k in ('conf', 'x', 'y', 'count')))
    ad.assign_ids()
    ad.set_target((5, 5))
    off, moves = ad.target_field()
    grid = ad._mask_dev()
    res['sample_64_frames'] = dict(event_ms(lambda: hp.target_sample(off, moves, ad.d_x, ad.d_y, ad.d_count)),
                                   detections=int(d['count'].sum()))
    dm = hp.target_sample(off, moves, ad.d_x, ad.d_y, ad.d_count)[1]
    cells = hp.target_paths([(off, moves)], [grid], ad.d_x, ad.d_y, dm, H, W)[1]
    res['paths_64_frames'] = dict(event_ms(lambda: hp.target_paths([(off, moves)], [grid], ad.d_x, ad.d_y, dm, H, W)),
                                  cells=int(cells.numel()))

    def end_to_end():
        ad.set_target((5, 5))                   # drops the cached field: field + sampling + table
        return ad.get_target_distances()
    res['get_target_distances_cold'] = dict(wall_ms(end_to_end), rows=int(len(end_to_end())))
    res['get_target_distances_cached_field'] = wall_ms(ad.get_target_distances)


def rendering(res):
    H = W = 512
    F = 256
    d = synth.synth_detections(F, H, W, n_alive=75, seed=1)
    tl = axtrack_amd.Timelapse(synth.synth_frames(F + 4, H, W, seed=3), name='c3', device=torch.device('cuda', 0))
    P = params.load_parameters()
    P['MCF_MIN_FLOW'], P['MCF_MAX_FLOW'] = 1, 100000
    ad = axtrack_amd.AxonDetections(None, tl, P, None)
    ad.set_detections(*(torch.from_numpy(d[k]).cuda() for k in ('conf', 'x', 'y', 'count')))
    ad.assign_ids()
    ad.set_target((256, 500))
    ad.get_trg_path(0)                          # the paths are cached with the screen: not part of a render
    res['render_256_frames_without_layer'] = wall_ms(lambda: ad.render_frames(), reps=3)
    res['render_256_frames_with_layer'] = wall_ms(lambda: ad.render_frames(draw_target_paths=True), reps=3)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'target_timing.json')
    if not torch.cuda.is_available():
        raise SystemExit('target_timing.py needs the GPU: there is no CPU path to time')
    res = dict(device=torch.cuda.get_device_name(0), reps=REPS)
    fields(res)
    screens(res)
    rendering(res)
    with open(out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print('| case | target_field ms (median of 5) | rounds | path_cost, one source ms | ratio | SciPy ms |')
    print('|---|---|---|---|---|---|')
    for k, v in res.items():
        if k.startswith('field_'):
            print(f"| {k[6:]} | {v['target_field']['median_ms']:.2f} | {v['rounds']} | {v['path_cost_one_source']['median_ms']:.1f} | "
                  f"{v['ratio']:.1f} | {v['scipy_reference_ms']:.0f} |")
    for k, v in res.items():
        if isinstance(v, dict) and 'median_ms' in v:
            print(f"{k}: {v['median_ms']:.2f} ms (min {v['min_ms']:.2f}, max {v['max_ms']:.2f}) "
                  + ' '.join(f'{a}={b}' for a, b in v.items() if not a.endswith('_ms')))


if __name__ == '__main__':
    main()
