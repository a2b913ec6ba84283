"""Rendering on the MI355X: AxonDetections.render_frames with every layer on, timed with device events after a warm-up
(the host-side binning of the boxes, labels, header and trail cells included, as it precedes the launch), the kernel
alone (events around hotpath.render_frames with the binned lists already on the device), and the wall time of
render_inference (PNG frames and one APNG) -- for config 3's scene (512^2 x 256, open grid) and one config-4 share
(1024^2 x 128, corridor mask). Usage: python profiles/render_timing.py [out.json]"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import axtrack_amd                                     # noqa: E402
from axtrack_amd import synth, params, hotpath as hp  # noqa: E402
from axtrack_amd import render as rnd                  # noqa: E402

LAYERS = dict(draw_grid=True, draw_scalebar=True, draw_axon_reconstructions=True, draw_true_dets=True,
              draw_brightened_bg=True, annotate=True, description='timing')


def scene(F, size, alive, mask):
    dev = torch.device('cuda', 0)
    d = synth.synth_detections(F, size, size, n_alive=alive, seed=0)
    P = params.load_parameters()
    P['MCF_MAX_FLOW'] = 100000
    tl = axtrack_amd.Timelapse(synth.synth_frames(F + 4, size, size, seed=1), name='render', mask=mask, device=dev,
                               pixelsize=0.62, dt=31, incubation_time=3000)
    ad = axtrack_amd.AxonDetections(None, tl, P, None)
    ad.set_detections(*(torch.from_numpy(d[k]).to(dev) for k in ('conf', 'x', 'y', 'count')))
    ad.assign_ids()
    cnt, _, x, y = ad._host_dets()
    ad.set_groundtruth([(x[t, :cnt[t]] + 2, y[t, :cnt[t]] + 2) for t in range(len(ad))])
    return ad


def kernel_only(ad, reps):
    """Events around the launch alone: the same inputs as render_frames builds, captured once."""
    captured = {}
    real = hp.render_frames

    def spy(*a):
        captured['args'] = a
        return real(*a)
    rnd.hp.render_frames = spy
    try:
        ad.render_frames(**LAYERS)
    finally:
        rnd.hp.render_frames = real
    a = captured['args']
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record()
        out = real(*a)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
        del out
    return times, int(a[13].shape[0]), int(a[16].shape[0])            # (trail cells, primitives)


def timed(ad, reps=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = ad.render_frames(**LAYERS)                       # warm-up (reconstructions, tables, first launch)
    T, H, W, _ = out.shape
    del out
    gpu, wall = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = ad.render_frames(**LAYERS)
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        gpu.append(e0.elapsed_time(e1))
        del out
    kern, n_trail, n_prims = kernel_only(ad, reps)
    moved = T * H * W * (4 + 3)
    res = dict(frames=T, height=H, width=W, trail_cells_binned=n_trail, primitives_binned=n_prims,
               render_frames_event_ms=float(np.median(gpu)), render_frames_wall_ms=float(np.median(wall)),
               kernel_event_ms=float(np.median(kern)), kernel_event_ms_all=[float(v) for v in kern],
               bytes_f32_in_rgb_out=moved, kernel_GBps=moved / (float(np.median(kern)) * 1e-3) / 1e9, reps=reps)
    with tempfile.TemporaryDirectory() as d:
        for animated in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            paths = axtrack_amd.render_inference(ad, dest_dir=d, animated=animated, **LAYERS)
            key = 'render_inference_apng_wall_s' if animated else 'render_inference_png_frames_wall_s'
            res[key] = time.perf_counter() - t0
            res[key.replace('wall_s', 'MB')] = sum(os.path.getsize(p) for p in paths) / 1e6
    return res


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    res = {'device': torch.cuda.get_device_name(0), 'target_kernel_ms_config3': 0.3}
    res['config3_open_512x256'] = timed(scene(256, 512, 90, None))
    print(json.dumps(res, indent=1), flush=True)
    torch.cuda.empty_cache()
    res['config4_share_corridor_1024x128'] = timed(scene(128, 1024, 120, synth.corridor_mask(1024, 1024)), reps=3)
    print(json.dumps(res, indent=1))
    if out:
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
