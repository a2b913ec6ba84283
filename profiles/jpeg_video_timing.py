"""The MJPEG video route (csrc/jpeg.hip, axtrack_amd/jpeg.py) on two scenes: config 3's 252 detection
frames of 512 x 512 and 128 frames of 1024 x 1024, both detected, tracked and drawn with every layer. Per scene: the
device time of axt_jpeg_encode_rgb8 on the whole batch (its five kernels; device events around the call after a warm-up,
median of 20), the bytes it writes, and the wall time of render_inference(video=True) against render_inference(
animated=True), the route that existed before, in the same process, alternating, after one warm-up of each (host clock;
both end with the file written), plus where the video route's time goes (render, encode + copy, container). Run from the
repository root: python profiles/jpeg_video_timing.py [out.json] (default profiles/jpeg_video_timing.json)."""
import json, os, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import numpy as np, torch
import axtrack_amd
from axtrack_amd import hotpath as hp, jpeg, params, synth

assert torch.cuda.is_available(), 'this measurement needs the GPU'
DEV = torch.device('cuda', 0)
LAYERS = dict(draw_grid=True, draw_scalebar=True, draw_axon_reconstructions=True, draw_brightened_bg=True, annotate=True,
              description='timing')
QUALITY, REPS = 90, 5


def scene(n_frames, H, W, seed):
    sd = synth.synth_state_dict(42)
    tl = axtrack_amd.Timelapse(synth.synth_frames(n_frames, H, W, seed=seed), name='timing', pixelsize=0.62, dt=31,
                               incubation_time=3000)
    P = params.load_parameters()
    P['MCF_MIN_FLOW'] = 1
    ad = axtrack_amd.AxonDetections(axtrack_amd.Detector(sd, max_batch=64), tl, P, None)
    ad.detect_dataset()
    ad.assign_ids()
    return ad


def stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), reps=len(v))


def kernel_time(rgb):
    N, H, W, _ = rgb.shape
    scan = torch.empty((N, 3 * H * W), dtype=torch.uint8, device=DEV)
    counts = torch.empty(N, dtype=torch.int64, device=DEV)
    status = torch.empty(N, dtype=torch.int32, device=DEV)
    scratch = torch.empty(hp.jpeg_scratch_bytes(N, H, W), dtype=torch.uint8, device=DEV)
    run = lambda: hp.jpeg_encode_launch(rgb, QUALITY, scan, counts, status, scratch)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for a, b in ev:
        a.record(); run(); b.record()
    torch.cuda.synchronize()
    assert not status.any().item()
    return dict(ms=stats([a.elapsed_time(b) for a, b in ev]), bytes_out=int(counts.sum().item()), bytes_in=int(rgb.numel()),
                scratch_bytes=int(scratch.numel()))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


out = {'quality': QUALITY, 'layers': sorted(LAYERS)}
with tempfile.TemporaryDirectory() as tmp:
    for name, (n, H, W) in {'config3_252x512x512': (256, 512, 512), 'scene_128x1024x1024': (132, 1024, 1024)}.items():
        ad = scene(n, H, W, 3)
        rgb = ad.render_frames(**LAYERS)
        res = dict(frames=int(rgb.shape[0]), H=H, W=W, encode=kernel_time(rgb))
        video = lambda: axtrack_amd.render_inference(ad, dest_dir=tmp, video=True, quality=QUALITY, **LAYERS)
        apng = lambda: axtrack_amd.render_inference(ad, dest_dir=tmp, animated=True, **LAYERS)
        video(); apng()
        tv, ta = [], []
        for _ in range(REPS):
            tv.append(wall(video)[0]); ta.append(wall(apng)[0])
        res['render_inference_video_s'], res['render_inference_apng_s'] = stats(tv), stats(ta)
        res['avi_bytes'] = os.path.getsize(f'{tmp}/timing_dets.avi')
        res['apng_bytes'] = os.path.getsize(f'{tmp}/timing_dets.png')
        parts = dict(render=[], encode_and_copy=[], container=[])
        for _ in range(REPS):
            t, rgb2 = wall(lambda: ad.render_frames(**LAYERS)); parts['render'].append(t)
            t, files = wall(lambda: jpeg.jpeg_encode(rgb2, QUALITY)); parts['encode_and_copy'].append(t)
            t, _ = wall(lambda: jpeg.write_mjpeg_avi(f'{tmp}/parts.avi', files, H, W, 6)); parts['container'].append(t)
        res['video_route_parts_s'] = {k: stats(v) for k, v in parts.items()}
        out[name] = res
        print(name, json.dumps(res), flush=True)
        del ad, rgb, rgb2, files
        torch.cuda.empty_cache()
path = sys.argv[1] if len(sys.argv) > 1 else 'profiles/jpeg_video_timing.json'
with open(path, 'w') as f:
    json.dump(out, f, indent=1)
print('wrote', path)
