"""Axon reconstructions on the MI355X: reconstruction_arrays() (axt_track_links + axt_link_paths + axt_link_cells and the
copies to the host) timed with device events after a warm-up, and the DataFrame assembly of get_axon_reconstructions()
on the host, for config 3's scene (512^2 x 256, open grid) and one config-5 share (1024^2 x 64, corridor mask).
Usage: python profiles/recon_timing.py [out.json] [--astar-frames N] (astar_dets_paths() of the first N frames of the
config-5 share, for comparison)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import axtrack_amd                                     # noqa: E402
from axtrack_amd import synth, params                   # noqa: E402


def scene(F, size, alive, mask):
    dev = torch.device('cuda', 0)
    d = synth.synth_detections(F, size, size, n_alive=alive, seed=0)
    P = params.load_parameters()
    P['MCF_MAX_FLOW'] = 100000
    tl = axtrack_amd.Timelapse(torch.zeros((5, size, size)), name='recon', mask=mask, device=dev)
    ad = axtrack_amd.AxonDetections(None, tl, P, None)
    ad.set_detections(*(torch.from_numpy(d[k]).to(dev) for k in ('conf', 'x', 'y', 'count')))
    ad.assign_ids()
    return ad


def timed(ad, reps=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ad._recon = None
    ad.reconstruction_arrays()                          # warm-up (grid, kernels' first launch, staging buffers)
    gpu, wall, df = [], [], []
    for _ in range(reps):
        ad._recon = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        r = ad.reconstruction_arrays()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        gpu.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        ad.get_axon_reconstructions()
        df.append((time.perf_counter() - t0) * 1e3)
    return dict(links=int(len(r['len'])), cells=int(len(r['cells'])), no_path=int((r['len'] >= r['max_dist']).sum()),
                interpolated=int(len(r['interp_frame'])), reconstruction_arrays_event_ms=float(np.median(gpu)),
                reconstruction_arrays_wall_ms=float(np.median(wall)), dataframe_ms=float(np.median(df)), reps=reps)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith('--') else None
    n_astar = int(sys.argv[sys.argv.index('--astar-frames') + 1]) if '--astar-frames' in sys.argv else 0
    res = {'device': torch.cuda.get_device_name(0)}
    res['config3_open_512x256'] = timed(scene(256, 512, 90, None))
    c5 = scene(64, 1024, 330, synth.corridor_mask(1024, 1024))
    res['config5_share_corridor_1024x64'] = timed(c5)
    if n_astar:
        cnt = c5.d_count[:n_astar].clone()
        c5.d_count = torch.zeros_like(c5.d_count)
        c5.d_count[:n_astar] = cnt
        c5._host = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c5.astar_dets_paths()
        res['config5_share_astar_dets_paths_first_frames'] = dict(frames=n_astar, seconds=time.perf_counter() - t0)
    print(json.dumps(res, indent=1))
    if out:
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
