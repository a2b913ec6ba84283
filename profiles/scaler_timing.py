"""Time the scaler statistics pass against what existed before it, in one process on one GPU:

  (a) axt_preprocess_stats_u16            per-frame n / sum / sumsq / max, 2 B of traffic per pixel
  (b) axt_preprocess_u16                  the existing fused pass, 6 B per pixel
  (c) estimate + frame-wise preprocess    (a), the scaler on the host, axt_preprocess_u16_framewise
  (d) the same result from (b) and torch  axt_preprocess_u16(scale=1), torch reductions over the f32 stack, a torch divide

Medians of `--runs` timed runs (wall clock around a device synchronisation, so (c) includes its host round trip) after
`--warmup` untimed ones, on T x H x W uint16 with 3 % of the pixels non-zero. Prints one JSON line.

    python profiles/scaler_timing.py [--frames 256] [--size 1024] [--runs 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from axtrack_amd import hotpath as hp, timelapse as tlm  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    T, H, W = args.frames, args.size, args.size
    g = torch.Generator(device=dev).manual_seed(1)
    raw = torch.empty((T, H, W), dtype=torch.int16, device=dev)
    for t in range(T):                              # frame by frame: no temporaries of the size of the stack
        on = torch.rand((H, W), device=dev, generator=g) < 0.03
        raw[t] = (torch.randint(200, 4001, (H, W), device=dev, generator=g) * on).to(torch.int16)
    out = torch.empty((T, H, W), dtype=torch.float32, device=dev)
    off, lo = 121 / 2 ** 16, 55 / 2 ** 16
    px = T * H * W

    def stats():
        return hp.preprocess_stats_u16(raw, None, off, lo, True)

    def existing():
        hp.preprocess_u16(raw, None, off, lo, True, 0.015176106, out=out)

    def new_path():
        st = stats()
        scaler, per_frame, scales = tlm.scaler_from_stats(st['n'], st['sum'], st['sumsq'], st['max'], 'zscore', True)
        hp.preprocess_u16_framewise(raw, scales, None, off, lo, True, out=out)
        return scales

    def composed():
        hp.preprocess_u16(raw, None, off, lo, True, 1.0, out=out)
        n = torch.count_nonzero(out, dim=(1, 2)).to(torch.float64)
        s = out.sum(dim=(1, 2), dtype=torch.float64)
        q = torch.linalg.vector_norm(out, dim=(1, 2), dtype=torch.float64) ** 2
        mean = s / n
        std = torch.sqrt(q / n - mean * mean)
        out.div_(std.to(torch.float32)[:, None, None])
        return std.cpu().numpy()

    res = {'shape': [T, H, W], 'runs': args.runs, 'warmup': args.warmup}
    res['a_stats_ms'] = median_ms(stats, args.runs, args.warmup)
    res['b_preprocess_ms'] = median_ms(existing, args.runs, args.warmup)
    res['c_estimate_framewise_ms'] = median_ms(new_path, args.runs, args.warmup)
    res['d_composed_ms'] = median_ms(composed, args.runs, args.warmup)
    res['a_GBps_at_2B_per_px'] = 2 * px / res['a_stats_ms'] / 1e6
    res['b_GBps_at_6B_per_px'] = 6 * px / res['b_preprocess_ms'] / 1e6
    # the two routes give the same scales (to the summation order) -- checked once, outside the timings
    a, b = new_path(), composed()
    res['max_rel_scale_difference'] = float(np.max(np.abs(a - b) / b))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
