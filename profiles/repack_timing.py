#!/usr/bin/env python3
"""What it costs to put a trained set of weights into a detector for evaluation, at fine-tuning depths 0
(the head alone), 3 (the last conv stage) and 8 (every conv block), two ways:

  export      the trainers' export_to into a live Detector: device kernels only (csrc/repack.hip);
  round trip  what fine-tuning did before for the same purpose: the state dict of the moment (trainer.state_dict(): every
              trained tensor device -> host), then Detector(state dict) (fold, Winograd transform and linear transposes in
              host loops, upload of everything, allocation of the activations).

Each is a host clock around the work, ending in a device synchronise. The two alternate within one process, after a warm-up
of both; per depth one JSON line with the median and the min..max spread of the repeats in milliseconds, after a check
that both detectors give the same bytes on one tile. Needs the GPU."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from axtrack_amd import synth, training
from axtrack_amd.hotpath import Detector

DEV = 'cuda:0'
REPEATS = int(os.environ.get('REPACK_TIMING_REPEATS', 7))
EXPORTS_PER_REPEAT = 5                                      # the export is short: several per repeat, the mean of them


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    assert torch.cuda.is_available(), 'repack_timing.py needs the GPU'
    sd = synth.synth_state_dict(42)
    frames = torch.from_numpy(synth.synth_frames(5, 512, 512, seed=3)).to(DEV)
    for depth in (0, 3, 8):
        head = training.HeadTrainer(sd, max_batch=2, device=DEV)
        trunk = training.ConvTrunkTrainer(sd, training.DEPTH_INPUT[depth][1], depth, max_batch=2, device=DEV) if depth else None
        live = Detector(sd, max_batch=32, device=DEV)

        def export():
            for _ in range(EXPORTS_PER_REPEAT):
                head.export_to(live)
                if trunk:
                    trunk.export_to(live)

        def round_trip():
            now = trunk.state_dict(head.state_dict()) if trunk else head.state_dict()
            return Detector(now, max_batch=32, device=DEV)

        export()
        built = clock(round_trip)[1]                        # warm-up of both, and the check
        assert torch.equal(live.detect_frames(frames, [(0, 0)]), built.detect_frames(frames, [(0, 0)]))
        del built
        t_export, t_trip = [], []
        for _ in range(REPEATS):
            t_export.append(clock(export)[0] / EXPORTS_PER_REPEAT)
            ms, built = clock(round_trip)
            del built
            t_trip.append(ms)
        row = dict(depth=depth, repeats=REPEATS,
                   export_ms=dict(median=statistics.median(t_export), min=min(t_export), max=max(t_export)),
                   round_trip_ms=dict(median=statistics.median(t_trip), min=min(t_trip), max=max(t_trip)))
        row['round_trip_over_export'] = row['round_trip_ms']['median'] / row['export_ms']['median']
        print(json.dumps(row), flush=True)
        del head, trunk, live


if __name__ == '__main__':
    main()
