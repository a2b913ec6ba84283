"""The augmentation warp (csrc/augment.hip) and one augmented epoch of fine_tune_head on config 3's frame stack (BASELINE.md:
256 frames of 512 x 512, 252 detection frames, one tile). The warp for translate + flip and for a 20 degree rotation, each
against a plain copy_ of the same buffers in the same run (the yardstick, alternating with it): device events around every
call after a warm-up, the median of 100; GB/s from the 2 x 4 bytes per pixel that either moves. One augmented epoch (warp +
occupancy read-back + label transform + trunk pass + targets + the head steps at B = 32) against one cached epoch (the head
steps alone, the parent path): host clock around work that ends in a device synchronise, the median of 7. Run from the
repository root: python profiles/augment_epoch_timing.py [out.json] (default profiles/augment_epoch_timing.json).
DESIGN.md 6.8e."""
import json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np, torch
import axtrack_amd
from axtrack_amd import augment, synth, training
from axtrack_amd.hotpath import tile_list

DEV = 'cuda:0'
T_ALL, H, W, B = 256, 512, 512, 32
assert torch.cuda.is_available(), 'this measurement needs the GPU'
frames = torch.from_numpy(synth.synth_frames(T_ALL, H, W, seed=0)).to(DEV)
warped = torch.empty_like(frames)
BYTES = 2 * frames.numel() * 4
CASES = {'translate_flip': augment.Transform(dy=-37, dx=53, flip_y=True, flip_x=True),
         'rotate_20': augment.Transform(angle=20.0),
         'all_five': augment.Transform(dy=-37, dx=53, flip_y=True, flip_x=True, angle=20.0)}


def timed_pair(fn, n_warm=10, n_rep=100):
    """fn and the copy alternating -> (fn's stats, the copy's stats)."""
    copy = lambda: warped.copy_(frames)
    for _ in range(n_warm):
        fn(); copy()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n_rep)]
    for a, b, c in ev:
        a.record(); fn(); b.record(); copy(); c.record()
    torch.cuda.synchronize()
    out = []
    for ms in (np.array([a.elapsed_time(b) for a, b, _ in ev]), np.array([b.elapsed_time(c) for _, b, c in ev])):
        out.append(dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), p90_ms=float(np.percentile(ms, 90)),
                        GBps=BYTES / float(np.median(ms)) / 1e6, reps=n_rep))
    return out


out = {'shape': [T_ALL, H, W], 'bytes_moved': BYTES, 'frame_chunk': augment.frame_chunk()}
for name, tf in CASES.items():
    for occ in (False, True):
        w, c = timed_pair(lambda: augment.augment_frames(frames, tf, return_occupancy=occ, out=warped))
        w['ratio_to_copy'] = w['median_ms'] / c['median_ms']
        out[f'warp_{name}' + ('_occ' if occ else '')] = dict(warp=w, copy=c)

# ---- one epoch, cached against augmented
sd = synth.synth_state_dict(42)
det = axtrack_amd.Detector(sd, max_batch=32, device=DEV)
rng = np.random.default_rng(0)
labels = [(list(rng.integers(20, W - 20, 3)), list(rng.integers(20, H - 20, 3))) for _ in range(T_ALL - 4)]
label_xy = augment.label_floats(labels)
label_xy = (*label_xy, np.full(len(labels), label_xy[0].shape[1], np.int32))
trainer = training.HeadTrainer(sd, max_batch=B, device=DEV)
table = torch.empty(((T_ALL - 4), 160 * 16 * 16), dtype=torch.float32, device=DEV)
tiles0 = [(0, 0)]
feats0 = det.features_frames(frames, tiles0)
tgt0 = training.yolo_targets(labels, tiles0, device=DEV).reshape(-1, 12, 12, 4)


def steps(feats, tgt):
    for batch in training.epoch_batches(feats.shape[0], B, True, False, rng):
        y = trainer.forward(feats, batch)
        comp, dy = trainer.loss(y, tgt, batch)
        trainer.step(feats, batch, dy, lr=1e-6)


def cached_epoch():
    steps(feats0, tgt0)


def prepare(tf):
    w, occ = augment.augment_frames(frames, tf, return_occupancy=True, out=warped)
    lab = augment.transform_labels(label_xy, tf, H, W)
    occ = occ.cpu()
    rate = augment.pos_label_rate(occ, *lab)
    tiles = tile_list(occ.amax(0), H, W)
    feats = det.features_frames(w, tiles, out=table)
    tgt = training.yolo_targets(lab, tiles, device=DEV).reshape(-1, 12, 12, 4)
    return feats, tgt, rate


def augmented_epoch(tf=CASES['all_five']):
    feats, tgt, _ = prepare(tf)
    steps(feats, tgt)


def wall(fn, n_warm=2, n_rep=7):
    for _ in range(n_warm):
        fn()
    ms = []
    for _ in range(n_rep):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), reps=n_rep)


out['trunk_pass_252_items'] = wall(lambda: det.features_frames(frames, tiles0, out=table))
out['prepare_only'] = wall(lambda: prepare(CASES['all_five']))
out['cached_epoch'] = wall(cached_epoch)
out['augmented_epoch'] = wall(augmented_epoch)
out['augmented_minus_cached_ms'] = out['augmented_epoch']['median_ms'] - out['cached_epoch']['median_ms']
out['steps_per_epoch'] = -(-(T_ALL - 4) // B)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'augment_epoch_timing.json')
json.dump(out, open(OUT, 'w'), indent=1)
print(json.dumps(out, indent=1))
