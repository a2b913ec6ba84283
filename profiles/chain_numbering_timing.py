#!/usr/bin/env python3
"""HIP-event time of axt_chain_tracks alone, for the library in AXT_LIB_PATH (default: the tree's), at the headline
workload's shape (252 frames of 144 slots, ~77 detections a frame, nine in ten linked to the frame before and some of the
rest to the one before that), at slot counts on both sides of the bound between its two routes and at twice the slots. Prints one line
per shape: microseconds per call over 200 calls on one stream (back to back, so launch gaps of the multi-launch path count
as they do in the pipeline), after checking the track table against a walk on the CPU."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from axtrack_amd import _lib, hotpath as hp


def scene(F, cap, per_frame, seed=0):
    rng = np.random.default_rng(seed)
    count = np.minimum(rng.integers(per_frame - 8, per_frame + 9, F), cap).astype(np.int32)
    pred1 = np.full((F, cap), -1, np.int32)
    pred2 = np.full((F, cap), -1, np.int32)
    for t in range(1, F):
        k = int(0.9 * min(count[t], count[t - 1]))
        into = rng.permutation(int(count[t]))
        src1 = rng.permutation(int(count[t - 1]))[:k]
        pred1[t, into[:k]] = src1
        if t >= 2:                      # detections of t-2 that found no successor in t-1
            free = np.setdiff1d(np.arange(count[t - 2]), pred1[t - 1][pred1[t - 1] >= 0])
            k2 = min(len(free), len(into) - k) // 2
            pred2[t, into[k:k + k2]] = rng.permutation(free)[:k2]
    return count, pred1, pred2


def walk(count, cap, pred1, pred2):
    F = len(count)
    s = np.arange(F * cap)
    t, i = s // cap, s % cap
    valid = i < count[t]
    p1, p2 = pred1.reshape(-1), pred2.reshape(-1)
    parent = np.where(valid & (p1 >= 0), (t - 1) * cap + p1, np.where(valid & (p2 >= 0), (t - 2) * cap + p2, s))
    root = parent
    for _ in range(int(np.ceil(np.log2(max(F, 2)))) + 1):
        root = root[root]
    ids = np.cumsum(valid & (root == s)) - 1
    return np.where(valid, ids[root], -1).astype(np.int32).reshape(F, cap)


lib = _lib.load()
for F, cap, per in ((252, 144, 77), (56, 144, 77), (57, 144, 77), (252, 288, 150)):
    count, pred1, pred2 = scene(F, cap, per)
    slots = F * cap
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    d_count, pred = d(count), d(np.concatenate([pred1.reshape(-1), pred2.reshape(-1)]))
    work = torch.empty((2 * slots,), dtype=torch.int32, device='cuda')
    track = torch.empty((F, cap), dtype=torch.int32, device='cuda')
    n = torch.empty((1,), dtype=torch.int32, device='cuda')
    call = lambda: lib.axt_chain_tracks(d_count.data_ptr(), F, cap, pred.data_ptr(), work.data_ptr(), track.data_ptr(), n.data_ptr(), hp._stream())
    for _ in range(20):
        assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(track.cpu().numpy(), walk(count, cap, pred1, pred2)), (F, cap)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        call()
    e1.record()
    torch.cuda.synchronize()
    print(f'{os.path.basename(os.environ.get("AXT_LIB_PATH", "tree"))}: {F} frames x {cap} slots = {slots}: {e0.elapsed_time(e1) * 5:.1f} us per call', flush=True)
