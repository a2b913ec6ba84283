"""Generate tests/golden/train_parts.npz: inputs and outputs of the reference's tiled_target2yolo_format
(Timelapse.py:451-490) and YOLO_AXTrack_loss (loss.py:18-68) for small cases. Runs only where the read-only reference
checkout is present (tests/golden/_ref_import.py); only the data it writes is committed.

    python tests/golden/make_golden_train.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import import_reference  # noqa: E402

TS, S = 512, 12


def tiled_labels(lx, ly, ytiles, xtiles):
    """Whole-frame anchors i64 [F, cap] (-1 = none) -> [ytiles, xtiles, F, cap, 2] (y, x) tile coordinates, -1 outside
    the tile: the target half of construct_tiles (Timelapse.py:530-545), which needs a whole labelled dataset to run."""
    out = np.full((ytiles, xtiles) + lx.shape + (2,), -1, np.int64)
    for ty in range(ytiles):
        for tx in range(xtiles):
            inside = (ly >= ty * TS) & (ly < (ty + 1) * TS) & (lx >= tx * TS) & (lx < (tx + 1) * TS)
            out[ty, tx, ..., 0] = np.where(inside, ly - ty * TS, -1)
            out[ty, tx, ..., 1] = np.where(inside, lx - tx * TS, -1)
    return out


def main():
    import_reference()
    from reference.axtrack.Timelapse import Timelapse
    from reference.axtrack.machinelearning.loss import YOLO_AXTrack_loss
    rng = np.random.default_rng(20240607)
    out = {}
    # ---- targets: a 1024 x 700 frame (2 x 2 tiles), borders, a missing entry, two labels in one cell, an empty frame
    cases = {
        'a': ([[0, 511, 512, 699, 300, 301, -1, 5], [17, 650], [], [100, 100, 100]],
              [[0, 511, 512, 1023, 100, 101, -1, 900], [1000, 3], [], [40, 41, 42]]),
        'b': ([list(rng.integers(0, 700, 9)) for _ in range(5)], [list(rng.integers(0, 1024, 9)) for _ in range(5)]),
    }
    for name, (xs, ys) in cases.items():
        cap = max(len(x) for x in xs) + 2
        lx = np.full((len(xs), cap), -1, np.int64)
        ly = np.full((len(xs), cap), -1, np.int64)
        for t, (x, y) in enumerate(zip(xs, ys)):
            lx[t, :len(x)] = x
            ly[t, :len(y)] = y
        tiled = tiled_labels(lx, ly, 2, 2)
        me = types.SimpleNamespace(Sx=S, Sy=S, tilesize=TS)
        yolo = Timelapse.tiled_target2yolo_format(me, torch.from_numpy(tiled))
        out[f'tgt_{name}_lx'], out[f'tgt_{name}_ly'] = lx.astype(np.int32), ly.astype(np.int32)
        out[f'tgt_{name}_cnt'] = np.array([len(x) for x in xs], np.int32)
        out[f'tgt_{name}_tiled'] = tiled
        out[f'tgt_{name}_yolo'] = yolo.numpy().astype(np.float32)            # [ytile, xtile, F, 12, 12, 4]
    # ---- loss: random predictions against the targets of case b's tile (0, 0), in f32 and in f64
    target = torch.from_numpy(out['tgt_b_yolo'][0, 0])                        # [5, 12, 12, 4]
    for name, bs, lam in (('x', 5, (49.5, 1.0, 49.5)), ('y', 3, (2.0, 0.25, 7.0))):
        pred = torch.from_numpy(rng.normal(0.3, 0.6, (bs, S * S * 3)).astype(np.float32))
        fn = YOLO_AXTrack_loss(S, S, lam[0], lam[1], lam[2])
        _, c32 = fn(pred, target[:bs])
        p64 = pred.double().requires_grad_(True)
        loss64, c64 = fn(p64, target[:bs].double())
        loss64.backward()
        out[f'loss_{name}_pred'] = pred.numpy()
        out[f'loss_{name}_target'] = target[:bs].numpy()
        out[f'loss_{name}_lambda'] = np.array(lam, np.float64)
        out[f'loss_{name}_names'] = np.array(list(c64.index))
        out[f'loss_{name}_f32'] = c32.to_numpy(np.float64)
        out[f'loss_{name}_f64'] = c64.to_numpy(np.float64)
        out[f'loss_{name}_grad64'] = p64.grad.numpy()
    np.savez_compressed(os.path.join(HERE, 'train_parts.npz'), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
