"""Generate tests/golden/scaler_parts.npz: the reference's own Timelapse._standardize (Timelapse.py:277-326) run on seven
sparse frames of preprocessed f32 values, for the four combinations of ('zscore' | '0to1') x (timelapse-wide | frame-wise):
the scaler it returns and the frames it leaves standardised. The method is called on a bare object that carries what it
reads (imseq, sizet), as make_golden.py bypasses Timelapse.__init__ (which reads a TIFF through tifffile). Runs only where the
read-only reference checkout is present (tests/golden/_ref_import.py); only the data it writes is committed.

    python tests/golden/make_golden_scaler.py
"""
import os
import sys
import types

import numpy as np
from scipy.sparse import coo_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import import_reference  # noqa: E402

T, H, W = 7, 64, 96


def frames_in():
    """Values as the preprocessing leaves them before scaling (log2(1 + x) of small x): about 5 % of the pixels non-zero,
    frame 3 much denser, the level drifting from frame to frame."""
    rng = np.random.default_rng(20241019)
    f = np.zeros((T, H, W), np.float32)
    for t in range(T):
        on = rng.random((H, W)) < (0.6 if t == 3 else 0.05)
        x = rng.integers(200, 4001, (H, W)) / 65535.0 * (1.0 + 0.15 * t)
        f[t] = np.where(on, np.log2(1.0 + x), 0.0).astype(np.float32)
    return f


def main():
    import_reference()
    from reference.axtrack.Timelapse import Timelapse
    f = frames_in()
    out = {'frames': f}
    for name in ('zscore', '0to1'):
        for framewise in (False, True):
            obj = types.SimpleNamespace(imseq=[coo_matrix(fr) for fr in f], sizet=T, name='train')
            scaler = Timelapse._standardize(obj, (name, None), framewise, None, False)
            key = f'{name}_{"framewise" if framewise else "global"}'
            assert scaler[0] == name and (scaler[1] is None) == framewise
            out[f'{key}_scaler'] = np.array([np.nan, np.nan] if framewise else scaler[1], np.float64)
            out[f'{key}_frames'] = np.stack([np.asarray(m.todense(), np.float32) for m in obj.imseq])
    np.savez_compressed(os.path.join(HERE, 'scaler_parts.npz'), **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()})
    print({k: v for k, v in out.items() if k.endswith('_scaler')})


if __name__ == '__main__':
    main()
