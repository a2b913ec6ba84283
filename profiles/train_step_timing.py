"""One training step of the deployed linear head (40960 -> 1024 -> 1024 -> 432) at B = 32 on the GPU: HeadTrainer's forward +
loss + step (csrc/train.hip) against the same step in torch on the same GPU (addmm, sigmoid, autograd, torch.optim.Adam).
Device events around every step after a warm-up, the median of 100 ... 200; bytes from the shapes. Run from the
repository root: python profiles/train_step_timing.py [out.json] (default profiles/train_step_timing.json). DESIGN.md 6.8e."""
import json, os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))
import numpy as np, torch
from axtrack_amd import synth, training
import train_reference as tr

DEV = 'cuda:0'
B, N_ITEMS, K0, H1, H2, NO = 32, 256, 40960, 1024, 1024, 432
sd = synth.synth_state_dict(42)
w = [np.asarray(sd[k], np.float32) for k in training.FC_KEYS]
rng = np.random.default_rng(0)
feats = torch.from_numpy(np.abs(rng.normal(0, 1, (N_ITEMS, K0))).astype(np.float32)).to(DEV)
_, tgt = tr.synth_table(N_ITEMS, 8, 1)
tgt = torch.from_numpy(tgt).to(DEV)
batches = [torch.from_numpy(rng.permutation(N_ITEMS)[:B].astype(np.int32)).to(DEV) for _ in range(8)]

def timed(fn, n_warm, n_rep):
    for i in range(n_warm):
        fn(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_rep)]
    t0 = time.perf_counter()
    for i, (a, b) in enumerate(ev):
        a.record(); fn(i); b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / n_rep * 1e3
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), p90_ms=float(np.percentile(ms, 90)), wall_ms_per_step=wall, reps=n_rep)

out = {}
t = training.HeadTrainer(dict(zip(training.FC_KEYS, w)), max_batch=B, device=DEV)
def hip_step(i):
    idx = batches[i % 8]
    y = t.forward(feats, idx)
    _, dy = t.loss(y, tgt, idx, read=False)
    t.step(feats, idx, dy)
def hip_step_only(i):
    t.step(feats, batches[0], DY)
def hip_fwd_only(i):
    t.forward(feats, batches[0])
out['hip_full_step'] = timed(hip_step, 10, 200)
y = t.forward(feats, batches[0]); _, DY = t.loss(y, tgt, batches[0], read=False)
out['hip_backward_update_only'] = timed(hip_step_only, 5, 100)
out['hip_forward_only'] = timed(hip_fwd_only, 5, 100)
del t
torch.cuda.empty_cache()

# the same step in torch: addmm, sigmoid, autograd, torch.optim.Adam
params = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in w]
for foreach in (None, False):
    opt = torch.optim.Adam(params, lr=5e-4, weight_decay=5e-4, foreach=foreach)
    def torch_step(i):
        idx = batches[i % 8].long()
        X, T = feats[idx], tgt[idx]
        a1 = torch.sigmoid(torch.addmm(params[1], X, params[0].T))
        a2 = torch.sigmoid(torch.addmm(params[3], a1, params[2].T))
        y = torch.addmm(params[5], a2, params[4].T).reshape(-1, 12, 12, 3)
        obj = T[..., 0:1]
        loss = (1.0 * ((y[..., 0:1] * (1 - obj)) ** 2).sum() + 49.5 * ((y[..., 0:1] * obj - obj) ** 2).sum()
                + 49.5 * ((y[..., 1:3] * obj - T[..., 1:3]) ** 2).sum()) / B
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    out[f'torch_full_step_foreach_{foreach}'] = timed(torch_step, 10, 100)

nw = K0 * H1 + H1 * H2 + H2 * NO
out['bytes_per_step_model'] = dict(weights_forward=4 * nw, wmv_in_out=6 * 4 * nw, features_B32=4 * B * K0,
                                   total=7 * 4 * nw + 2 * 4 * B * K0)
for k in ('hip_full_step', 'hip_backward_update_only'):
    byt = out['bytes_per_step_model']['total'] if k == 'hip_full_step' else 6 * 4 * nw + 4 * B * K0
    out[k]['GBps'] = byt / out[k]['median_ms'] / 1e6
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'train_step_timing.json')
json.dump(out, open(OUT, 'w'), indent=1)
print(json.dumps(out, indent=1))
