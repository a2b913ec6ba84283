"""One joint training step of the last conv block (80 -> 160 on 16 x 16 maps) and the deployed linear head (40960 -> 1024 ->
1024 -> 432) at B = 32 on the GPU: ConvBlockTrainer + HeadTrainer (csrc/train_conv.hip, csrc/train.hip) against the head-only
step and against the same joint step in torch on the same GPU (conv2d, eval batch_norm, leaky_relu, addmm, sigmoid,
autograd, torch.optim.Adam). 256 cached items; device events around every step; the arms alternate in rounds within one
run (10 warm-up steps per arm, then ROUNDS x PER_ROUND timed steps per arm), the median over all of an arm's steps;
bytes and FLOPs from the shapes. Run from the repository root:
python profiles/train_conv_step_timing.py [out.json] (default profiles/train_conv_step_timing.json). DESIGN.md 6.8e."""
import json, os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))
import numpy as np, torch
import torch.nn.functional as F
from axtrack_amd import synth, training
import train_reference as tr

DEV = 'cuda:0'
B, N_ITEMS, CI, CO, HW, K0, H1, H2, NO = 32, 256, 80, 160, 256, 40960, 1024, 1024, 432
ROUNDS, PER_ROUND, WARM = 5, 25, 10
sd = synth.synth_state_dict(42)
rng = np.random.default_rng(0)
x6 = torch.from_numpy(np.abs(rng.normal(0, 1, (N_ITEMS, CI * HW))).astype(np.float32)).to(DEV)
feats = torch.from_numpy(np.abs(rng.normal(0, 1, (N_ITEMS, K0))).astype(np.float32)).to(DEV)
_, tgt = tr.synth_table(N_ITEMS, 8, 1)
tgt = torch.from_numpy(tgt).to(DEV)
batches = [torch.from_numpy(rng.permutation(N_ITEMS)[:B].astype(np.int32)).to(DEV) for _ in range(8)]
ident = torch.arange(B, dtype=torch.int32, device=DEV)

head = training.HeadTrainer(sd, max_batch=B, device=DEV)
conv = training.ConvBlockTrainer(sd, max_batch=B, device=DEV)


def head_only(i):
    idx = batches[i % 8]
    y = head.forward(feats, idx)
    _, dy = head.loss(y, tgt, idx, read=False)
    head.step(feats, idx, dy)


def joint(i):
    idx = batches[i % 8]
    f = conv.forward(x6, idx)
    y = head.forward(f, ident)
    _, dy = head.loss(y, tgt, idx, read=False)
    dfeat = head.input_grad(dy)
    conv.step(x6, idx, dfeat)
    head.step(f, ident, dy)


# the parts, on the stashes of one joint step with batch 0
state = {}


def prime():
    idx = batches[0]
    state['f'] = conv.forward(x6, idx)
    y = head.forward(state['f'], ident)
    _, state['dy'] = head.loss(y, tgt, idx, read=False)
    state['dfeat'] = head.input_grad(state['dy'])


def conv_forward(i):
    conv.forward(x6, batches[0])


def input_grad(i):
    head.input_grad(state['dy'])


def conv_step(i):
    conv.step(x6, batches[0], state['dfeat'])


blk = training.LAST_CONV_BLOCK
names = [f'{blk}.{k}' for k in training.CONV_SUFFIXES] + list(training.FC_KEYS)
params = [torch.from_numpy(np.asarray(sd[k], np.float32)).to(DEV).requires_grad_(True) for k in names]
mean, var = (torch.from_numpy(np.asarray(sd[f'{blk}.{k}'], np.float32)).to(DEV) for k in training.CONV_STATS)
opts = {fe: torch.optim.Adam(params, lr=5e-4, weight_decay=5e-4, foreach=fe) for fe in (None, False)}


def torch_joint(opt):
    def step(i):
        idx = batches[i % 8].long()
        X, T = x6[idx].reshape(B, CI, 16, 16), tgt[idx]
        z = F.conv2d(X, params[0], params[1], padding=1)
        f = F.leaky_relu(F.batch_norm(z, mean, var, params[2], params[3], training=False, eps=1e-5), 0.1).reshape(B, -1)
        a1 = torch.sigmoid(torch.addmm(params[5], f, params[4].T))
        a2 = torch.sigmoid(torch.addmm(params[7], a1, params[6].T))
        y = torch.addmm(params[9], a2, params[8].T).reshape(-1, 12, 12, 3)
        obj = T[..., 0:1]
        loss = (1.0 * ((y[..., 0:1] * (1 - obj)) ** 2).sum() + 49.5 * ((y[..., 0:1] * obj - obj) ** 2).sum()
                + 49.5 * ((y[..., 1:3] * obj - T[..., 1:3]) ** 2).sum()) / B
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return step


ARMS = dict(hip_head_only_step=head_only, hip_joint_step=joint, hip_conv_forward=conv_forward, hip_input_grad=input_grad,
            hip_conv_step=conv_step, torch_joint_step_foreach_None=torch_joint(opts[None]),
            torch_joint_step_foreach_False=torch_joint(opts[False]))
prime()
for fn in ARMS.values():
    for i in range(WARM):
        fn(i)
torch.cuda.synchronize()
ms = {k: [] for k in ARMS}
for r in range(ROUNDS):
    for k, fn in ARMS.items():
        if k == 'hip_conv_forward':
            prime()                     # the parts follow a joint step of another batch: restore the stashes of batch 0
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(PER_ROUND)]
        for i, (a, b) in enumerate(ev):
            a.record(); fn(r * PER_ROUND + i); b.record()
        torch.cuda.synchronize()
        ms[k] += [a.elapsed_time(b) for a, b in ev]
out = {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), p90_ms=float(np.percentile(v, 90)), reps=len(v),
               round_medians_ms=[float(np.median(v[r * PER_ROUND:(r + 1) * PER_ROUND])) for r in range(ROUNDS)])
       for k, v in ms.items()}

nw_head, nw_conv, R = K0 * H1 + H1 * H2 + H2 * NO, CO * CI * 9, B * HW
out['model'] = dict(
    conv_forward=dict(flops=2 * CO * CI * 9 * R, bytes=4 * (B * CI * HW + nw_conv + 2 * B * CO * HW)),
    input_grad=dict(flops=2 * B * (NO * H2 + H2 * H1 + H1 * K0), bytes=4 * (K0 * H1 + H1 * H2 + H2 * NO + B * K0)),
    conv_step=dict(flops=2 * CO * CI * 9 * R, bytes=4 * (3 * B * CO * HW + B * CI * HW + 6 * nw_conv)),
    head_only_step=dict(bytes=7 * 4 * nw_head + 2 * 4 * B * K0))
for k, m in (('hip_conv_forward', 'conv_forward'), ('hip_input_grad', 'input_grad'), ('hip_conv_step', 'conv_step')):
    out[k]['GFLOPs'] = out['model'][m]['flops'] / out[k]['median_ms'] / 1e6
    out[k]['GBps'] = out['model'][m]['bytes'] / out[k]['median_ms'] / 1e6
best_torch = min(out['torch_joint_step_foreach_None']['median_ms'], out['torch_joint_step_foreach_False']['median_ms'])
out['joint_step_vs_torch'] = best_torch / out['hip_joint_step']['median_ms']
out['joint_step_no_slower_than_torch'] = bool(out['hip_joint_step']['median_ms'] <= best_torch)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'train_conv_step_timing.json')
json.dump(out, open(OUT, 'w'), indent=1)
print(json.dumps(out, indent=1))
