"""One joint training step of the whole last conv stage (conv blocks 5 and 6, 80 -> 80 on 32 x 32 maps, the 2 x 2 max-pool,
conv block 7, 80 -> 160 on 16 x 16) and the deployed linear head (40960 -> 1024 -> 1024 -> 432) at B = 32 on the GPU:
ConvStageTrainer + HeadTrainer (csrc/train_conv.hip, csrc/train.hip), the step's parts one by one, and the same step in
torch on the same GPU (conv2d, eval batch_norm, leaky_relu, max_pool2d, addmm, sigmoid, autograd, torch.optim.Adam, foreach
and single-tensor). 256 cached items; device events around every step; the arms alternate in rounds within one run (10
warm-up steps per arm, then ROUNDS x PER_ROUND timed steps per arm), the median over all of an arm's steps with min and
p90; FLOPs of the conv products from the shapes. Run from the repository root:
python profiles/train_stage_step_timing.py [out.json] (default profiles/train_stage_step_timing.json). DESIGN.md 6.8e."""
import json, os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))
import numpy as np, torch
import torch.nn.functional as F
from axtrack_amd import synth, training
from axtrack_amd.hotpath import conv_block_key
import train_reference as tr

DEV = 'cuda:0'
B, N_ITEMS, C, C7, S5, S7, K0 = 32, 256, 80, 160, 32, 16, 40960
ROUNDS, PER_ROUND, WARM = 5, 25, 10
sd = synth.synth_state_dict(42)
rng = np.random.default_rng(0)
x4 = torch.from_numpy(np.abs(rng.normal(0, 1, (N_ITEMS, C * S5 * S5))).astype(np.float32)).to(DEV)
_, tgt = tr.synth_table(N_ITEMS, 8, 1)
tgt = torch.from_numpy(tgt).to(DEV)
batches = [torch.from_numpy(rng.permutation(N_ITEMS)[:B].astype(np.int32)).to(DEV) for _ in range(8)]
ident = torch.arange(B, dtype=torch.int32, device=DEV)

head = training.HeadTrainer(sd, max_batch=B, device=DEV)
stage = training.ConvStageTrainer(sd, 3, max_batch=B, device=DEV)
b5, b6, b7 = stage.blocks


def stage_step(i):
    idx = batches[i % 8]
    f = stage.forward(x4, idx)
    y = head.forward(f, ident)
    _, dy = head.loss(y, tgt, idx, read=False)
    dfeat = head.input_grad(dy)
    stage.backward_and_step(x4, idx, dfeat)
    head.step(f, ident, dy)


# the parts, on the tensors of one step with batch 0 (the steps move the weights, not the shapes: the times hold)
st = {}


def prime():
    idx = batches[0]
    st['f7'] = stage.forward(x4, idx)
    (_, _, st['f5']), (_, _, st['f6']), (st['pooled'], _, _) = stage._kept
    y = head.forward(st['f7'], ident)
    _, st['dy'] = head.loss(y, tgt, idx, read=False)
    st['dfeat'] = head.input_grad(st['dy'])
    st['dpooled'] = b7.input_grad(st['dfeat'])
    st['dF6'] = training.maxpool2_backward(st['f6'], st['dpooled'], S5, S5)
    st['dx6'] = b6.input_grad(st['dF6'])


def head_part(i):
    y = head.forward(st['f7'], ident)
    _, dy = head.loss(y, tgt, batches[0], read=False)
    head.input_grad(dy)
    head.step(st['f7'], ident, dy)


PARTS = dict(
    forward_5=lambda i: b5.forward(x4, batches[0]),
    forward_6=lambda i: b6.forward(st['f5'], ident),
    pool_forward=lambda i: training.maxpool2_forward(st['f6'], S5, S5),
    forward_7=lambda i: b7.forward(st['pooled'], ident),
    head_forward_loss_input_grad_step=head_part,
    input_grad_7=lambda i: b7.input_grad(st['dfeat']),
    pool_backward=lambda i: training.maxpool2_backward(st['f6'], st['dpooled'], S5, S5),
    input_grad_6=lambda i: b6.input_grad(st['dF6']),
    step_7=lambda i: b7.step(st['pooled'], ident, st['dfeat']),
    step_6=lambda i: b6.step(st['f5'], ident, st['dF6']),
    step_5=lambda i: b5.step(x4, batches[0], st['dx6']))

names = [f'{conv_block_key(i)}.{k}' for i in training.STAGE_BLOCKS for k in training.CONV_SUFFIXES] + list(training.FC_KEYS)
params = [torch.from_numpy(np.asarray(sd[k], np.float32)).to(DEV).requires_grad_(True) for k in names]
stats = [[torch.from_numpy(np.asarray(sd[f'{conv_block_key(i)}.{k}'], np.float32)).to(DEV) for k in training.CONV_STATS]
         for i in training.STAGE_BLOCKS]
opts = {fe: torch.optim.Adam(params, lr=5e-4, weight_decay=5e-4, foreach=fe) for fe in (None, False)}


def torch_stage(opt):
    def step(i):
        idx = batches[i % 8].long()
        h, T = x4[idx].reshape(B, C, S5, S5), tgt[idx]
        for j in range(3):
            p = params[4 * j:4 * j + 4]
            h = F.leaky_relu(F.batch_norm(F.conv2d(h, p[0], p[1], padding=1), stats[j][0], stats[j][1], p[2], p[3],
                                          training=False, eps=1e-5), 0.1)
            if j == 1:
                h = F.max_pool2d(h, 2, 2)
        hp = params[12:]
        a1 = torch.sigmoid(torch.addmm(hp[1], h.reshape(B, -1), hp[0].T))
        a2 = torch.sigmoid(torch.addmm(hp[3], a1, hp[2].T))
        y = torch.addmm(hp[5], a2, hp[4].T).reshape(-1, 12, 12, 3)
        obj = T[..., 0:1]
        loss = (1.0 * ((y[..., 0:1] * (1 - obj)) ** 2).sum() + 49.5 * ((y[..., 0:1] * obj - obj) ** 2).sum()
                + 49.5 * ((y[..., 1:3] * obj - T[..., 1:3]) ** 2).sum()) / B
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return step


ARMS = dict(hip_stage_step=stage_step, **{f'hip_{k}': v for k, v in PARTS.items()},
            torch_stage_step_foreach_None=torch_stage(opts[None]), torch_stage_step_foreach_False=torch_stage(opts[False]))
prime()
for fn in ARMS.values():
    for i in range(WARM):
        fn(i)
torch.cuda.synchronize()
ms = {k: [] for k in ARMS}
for r in range(ROUNDS):
    for k, fn in ARMS.items():
        if k == 'hip_forward_5':
            prime()                     # the parts follow a whole step of another batch: restore the tensors of batch 0
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(PER_ROUND)]
        for i, (a, b) in enumerate(ev):
            a.record(); fn(r * PER_ROUND + i); b.record()
        torch.cuda.synchronize()
        ms[k] += [a.elapsed_time(b) for a, b in ev]
out = {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), p90_ms=float(np.percentile(v, 90)), reps=len(v),
               round_medians_ms=[float(np.median(v[r * PER_ROUND:(r + 1) * PER_ROUND])) for r in range(ROUNDS)])
       for k, v in ms.items()}

flops = dict(forward_5=2 * C * C * 9 * B * S5 * S5, forward_6=2 * C * C * 9 * B * S5 * S5, forward_7=2 * C7 * C * 9 * B * S7 * S7)
flops.update(input_grad_6=flops['forward_6'], input_grad_7=flops['forward_7'])
out['model'] = dict(flops=flops)
for k, f in flops.items():
    out[f'hip_{k}']['GFLOPs'] = f / out[f'hip_{k}']['median_ms'] / 1e6
out['sum_of_parts_ms'] = float(sum(out[f'hip_{k}']['median_ms'] for k in PARTS))
out['sum_of_parts_over_whole'] = out['sum_of_parts_ms'] / out['hip_stage_step']['median_ms']
out['input_grad_over_forward'] = {k: out[f'hip_input_grad_{k}']['median_ms'] / out[f'hip_forward_{k}']['median_ms'] for k in '67'}
best_torch = min(out['torch_stage_step_foreach_None']['median_ms'], out['torch_stage_step_foreach_False']['median_ms'])
out['stage_step_vs_torch'] = best_torch / out['hip_stage_step']['median_ms']
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'train_stage_step_timing.json')
json.dump(out, open(OUT, 'w'), indent=1)
print(json.dumps(out, indent=1))
