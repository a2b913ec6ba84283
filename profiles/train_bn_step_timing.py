"""The joint depth-3 training step of the last conv stage with the deployed head at B = 32 (profiles/train_stage_step_timing.py's
sizes) with train-mode BatchNorm in the three blocks (ConvStageTrainer(batch_stats=True): bn_batch_fwd_k, bn_batch_back_k,
conv_dgrad_dz_k of csrc/train_conv.hip) against the same step with running statistics IN THE SAME RUN, the blocks' calls one
by one in both modes (their difference is what the new kernels cost: a forward adds bn_batch_fwd_k, a step exchanges
conv_bn_back_k for bn_batch_back_k<true>, an input gradient exchanges conv_dgrad_k for bn_batch_back_k<false> +
conv_dgrad_dz_k), and torch's step with F.batch_norm(training=True) on the same GPU. 256 cached items; device events around
every call; the arms alternate in rounds within one run (10 warm-up calls per arm, then ROUNDS x PER_ROUND timed calls per
arm); median with min and p90. Run from the repository root:
python profiles/train_bn_step_timing.py [out.json] (default profiles/train_bn_step_timing.json). DESIGN.md 6.8e."""
import json, os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))
import numpy as np, torch
import torch.nn.functional as F
from axtrack_amd import synth, training
from axtrack_amd.hotpath import conv_block_key
import train_reference as tr

DEV = 'cuda:0'
B, N_ITEMS, C, C7, S5, S7 = 32, 256, 80, 160, 32, 16
ROUNDS, PER_ROUND, WARM = 5, 25, 10
sd = synth.synth_state_dict(42)
rng = np.random.default_rng(0)
x4 = torch.from_numpy(np.abs(rng.normal(0, 1, (N_ITEMS, C * S5 * S5))).astype(np.float32)).to(DEV)
_, tgt = tr.synth_table(N_ITEMS, 8, 1)
tgt = torch.from_numpy(tgt).to(DEV)
batches = [torch.from_numpy(rng.permutation(N_ITEMS)[:B].astype(np.int32)).to(DEV) for _ in range(8)]
ident = torch.arange(B, dtype=torch.int32, device=DEV)

MODES = {}
for mode in ('batch', 'eval'):
    MODES[mode] = dict(head=training.HeadTrainer(sd, max_batch=B, device=DEV),
                       stage=training.ConvStageTrainer(sd, 3, max_batch=B, device=DEV, batch_stats=mode == 'batch'), st={})


def stage_step(mode):
    head, stage = MODES[mode]['head'], MODES[mode]['stage']

    def step(i):
        idx = batches[i % 8]
        f = stage.forward(x4, idx)
        y = head.forward(f, ident)
        _, dy = head.loss(y, tgt, idx, read=False)
        dfeat = head.input_grad(dy)
        stage.backward_and_step(x4, idx, dfeat)
        head.step(f, ident, dy)
    return step


def prime(mode):
    """The tensors of one step with batch 0, which the single calls below work on."""
    head, stage, st = MODES[mode]['head'], MODES[mode]['stage'], MODES[mode]['st']
    b5, b6, b7 = stage.blocks
    st['f7'] = stage.forward(x4, batches[0])
    (_, _, st['f5']), (_, _, st['f6']), (st['pooled'], _, _) = stage._kept
    _, dy = head.loss(head.forward(st['f7'], ident), tgt, batches[0], read=False)
    st['dfeat'] = head.input_grad(dy)
    st['dpooled'] = b7.input_grad(st['dfeat'])
    st['dF6'] = training.maxpool2_backward(st['f6'], st['dpooled'], S5, S5)
    st['dx6'] = b6.input_grad(st['dF6'])


def parts(mode):
    stage, st = MODES[mode]['stage'], MODES[mode]['st']
    b5, b6, b7 = stage.blocks
    return {f'forward_5_{mode}': lambda i: b5.forward(x4, batches[0]),
            f'forward_6_{mode}': lambda i: b6.forward(st['f5'], ident),
            f'forward_7_{mode}': lambda i: b7.forward(st['pooled'], ident),
            f'input_grad_7_{mode}': lambda i: b7.input_grad(st['dfeat']),
            f'input_grad_6_{mode}': lambda i: b6.input_grad(st['dF6']),
            f'step_7_{mode}': lambda i: b7.step(st['pooled'], ident, st['dfeat']),
            f'step_6_{mode}': lambda i: b6.step(st['f5'], ident, st['dF6']),
            f'step_5_{mode}': lambda i: b5.step(x4, batches[0], st['dx6'])}


names = [f'{conv_block_key(i)}.{k}' for i in training.STAGE_BLOCKS for k in training.CONV_SUFFIXES] + list(training.FC_KEYS)
params = [torch.from_numpy(np.asarray(sd[k], np.float32)).to(DEV).requires_grad_(True) for k in names]
stats = [[torch.from_numpy(np.asarray(sd[f'{conv_block_key(i)}.{k}'], np.float32)).to(DEV).clone() for k in training.CONV_STATS]
         for i in training.STAGE_BLOCKS]
opt = torch.optim.Adam(params, lr=5e-4, weight_decay=5e-4)


def torch_step(i):
    idx = batches[i % 8].long()
    h, T = x4[idx].reshape(B, C, S5, S5), tgt[idx]
    for j in range(3):
        p = params[4 * j:4 * j + 4]
        h = F.leaky_relu(F.batch_norm(F.conv2d(h, p[0], p[1], padding=1), stats[j][0], stats[j][1], p[2], p[3],
                                      training=True, momentum=0.1, eps=1e-5), 0.1)
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


ARMS = dict(hip_stage_step_batch=stage_step('batch'), hip_stage_step_eval=stage_step('eval'))
for k in parts('batch'):                                    # the two modes of a call next to each other
    ARMS['hip_' + k] = parts('batch')[k]
    ARMS['hip_' + k.replace('_batch', '_eval')] = parts('eval')[k.replace('_batch', '_eval')]
ARMS['torch_stage_step_train_bn'] = torch_step
for mode in MODES:
    prime(mode)
for fn in ARMS.values():
    for i in range(WARM):
        fn(i)
torch.cuda.synchronize()
ms = {k: [] for k in ARMS}
for r in range(ROUNDS):
    for k, fn in ARMS.items():
        if k.startswith('hip_forward_5'):
            prime(k.rsplit('_', 1)[1])      # the single calls follow whole steps of other batches: restore batch 0's tensors
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(PER_ROUND)]
        for i, (a, b) in enumerate(ev):
            a.record(); fn(r * PER_ROUND + i); b.record()
        torch.cuda.synchronize()
        ms[k] += [a.elapsed_time(b) for a, b in ev]
out = {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), p90_ms=float(np.percentile(v, 90)), reps=len(v),
               round_medians_ms=[float(np.median(v[r * PER_ROUND:(r + 1) * PER_ROUND])) for r in range(ROUNDS)])
       for k, v in ms.items()}
med = lambda k: out[k]['median_ms']
z_bytes = {'5': 4 * B * C * S5 * S5, '6': 4 * B * C * S5 * S5, '7': 4 * B * C7 * S7 * S7}
# what the batch mode adds to each call, and the passes over arrays of z's size that the new kernels make in it: a forward
# reads z three times and writes F; a step reads z and dF twice each and writes dz, where conv_bn_back_k reads each once
out['added_ms'] = {k[4:-6]: med(k) - med(k.replace('_batch', '_eval')) for k in ARMS if k.endswith('_batch')}
out['model'] = dict(z_bytes=z_bytes, forward_added_passes=4, step_added_passes=2)
out['forward_added_GBps'] = {b: 4 * z_bytes[b] / out['added_ms'][f'forward_{b}'] / 1e6 for b in '567'}
out['sum_of_added_parts_ms'] = float(sum(v for k, v in out['added_ms'].items() if k != 'stage_step'))
out['batch_over_eval'] = med('hip_stage_step_batch') / med('hip_stage_step_eval')
out['batch_step_vs_torch'] = med('torch_stage_step_train_bn') / med('hip_stage_step_batch')
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'train_bn_step_timing.json')
json.dump(out, open(OUT, 'w'), indent=1)
print(json.dumps(out, indent=1))
