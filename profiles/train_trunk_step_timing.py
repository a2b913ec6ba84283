"""One joint training step of the deployed detector at depths 5 and 8 at B = 32 on the GPU: ConvTrunkTrainer + HeadTrainer
(csrc/train_conv.hip, csrc/train.hip). Depth 5 reads the cached block-2 table (conv blocks 3..7 train); depth 8 gathers its
raw stacks per batch (hotpath.tile_stacks) and trains all eight conv blocks. The whole steps, each of their parts (per
block forward, input gradient and step, the pools, the gather, the head), and the same steps in torch on the same GPU
(conv2d, eval batch_norm, leaky_relu, max_pool2d, addmm, sigmoid, autograd, torch.optim.Adam foreach). Device events around
every step; the arms alternate in rounds within one run (WARM warm-up steps per arm, then ROUNDS x PER_ROUND timed steps
per arm), the median over all of an arm's steps with min and p90; FLOPs of the conv products from the shapes. Run from the
repository root: python profiles/train_trunk_step_timing.py [out.json] (default profiles/train_trunk_step_timing.json).
DESIGN.md 6.8e."""
import json, os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))
import numpy as np, torch
import torch.nn.functional as F
from axtrack_amd import hotpath, synth, training
from axtrack_amd.hotpath import conv_block_key, CONV_POOLED
import train_reference as tr

DEV = 'cuda:0'
B, N_TABLE, T_ALL = 32, 64, 68                      # 64 items in the block-2 table and 64 (frame, tile) items of raw stacks
ROUNDS, PER_ROUND, WARM = 3, 10, 3
sd = synth.synth_state_dict(42)
rng = np.random.default_rng(0)
x2 = torch.from_numpy(np.abs(rng.normal(0, 1, (N_TABLE, 80 * 64 * 64))).astype(np.float32)).to(DEV)
frames = torch.from_numpy(synth.synth_frames(T_ALL, 512, 512, seed=3)).to(DEV)
TILES = [(0, 0)]
_, tgt = tr.synth_table(N_TABLE, 8, 1)
tgt = torch.from_numpy(tgt).to(DEV)
batches = [torch.from_numpy(rng.permutation(N_TABLE)[:B].astype(np.int32)).to(DEV) for _ in range(8)]
ident = torch.arange(B, dtype=torch.int32, device=DEV)
stack_buf = torch.empty((B, 5 * 512 * 512), dtype=torch.float32, device=DEV)

head = training.HeadTrainer(sd, max_batch=B, device=DEV)
trunks = {5: training.ConvTrunkTrainer(sd, 3, 5, max_batch=B, device=DEV), 8: training.ConvTrunkTrainer(sd, 0, 8, max_batch=B, device=DEV)}


def source(depth, idx):
    if depth == 5:
        return x2, idx
    return hotpath.tile_stacks(frames, TILES, idx, out=stack_buf).view(B, -1), ident


def whole_step(depth):
    trunk = trunks[depth]

    def step(i):
        idx = batches[i % 8]
        x, rows = source(depth, idx)
        f = trunk.forward(x, rows)
        y = head.forward(f, ident)
        _, dy = head.loss(y, tgt, idx, read=False)
        dfeat = head.input_grad(dy)
        trunk.backward_and_step(x, rows, dfeat)
        head.step(f, ident, dy)
    return step


# the parts, on the tensors of one step with batch 0 (the steps move the weights, not the shapes: the times hold)
st = {}


def prime(depth):
    trunk = trunks[depth]
    x, rows = source(depth, batches[0])
    f = trunk.forward(x, rows)
    y = head.forward(f, ident)
    _, dy = head.loss(y, tgt, batches[0], read=False)
    g = head.input_grad(dy)
    kept = list(trunk._kept)
    kept[0] = (x, rows, kept[0][2])
    grads = {}
    for k in range(len(trunk.blocks) - 1, -1, -1):                          # every block's dF, formed without stepping
        blk, (xi, ri, fo) = trunk.blocks[k], kept[k]
        if trunk.pooled[k]:
            grads[('pool', k)] = g
            g = training.maxpool2_backward(fo, g, blk.H, blk.W).reshape(fo.shape)
        grads[('dF', k)] = g
        if k:
            g = blk.input_grad(g)
    st[depth] = dict(kept=kept, grads=grads, f=f, dy=dy)


def head_part(depth):
    def part(i):
        s = st[depth]
        y = head.forward(s['f'], ident)
        _, dy = head.loss(y, tgt, batches[0], read=False)
        head.input_grad(dy)
        head.step(s['f'], ident, dy)
    return part


def parts(depth):
    trunk, first = trunks[depth], trunks[depth].first_block
    P = {}
    if depth == 8:
        P['gather'] = lambda i: source(8, batches[0])
    for k, blk in enumerate(trunk.blocks):
        n = first + k
        P[f'forward_{n}'] = lambda i, k=k, blk=blk: blk.forward(*st[depth]['kept'][k][:2])
        if trunk.pooled[k]:
            P[f'pool_forward_{n}'] = lambda i, k=k, blk=blk: training.maxpool2_forward(st[depth]['kept'][k][2], blk.H, blk.W)
            P[f'pool_backward_{n}'] = lambda i, k=k, blk=blk: training.maxpool2_backward(st[depth]['kept'][k][2],
                                                                                         st[depth]['grads'][('pool', k)], blk.H, blk.W)
        if k:
            P[f'input_grad_{n}'] = lambda i, k=k, blk=blk: blk.input_grad(st[depth]['grads'][('dF', k)])
        P[f'step_{n}'] = lambda i, k=k, blk=blk: blk.step(*st[depth]['kept'][k][:2], st[depth]['grads'][('dF', k)])
    P['head_forward_loss_input_grad_step'] = head_part(depth)
    return P


def torch_step(depth):
    first = trunks[depth].first_block
    blocks = list(range(first, 8))
    names = [f'{conv_block_key(i)}.{k}' for i in blocks for k in training.CONV_SUFFIXES] + list(training.FC_KEYS)
    params = [torch.from_numpy(np.asarray(sd[k], np.float32)).to(DEV).requires_grad_(True) for k in names]
    stats = [[torch.from_numpy(np.asarray(sd[f'{conv_block_key(i)}.{k}'], np.float32)).to(DEV) for k in training.CONV_STATS]
             for i in blocks]
    opt = torch.optim.Adam(params, lr=5e-4, weight_decay=5e-4, foreach=True)

    def step(i):
        idx = batches[i % 8]
        x, _ = source(depth, idx)
        h = (x[idx.long()].reshape(B, 80, 64, 64) if depth == 5 else x.reshape(B, 5, 512, 512))
        T = tgt[idx.long()]
        for j, n in enumerate(blocks):
            p = params[4 * j:4 * j + 4]
            h = F.leaky_relu(F.batch_norm(F.conv2d(h, p[0], p[1], stride=2 if n < 2 else 1, padding=1), stats[j][0], stats[j][1],
                                          p[2], p[3], training=False, eps=1e-5), 0.1)
            if CONV_POOLED[n]:
                h = F.max_pool2d(h, 2, 2)
        hp = params[4 * len(blocks):]
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


ARMS, PRIME_AT = {}, {}
for depth in (5, 8):
    ARMS[f'hip_depth{depth}_step'] = whole_step(depth)
    ps = parts(depth)
    PRIME_AT[f'hip_depth{depth}_{next(iter(ps))}'] = depth
    ARMS.update({f'hip_depth{depth}_{k}': v for k, v in ps.items()})
    ARMS[f'torch_depth{depth}_step'] = torch_step(depth)
for depth in (5, 8):
    prime(depth)
for fn in ARMS.values():
    for i in range(WARM):
        fn(i)
torch.cuda.synchronize()
ms = {k: [] for k in ARMS}
for r in range(ROUNDS):
    for k, fn in ARMS.items():
        if k in PRIME_AT:
            prime(PRIME_AT[k])          # the parts follow a whole step of another batch: restore the tensors of batch 0
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(PER_ROUND)]
        for i, (a, b) in enumerate(ev):
            a.record(); fn(r * PER_ROUND + i); b.record()
        torch.cuda.synchronize()
        ms[k] += [a.elapsed_time(b) for a, b in ev]
out = {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), p90_ms=float(np.percentile(v, 90)), reps=len(v)) for k, v in ms.items()}

for depth, trunk in trunks.items():
    for k, blk in enumerate(trunk.blocks):
        n = trunk.first_block + k
        fl = 2 * blk.Co * blk.Ci * 9 * B * blk.H * blk.W                    # forward, weight gradient and input gradient alike
        out[f'hip_depth{depth}_forward_{n}']['GFLOPs'] = fl / out[f'hip_depth{depth}_forward_{n}']['median_ms'] / 1e6
        if k:
            out[f'hip_depth{depth}_input_grad_{n}']['GFLOPs'] = fl / out[f'hip_depth{depth}_input_grad_{n}']['median_ms'] / 1e6
    part_ms = sum(v['median_ms'] for a, v in out.items() if isinstance(v, dict) and a.startswith(f'hip_depth{depth}_') and a != f'hip_depth{depth}_step')
    out[f'depth{depth}'] = dict(sum_of_parts_ms=part_ms, sum_of_parts_over_whole=part_ms / out[f'hip_depth{depth}_step']['median_ms'],
                                step_vs_torch=out[f'torch_depth{depth}_step']['median_ms'] / out[f'hip_depth{depth}_step']['median_ms'],
                                trunk_device_bytes=trunk.device_bytes)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'train_trunk_step_timing.json')
json.dump(out, open(OUT, 'w'), indent=1)
print(json.dumps(out, indent=1))
