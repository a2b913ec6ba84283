"""Training of every conv block on the GPU (csrc/train_conv.hip: the stride-2 forms of conv_fwd_k, conv_wgrad_k and
conv_dgrad_k, tile_stacks_k; csrc/cnn.hip: the block-2 tap; axtrack_amd/training.py: ConvBlockTrainer(stride=, in_size=),
ConvTrunkTrainer, fine_tune_detector) against tests/train_trunk_reference.py: every quantity no further from the f64
reference than a small multiple of what plain f32 on the CPU is on the same input (train_reference.judge), the pools and
the gather byte for byte.

The single blocks are train_trunk_reference.BLOCK_CASES at stride 2 (odd and even input sides, a single window, Co and Ci
one past the 64-wide tile, r one past 64, 9 Ci no multiple of 16), a 5 x 66 map at stride 1 through the new create, and a
map both creates take, whose bytes must agree. The chain is the synthetic eight-block trunk with the deployed strides and
pools on an 80 x 48 input, which the three pools bring to 2 x 1 (a 40 x 24 input would leave the third pool a 2 x 1 map and
nothing to write). At deployed sizes the new tap, the gather and the chain's forward are held against the detector."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import entry_cases as ec
import train_conv_reference as cr
import train_reference as tr
import train_trunk_reference as tk
from axtrack_amd import hotpath, synth, training
from axtrack_amd.hotpath import conv_block_key
from test_entry_conventions_gpu import check, delay, new_handle, run, side_stream_run  # noqa: F401 (delay: a fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LR, WD, EPS = 1e-2, 0.05, 1e-3      # as tests/test_train_stage_gpu.py
ALL = training.CONV_SUFFIXES + training.CONV_STATS


def _sd(conv, key='blk'):
    return {f'{key}.{k}': a for k, a in zip(ALL, conv)}


def _block_trainer(conv, case, s, batch_stats=False, **kw):
    Ci, Co, Hin, Win, B = case
    return training.ConvBlockTrainer(_sd(conv), 'blk', dict(LR=LR, WEIGHT_DECAY=WD), max_batch=B, device=DEV,
                                     batch_stats=batch_stats, stride=s, in_size=(Hin, Win), **kw)


def _run_block(ct, x, dF):
    """forward, input_grad, step on rows 0..B-1 -> judge_block's `got`."""
    B = len(x)
    d_x, d_dF = torch.from_numpy(x.reshape(B, -1)).to(DEV), torch.from_numpy(dF.reshape(B, -1)).to(DEV)
    Fo = ct.forward(d_x)
    dx = ct.input_grad(d_dF)
    ct.step(d_x, None, d_dF, lr=LR, eps=EPS)
    mom = [ct.moments(i) for i in range(4)]
    assert [m[2] for m in mom] == [1] * 4
    got = dict(F=Fo.cpu().numpy(), dx=dx.cpu().numpy(), cw=ct.weights(), cm=[m[0] for m in mom], cv=[m[1] for m in mom])
    if ct.batch_stats:
        st = ct.stats()
        got['stats'] = [st['running_mean'], st['running_var']]
        assert st['num_batches_tracked'] == 1
    return got


def _judge_block(got, conv, x, dF, s, label, batch_stats=False):
    failures = []
    tk.judge_block(got, conv, x, dF, s, label, batch_stats, LR, WD, EPS, log=print, collect=failures)
    assert not failures, f'{len(failures)} comparisons failed:\n' + '\n'.join(failures[:10])


# ------------------------------------------------------------------------------------------------ one strided block
@pytest.mark.parametrize('case', tk.BLOCK_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_strided_block(case):
    """Forward, input gradient and one step of a stride-2 block with running statistics."""
    conv, x, dF = tk.block_case(case, 2)
    ct = _block_trainer(conv, case, 2)
    Ci, Co, Hin, Win, B = case
    assert (ct.H, ct.W) == (tk.out_size(Hin, 2), tk.out_size(Win, 2)) == dF.shape[2:]
    assert (ct.in_width, ct.out_width) == (Ci * Hin * Win, Co * ct.H * ct.W)
    _judge_block(_run_block(ct, x, dF), conv, x, dF, 2, f'stride 2 {case}')


@pytest.mark.parametrize('case', tk.BN_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_strided_block_with_batch_statistics(case):
    conv, x, dF = tk.block_case(case, 2, True)
    ct = _block_trainer(conv, case, 2, batch_stats=True)
    _judge_block(_run_block(ct, x, dF), conv, x, dF, 2, f'stride 2 batch statistics {case}', batch_stats=True)


def test_stride_one_on_a_map_beyond_64():
    """5 x 66 at stride 1: only the new create takes it."""
    conv, x, dF = tk.block_case(tk.WIDE_CASE, 1)
    with pytest.raises(Exception, match='axt_conv_trainer_create'):
        training.ConvBlockTrainer(_sd(conv), 'blk', map_size=tk.WIDE_CASE[2:4], max_batch=2, device=DEV)
    ct = _block_trainer(conv, tk.WIDE_CASE, 1)
    assert (ct.H, ct.W) == tk.WIDE_CASE[2:4]
    _judge_block(_run_block(ct, x, dF), conv, x, dF, 1, f'stride 1 {tk.WIDE_CASE}')


@pytest.mark.parametrize('batch_stats', [False, True])
def test_the_new_create_is_the_old_arithmetic(batch_stats):
    """On a map both creates take, a stride-1 handle of the new one gives the old one's bytes, and holds its memory."""
    case = (5, 41, 10, 9, 33)
    conv, x, dF = tk.block_case(case, 1)
    old = training.ConvBlockTrainer(_sd(conv), 'blk', dict(LR=LR, WEIGHT_DECAY=WD), map_size=case[2:4], max_batch=33, device=DEV,
                                    batch_stats=batch_stats)
    new = _block_trainer(conv, case, 1, batch_stats)
    assert old._CREATE == 'axt_conv_trainer_create' and new._CREATE == 'axt_conv_trainer_create_strided'
    assert old.device_bytes == new.device_bytes
    a, b = _run_block(old, x, dF), _run_block(new, x, dF)
    for k in a:
        for u, v in zip(*(([g[k]] if isinstance(g[k], np.ndarray) else g[k]) for g in (a, b))):
            assert u.tobytes() == v.tobytes(), k
    assert np.abs(a['cw'][0] - conv[0]).max() > LR / 2


def test_strided_trainer_refuses():
    conv, x, dF = tk.block_case((5, 20, 7, 10, 2), 2)
    for kw in (dict(stride=3), dict(stride=True), dict(stride=0)):
        with pytest.raises(ValueError, match='stride'):
            training.ConvBlockTrainer(_sd(conv), 'blk', device=DEV, **kw)
    with pytest.raises(Exception, match='axt_conv_trainer_create_strided'):
        training.ConvBlockTrainer(_sd(conv), 'blk', device=DEV, stride=2, in_size=(513, 8))
    with pytest.raises(Exception, match='axt_conv_trainer_create_strided'):
        training.ConvBlockTrainer(_sd(conv), 'blk', device=DEV, stride=1, in_size=(129, 8))
    ct = _block_trainer(conv, (5, 20, 7, 10, 2), 2)
    with pytest.raises(ValueError):
        ct.forward(torch.zeros((2, 5 * 4 * 5), device=DEV))                 # the output's width, not the input's


# ------------------------------------------------------------------------------------------------ the chain
def _trunk(args, first_block, n_trained, batch_stats=False, max_batch=2):
    convs, spec, shape, table, batches, dfeats, lrs, wd = args
    sd = {}
    for k, conv in enumerate(convs):
        sd.update(_sd(conv, f'c{first_block + k}'))
    return training.ConvTrunkTrainer(sd, first_block, n_trained, dict(LR=LR, WEIGHT_DECAY=wd), max_batch=max_batch, device=DEV,
                                     batch_stats=batch_stats, block_keys=[f'c{first_block + k}' for k in range(len(convs))],
                                     strides=[s for s, _, _ in spec], pooled=[p for _, p, _ in spec], in_size=shape[1:])


def _trunk_snapshot(tt):
    snap = []
    for blk in tt.blocks:
        mom = [blk.moments(i) for i in range(4)]
        st = blk.stats()
        snap.append(dict(cw=blk.weights(), cm=[m[0] for m in mom], cv=[m[1] for m in mom],
                         stats=[st['running_mean'], st['running_var']], nbt=st['num_batches_tracked'], t=mom[0][2]))
    return snap


def _run_trunk(tt, args):
    """ConvTrunkTrainer's steps -> (outs, snaps) shaped like train_trunk_reference.run_steps'; the pools against torch's CPU
    max_pool2d and its autograd on the run's own maps, bit for bit, on the way."""
    convs, spec, shape, table, batches, dfeats, lrs, wd = args
    d_table = torch.from_numpy(table).to(DEV)
    first = tt.first_block
    outs, snaps = [], []
    for idx, dfe, lr in zip(batches, dfeats, lrs):
        B = len(idx)
        Fo = tt.forward(d_table, idx)
        grads = tt.backward_and_step(d_table, idx, torch.from_numpy(dfe).to(DEV), lr=lr, eps=EPS)
        out = {}
        for k, (blk, (x, rows, f)) in enumerate(zip(tt.blocks, tt._kept)):
            out[f'F{k}'] = f.cpu().numpy()
            if tt.pooled[k]:
                nxt = tt._kept[k + 1][0].cpu().numpy()
                out[f'P{k}'] = nxt
                ft = f.cpu().reshape(B, blk.Co, blk.H, blk.W).clone().requires_grad_(True)
                want = F.max_pool2d(ft, 2, 2)
                assert nxt.tobytes() == want.detach().reshape(B, -1).numpy().tobytes(), f'pool behind block {first + k}'
                if f'p{first + k}' in grads:
                    want.backward(grads[f'p{first + k}'].cpu().reshape(want.shape))
                    assert grads[f'f{first + k}'].cpu().numpy().tobytes() == ft.grad.reshape(B, -1).numpy().tobytes()
        assert Fo.data_ptr() == tt._kept[-1][2].data_ptr()                   # no pool behind the last block
        for name, g in grads.items():                                        # 'p4' -> 'dP1' for a chain that starts at 3
            out[f'd{name[0].upper()}{int(name[1:]) - first}'] = g.cpu().numpy().reshape(B, -1)
        outs.append(out)
        snaps.append(_trunk_snapshot(tt))
    return outs, snaps


EXPECTED_GRADS = {4: {'p6', 'f6', 'f5', 'p4', 'f4'}, 5: {'p6', 'f6', 'f5', 'p4', 'f4', 'f3'},
                  6: {'p6', 'f6', 'f5', 'p4', 'f4', 'f3', 'p2', 'f2'},
                  8: {'p6', 'f6', 'f5', 'p4', 'f4', 'f3', 'p2', 'f2', 'f1', 'f0'}}


@pytest.mark.parametrize('depth,batch_stats', [(4, False), (5, False), (6, False), (8, False), (8, True)])
def test_trunk_steps(depth, batch_stats):
    """Three steps of the synthetic trunk at the depths that need the new chain, each judged per quantity against one
    restarted step of the chained reference; a forward-only block keeps its bytes (the judge compares them)."""
    first = 3 if depth <= 5 else 0
    args = tk.trunk_case(first, depth, batch_stats)
    tt = _trunk(args, first, depth, batch_stats)
    sizes, (C, h, w) = tk.chain_sizes(args[1], args[2], args[0])
    assert (h, w) == (2, 1) and tt.out_width == C * 2 and tt.in_width == int(np.prod(args[2]))
    assert [(b.Hin, b.Win, b.H, b.W) for b in tt.blocks] == [s[2:] for s in sizes]
    assert tt.trained == [k >= 8 - first - depth for k in range(8 - first)]
    held = tt.device_bytes
    outs, snaps = _run_trunk(tt, args)
    assert tt.device_bytes == held
    d_table = torch.from_numpy(args[3]).to(DEV)
    tt.forward(d_table, args[4][0])
    named = tt.backward_and_step(d_table, args[4][0], torch.from_numpy(args[5][0]).to(DEV), lr=0.0, eps=EPS)
    assert set(named) == EXPECTED_GRADS[depth]
    failures = []
    tk.judge_restarted(outs, snaps, args, (0, 1, 2), f'depth {depth}', eps=EPS, batch_stats=batch_stats, log=print,
                       collect=failures, names=[f'b{first + k}' for k in range(8 - first)])
    assert not failures, f'{len(failures)} comparisons failed:\n' + '\n'.join(failures[:10])
    sd = tt.state_dict()
    for k, blk in enumerate(tt.blocks):
        for key in blk.keys:
            assert (sd[key] is tt._sd[key]) == (not tt.trained[k] or (key.endswith(training.CONV_STATS) and not batch_stats)), key


def test_trunk_refuses():
    args = tk.trunk_case(3, 4)
    for first, n in ((8, 1), (-1, 1), (True, 1), (3, 6), (3, -1), (3, True)):
        with pytest.raises(ValueError):
            _trunk(args, first, n)
    tt = _trunk(args, 3, 4)
    with pytest.raises(ValueError, match='forward'):
        tt.backward_and_step(torch.zeros((6, tt.in_width), device=DEV), None, torch.zeros((2, tt.out_width), device=DEV))
    convs, spec, shape = args[:3]
    with pytest.raises(ValueError, match='max-pool'):                       # a 20 x 12 input reaches the third pool as 2 x 1
        training.ConvTrunkTrainer(tt._sd, 3, 4, device=DEV, block_keys=[f'c{3 + k}' for k in range(5)], strides=[1] * 5,
                                  pooled=[p for _, p, _ in spec], in_size=(5, 3))


# ------------------------------------------------------------------------------------------------ the gather
def _numpy_stacks(frames, tile_yx, index):
    T, H, W = frames.shape
    out = np.zeros((len(index), 5, 512, 512), np.float32)
    for b, item in enumerate(index):
        f, k = divmod(int(item), len(tile_yx))
        ty, tx = tile_yx[k]
        part = frames[f:f + 5, ty * 512:(ty + 1) * 512, tx * 512:(tx + 1) * 512]
        out[b, :, :part.shape[1], :part.shape[2]] = part
    return out


@pytest.mark.parametrize('W', [700, 701])
def test_tile_stacks_are_numpy_slices(W):
    """H = 520, T = 7, all four tiles (the lower right one holds 8 x 188 pixels), a shuffled index with a repeated item; a
    width that is no multiple of 4 takes the scalar kernel. The output is poisoned first: every float is written."""
    frames = np.random.default_rng(W).random((7, 520, W), dtype=np.float32) + 0.5
    tile_yx = [(0, 0), (0, 1), (1, 0), (1, 1)]
    index = np.random.default_rng(1).permutation(12)[:7]
    index[3], index[5] = index[0], 7                                        # a repeated item; frame 1, the lower right tile
    want = _numpy_stacks(frames, tile_yx, index)
    assert (want[5] != 0).sum() == 5 * 8 * (W - 512)
    d_frames = torch.from_numpy(frames).to(DEV)
    got = hotpath.tile_stacks(d_frames, tile_yx, index)
    assert got.shape == (7, 5, 512, 512) and got.cpu().numpy().tobytes() == want.tobytes()
    buf = torch.full((8, 5 * 512 * 512), float('nan'), device=DEV)
    part = hotpath.tile_stacks(d_frames, tile_yx, torch.from_numpy(index.astype(np.int32)).to(DEV), out=buf)
    assert part.data_ptr() == buf.data_ptr() and part.cpu().numpy().tobytes() == want.tobytes() and bool(buf[7].isnan().all())
    with pytest.raises(IndexError):
        hotpath.tile_stacks(d_frames, tile_yx, [12])
    far = hotpath.tile_stacks(d_frames, tile_yx, torch.tensor([12, -1, 7], dtype=torch.int32, device=DEV))
    assert not far[:2].any() and far[2].cpu().numpy().tobytes() == want[5].tobytes()     # beyond the items: +0.0, nothing read


# ------------------------------------------------------------------------------------------------ at deployed sizes
@pytest.fixture(scope='module')
def deployed(weights):
    import axtrack_amd
    import cnn_reference as cnr
    frames = torch.from_numpy(synth.synth_frames(6, 512, 512, seed=3)).to(DEV)
    det = axtrack_amd.Detector(weights, max_batch=2, device=DEV)
    stacks = hotpath.tile_stacks(frames, [(0, 0)], [0, 1])
    x, refs, yards = stacks.cpu().numpy(), [], []
    r = y = x
    for layer in range(8):                                                  # the f64 and f32 chains from the stacks, once
        r, y = cnr.ref_block(weights, layer, r), cnr.yard_block(weights, layer, y)
        refs.append(np.asarray(r))
        yards.append(np.asarray(y))
    return det, frames, stacks, refs, yards


def test_block_two_features(deployed):
    """block=2 is the detector's buffer 2 byte for byte; blocks 4, 6 and 7 return what they return without it in between."""
    import helpers
    det, frames, *_ = deployed
    old = {b: det.features_frames(frames, [(0, 0)], block=b).cpu().numpy() for b in (4, 6, 7)}
    x2 = det.trunk_features_frames(frames, [(0, 0)], block=2)
    assert tuple(x2.shape) == (2, 80 * 64 * 64)
    act2 = helpers.cnn_activation(det, 2, 0, 2)
    assert x2.cpu().numpy().tobytes() == act2.tobytes() and np.abs(act2).max() > 0
    for b, was in old.items():
        assert det.features_frames(frames, [(0, 0)], block=b).cpu().numpy().tobytes() == was.tobytes()
    for bad in (4, 5, 3):
        with pytest.raises(ValueError):
            det.trunk_features_frames(frames, [(0, 0)], block=bad)
    with pytest.raises(ValueError):
        det.features_frames(frames, [(0, 0)], block=2)
    table = torch.zeros((3, 80 * 64 * 64), device=DEV)                       # spare rows, as under augmentation
    part = det.trunk_features_frames(frames, [(0, 0)], out=table)
    assert part.data_ptr() == table.data_ptr() and part.cpu().numpy().tobytes() == act2.tobytes() and not table[2].any()


def test_block_two_features_over_several_chunks(weights):
    """More items than the front's chunk and than max_batch: every chunk's copy lands in its rows."""
    import axtrack_amd
    import helpers
    chunk_a, chunk_b = helpers.cnn_chunks()
    n = min(2 * chunk_b + 1, 9)
    frames = torch.from_numpy(synth.synth_frames(n + 4, 512, 512, seed=4)).to(DEV)
    det = axtrack_amd.Detector(weights, max_batch=max(2, min(chunk_b, n - 1)), device=DEV)
    whole = det.trunk_features_frames(frames, [(0, 0)]).cpu().numpy()
    for t in (0, n // 2, n - 1):
        one = det.trunk_features_frames(frames, [(0, 0)], t0=t, n_frames=1).cpu().numpy()
        assert one.tobytes() == whole[t:t + 1].tobytes(), t


def _forward_check(tt, table, first, refs, yards, x7, inp0, B=2):
    import cnn_reference as cnr
    out = tt.forward(table)
    inp = inp0
    for k, (blk, (x, rows, f)) in enumerate(zip(tt.blocks, tt._kept)):
        layer = first + k
        got = (tt._kept[k + 1][0] if tt.pooled[k] else f).cpu().numpy().reshape(refs[layer].shape)
        ref, yard = cnr.ref_block(tt._sd, layer, inp), cnr.yard_block(tt._sd, layer, inp)
        r = cnr.judge(got, ref, yard, *cnr.bound_for('f32_direct', layer), layer=f'ConvTrunkTrainer.forward (conv block {layer})')
        print(f'ConvTrunkTrainer.forward conv block {layer} against f64: {r[0]:.3f} (max) {r[1]:.3f} (rms) of the f32 yardstick')
        inp = got
    c_direct, c_det = cnr.bound_for('f32_direct', 7), cnr.bound_for('f32_winograd', 7)
    got = out.cpu().numpy().reshape(x7.shape)
    diff, allowed = np.abs(got - x7).max(), (c_direct[0] + c_det[0]) * (np.abs(yards[7] - refs[7]).max() + cnr.FLOOR_MAX)
    print(f'the chain\'s output against features_frames(block=7): max difference {diff:.3g}, allowed {allowed:.3g}')
    assert diff <= allowed


def test_trunk_forward_from_the_block_two_table_is_the_detectors(deployed, weights):
    det, frames, stacks, refs, yards = deployed
    x7 = det.features_frames(frames, [(0, 0)], block=7).cpu().numpy().reshape(2, 160, 16, 16)
    x2 = det.trunk_features_frames(frames, [(0, 0)])
    tt = training.ConvTrunkTrainer(weights, 3, 5, max_batch=2, device=DEV)
    assert [(b.Ci, b.Co, b.H, b.W) for b in tt.blocks] == [(80, 80, 64, 64), (80, 80, 64, 64), (80, 80, 32, 32), (80, 80, 32, 32),
                                                           (80, 160, 16, 16)]
    assert all(b._CREATE == 'axt_conv_trainer_create' for b in tt.blocks)    # maps the old create takes: its calls
    # refs / yards start from the stacks; from the block-2 table the chain's yardstick is the tail from the table itself
    import cnn_reference as cnr
    r = y = x2.cpu().numpy().reshape(2, 80, 64, 64)
    tail_r, tail_y = list(refs), list(yards)
    for layer in range(3, 8):
        r, y = cnr.ref_block(weights, layer, r), cnr.yard_block(weights, layer, y)
        tail_r[layer], tail_y[layer] = np.asarray(r), np.asarray(y)
    _forward_check(tt, x2, 3, tail_r, tail_y, x7, x2.cpu().numpy().reshape(2, 80, 64, 64))


def test_trunk_forward_from_gathered_stacks_is_the_detectors(deployed, weights):
    det, frames, stacks, refs, yards = deployed
    x7 = det.features_frames(frames, [(0, 0)], block=7).cpu().numpy().reshape(2, 160, 16, 16)
    tt = training.ConvTrunkTrainer(weights, 0, 8, max_batch=2, device=DEV)
    assert [(b.stride, b.Hin, b.H) for b in tt.blocks[:3]] == [(2, 512, 256), (2, 256, 128), (1, 128, 128)]
    assert tt.in_width == 5 * 512 * 512 and tt.out_width == 160 * 16 * 16
    _forward_check(tt, stacks.view(2, -1), 0, refs, yards, x7, stacks.cpu().numpy())


# ------------------------------------------------------------------------------------------------ end to end
def _e2e_setup(weights):
    import axtrack_amd
    E = tr.E2E
    frames = synth.synth_frames(E['T_all'], E['H'], E['W'], seed=E['frames_seed'])
    tl = axtrack_amd.Timelapse(frames, name='train', device=DEV)
    det = axtrack_amd.Detector(weights, max_batch=8, device=DEV)
    return E, tl, det, tr.e2e_labels()


def _same(a, b):
    return set(a) == set(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def _back(path):
    from axtrack_amd.interface import _load_state_dict
    return {k: v.numpy() for k, v in _load_state_dict(path).items()}


@pytest.fixture(scope='module')
def e2e(weights):
    return _e2e_setup(weights)


@pytest.mark.parametrize('depth', [0, 1, 2, 3])
def test_depths_up_to_three_are_fine_tune_heads_bytes(weights, e2e, tmp_path, depth):
    import axtrack_amd
    E, tl, det, labels = e2e
    runs = []
    for name, fn in (('head', axtrack_amd.fine_tune_head), ('detector', axtrack_amd.fine_tune_detector)):
        sd, hist = fn(tl, labels, det, E['parameters'], E['epochs'], dest_dir=f'{tmp_path}/{name}', seed=E['seed'],
                      train_conv_blocks=depth)
        runs.append((sd, hist.to_numpy().tobytes(), _back(f'{tmp_path}/{name}/E{E["epochs"] - 1:04}.pth')))
    assert _same(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and _same(runs[0][2], runs[1][2])


# Two f32 evaluations of one loss that differ in the order of their sums (the chain's direct convolutions, the detector's
# Winograd ones): each within 2^-24 sqrt(K) of the exact value per reduction of length K, relative to the largest value, summed
# over the eight conv blocks' 9 Ci and the three linear layers' widths, for both evaluations
FIRST_BATCH_RTOL = 2 * 2.0 ** -24 * sum(np.sqrt(k) for k in (45, 180, 360, 720, 720, 720, 720, 720, 40960, 1024, 1024))


@pytest.fixture(scope='module')
def depth0_first_batch(weights, e2e):
    import axtrack_amd
    E, tl, det, labels = e2e
    P = dict(E['parameters'], SHUFFLE=False, BATCH_SIZE=8)
    _, hist = axtrack_amd.fine_tune_detector(tl, labels, det, P, 1, seed=E['seed'])
    return P, hist[0].to_numpy()


@pytest.mark.parametrize('depth', [5, 8])
def test_fine_tune_detector_end_to_end(weights, e2e, depth0_first_batch, tmp_path, depth):
    """8 items, shuffled batches of 5 and 3, 3 epochs: two runs are byte-identical in state dict, history and reloaded
    checkpoint; exactly the trained blocks' four tensors and the head's moved, every other tensor is the object that went
    in; the result builds a Detector that detects what its checkpoint detects, and not what the start detected."""
    import axtrack_amd
    E, tl, det, labels = e2e
    runs = []
    for name in ('a', 'b'):
        sd, hist = axtrack_amd.fine_tune_detector(tl, labels, det, E['parameters'], E['epochs'], dest_dir=f'{tmp_path}/{name}',
                                                  seed=E['seed'], train_conv_blocks=depth)
        runs.append((sd, hist.to_numpy().tobytes(), _back(f'{tmp_path}/{name}/E{E["epochs"] - 1:04}.pth')))
    sd, back = runs[0][0], runs[0][2]
    assert _same(sd, runs[1][0]) and runs[0][1] == runs[1][1] and _same(back, runs[1][2])
    assert np.isfinite(hist.to_numpy()).all() and list(hist.index) == list(tr.COMPONENTS)
    trained = {f'{conv_block_key(i)}.{s}' for i in range(8 - depth, 8) for s in training.CONV_SUFFIXES} | set(training.FC_KEYS)
    assert set(sd) == set(weights) and all(sd[k] is weights[k] for k in weights if k not in trained)
    assert all(np.abs(np.asarray(sd[k], np.float64) - weights[k]).max() > 0 for k in trained), 'a trained tensor stayed'
    assert all(np.array_equal(back[k], np.asarray(sd[k])) for k in sd)
    grids = axtrack_amd.Detector(sd, max_batch=8, device=DEV).detect_frames(tl.frames, tl.tile_yx)
    assert (grids - axtrack_amd.Detector(back, max_batch=8, device=DEV).detect_frames(tl.frames, tl.tile_yx)).abs().max().item() == 0
    assert (grids - det.detect_frames(tl.frames, tl.tile_yx)).abs().max().item() > 1e-3
    # the first batch's loss before any weight has moved is depth 0's, within what the chain's forward differs from the
    # detector's by (test_trunk_forward_*): one epoch of one unshuffled batch of all 8 items
    P, want = depth0_first_batch
    _, h1 = axtrack_amd.fine_tune_detector(tl, labels, det, P, 1, seed=E['seed'], train_conv_blocks=depth)
    got = h1[0].to_numpy()
    print(f'depth {depth} first batch: {got} against depth 0: {want}')
    assert np.abs(got - want).max() <= FIRST_BATCH_RTOL * np.abs(want).max(), (got, want)


def test_batch_statistics_count_every_forward_at_depth_eight(weights, e2e):
    import axtrack_amd
    E, tl, det, labels = e2e
    sd, hist = axtrack_amd.fine_tune_detector(tl, labels, det, E['parameters'], E['epochs'], seed=E['seed'], train_conv_blocks=8,
                                              bn_batch_stats=True)
    forwards = 2 * E['epochs']
    for i in range(8):
        k = f'{conv_block_key(i)}.{training.CONV_COUNTER}'
        assert int(np.asarray(sd[k])) - int(np.asarray(weights[k])) == forwards if k in weights else int(np.asarray(sd[k])) == forwards
        rm = f'{conv_block_key(i)}.batchnorm.running_mean'
        assert np.abs(np.asarray(sd[rm], np.float64) - np.asarray(weights[rm], np.float64)).max() > 0
    assert np.isfinite(hist.to_numpy()).all()
    axtrack_amd.Detector(sd, max_batch=2, device=DEV)


@pytest.mark.parametrize('depth', [5, 7])
def test_augmented_epochs_read_the_warped_frames(weights, e2e, depth):
    """One explicit transform per epoch: the block-2 table (depth 5) or the gathered stacks (depth 7) come from the warped
    frames, so the run differs from the plain one; it repeats byte for byte and records its transforms."""
    import axtrack_amd
    from axtrack_amd.augment import Transform
    E, tl, det, labels = e2e
    tfs = [dict(dx=-40), Transform(dy=7, flip_y=True)]
    run = lambda **kw: axtrack_amd.fine_tune_detector(tl, labels, det, E['parameters'], 2, seed=E['seed'], train_conv_blocks=depth,
                                                      **kw)
    (sd, hist), (sd2, hist2), (plain, _) = run(transforms=tfs), run(transforms=tfs), run()
    assert _same(sd, sd2) and hist.to_numpy().tobytes() == hist2.to_numpy().tobytes() and np.isfinite(hist.to_numpy()).all()
    assert hist.attrs['transforms'] == [Transform(dx=-40), tfs[1]]
    k = f'{conv_block_key(7)}.conv.weight'
    assert np.asarray(sd[k]).tobytes() != np.asarray(plain[k]).tobytes()
    assert all(sd[key] is weights[key] for i in range(8 - depth) for key in (f'{conv_block_key(i)}.{s}' for s in training.CONV_SUFFIXES))


def test_depth_four_returns_block_three_as_it_came(weights, e2e):
    import axtrack_amd
    E, tl, det, labels = e2e
    sd, hist = axtrack_amd.fine_tune_detector(tl, labels, det, E['parameters'], E['epochs'], seed=E['seed'], train_conv_blocks=4)
    trained = {f'{conv_block_key(i)}.{s}' for i in range(4, 8) for s in training.CONV_SUFFIXES} | set(training.FC_KEYS)
    assert set(sd) == set(weights) and all(sd[k] is weights[k] for k in weights if k not in trained)
    assert all(np.abs(np.asarray(sd[k], np.float64) - weights[k]).max() > 0 for k in trained)
    assert np.isfinite(hist.to_numpy()).all()


def test_fine_tune_detector_errors_come_before_any_gpu_work(weights, e2e):
    import axtrack_amd
    E, tl, det, labels = e2e
    for bad in (9, -1, True):
        with pytest.raises(ValueError, match='train_conv_blocks'):
            axtrack_amd.fine_tune_detector(tl, labels, det, E['parameters'], 1, train_conv_blocks=bad)
    with pytest.raises(ValueError, match='train_conv_blocks'):
        axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], 1, train_conv_blocks=4)
    tl.frame_sharded = True
    try:
        with pytest.raises(NotImplementedError):
            axtrack_amd.fine_tune_detector(tl, labels, det, E['parameters'], 1, train_conv_blocks=8)
    finally:
        tl.frame_sharded = False


# ------------------------------------------------------------------------------------------------ streams and poison
SC, SO, SH, SW = 3, 5, 7, 10                        # the strided block of the stream cases: 3 -> 5 channels, 7 x 10 -> 4 x 5
S_ROWS, S_BATCH = 5, 3


def _strided_handle(host):
    sd = _sd(cr.synth_block(SC, SO, 6, scale=2.0))
    return training.ConvBlockTrainer(sd, 'blk', ec.TRAIN_P, max_batch=S_BATCH, stride=2, in_size=(SH, SW))


def _make_strided(kind, salt):
    rng = ec._rng(kind, salt)
    B = 2 if kind == 'other' else S_BATCH
    x, _ = cr.synth_inputs(S_ROWS, SC, SH, SW, 100 * salt + ec.SEED[kind])
    return ec.Inputs(dict(x=x, index=rng.permutation(S_ROWS)[:B].astype(np.int32),
                          dfeat=rng.normal(0, 1, (B, SO * 4 * 5)).astype(np.float32)), limits={'index': (0, S_ROWS)})


def _make_stacks(kind):
    rng = ec._rng(kind, 97)
    T = 8 if kind == 'other' else 7
    return ec.Inputs(dict(frames=ec._frames(rng, T, 520, 700), index=rng.permutation(4 * (T - 4))[:3].astype(np.int32)),
                     dict(tile_yx=np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.int32)), limits={'index': (0, 4 * (T - 4))})


STREAM_ENTRIES = [
    ec.Entry('strided_forward', 'axt_conv_trainer_forward', lambda k: _make_strided(k, 93), ec._call_conv_forward,
             handle=_strided_handle, waits_first=ec._INDEX_FIRST),
    ec.Entry('strided_step', 'axt_conv_trainer_step', lambda k: _make_strided(k, 94), ec._call_conv_step, handle=_strided_handle,
             waits_first=ec._INDEX_FIRST, fresh_handle=True),
    ec.Entry('strided_input_grad', 'axt_conv_trainer_input_grad', lambda k: _make_strided(k, 95), ec._call_conv_input_grad,
             handle=_strided_handle, prepare=ec._prepare_conv_forward),
    ec.Entry('tile_stacks', 'axt_tile_stacks', _make_stacks,
             lambda _, d, p: {'stacks': hotpath.tile_stacks(d['frames'], p['tile_yx'], d['index'])}),
    ec.Entry('trunk_features_frames', 'axt_cnn_block_features_frames', lambda k: ec._cnn_frames(k, 96, 5, 7),
             lambda det, d, p: {'feat2': det.trunk_features_frames(d['frames'], p['tile_yx'])}, handle='detector'),
]


@pytest.mark.parametrize('e', STREAM_ENTRIES, ids=repr)
def test_new_entry_points_on_a_side_stream_and_with_poison(e, weights, delay, monkeypatch):
    """tests/test_entry_conventions_gpu.py's protocols 1 to 3 for the new entry points: the decoy gives another result; on a
    side stream, behind a delay and the copy of the real input, the bytes are the default stream's; so they are with every
    allocation poisoned."""
    base = run(e, new_handle(e, weights), 'real')
    decoy = run(e, new_handle(e, weights), 'decoy')
    assert all(decoy[k].shape != base[k].shape or decoy[k].tobytes() != base[k].tobytes() for k in base)
    got, seconds, busy = side_stream_run(e, new_handle(e, weights), delay, monkeypatch)
    check(e, got, base, 'side stream')
    if e.waits_first is None:
        assert busy, f'{e}: the side stream was idle right after the call: it waited for the stream'
    for which in (1, 2):
        check(e, run(e, new_handle(e, weights), 'real', which, monkeypatch), base, f'poison {which}', which)
