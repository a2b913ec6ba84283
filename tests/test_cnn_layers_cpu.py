"""CPU side of the layer-by-layer CNN checks (tests/cnn_reference.py): the f64 reference is pinned to the reference
project's own output, the judge rejects every seeded fault and accepts a correct f32 layer, and the driver that walks a
detector's buffers is exercised on buffers made on the CPU. The GPU side is tests/test_cnn_layers_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_reference as cr
from axtrack_amd import synth
from oracle import oracle as orc

CNN_ATOL, CNN_RTOL = 1e-5, 1e-5            # the end-to-end tolerance of test_oracle_golden.py / test_gpu_parity.py


@pytest.fixture(scope='module')
def chain(weights):
    """One 512x512 tile of synth_frames through the net, layer by layer: inputs[k] is the f32 input of layer k (the
    yardstick's output of layer k-1), yard[k] / ref[k] the f32 / f64 output of layer k computed from inputs[k]."""
    fr = synth.synth_frames(5, 512, 512, seed=3)
    x = fr[None]
    inputs, yard, ref = [], [], []
    for i in range(8):
        inputs.append(x)
        yard.append(cr.yard_block(weights, i, x))
        ref.append(cr.ref_block(weights, i, x))
        x = yard[-1]
    x = x.reshape(1, -1)
    for idx, sig in cr.FC:
        inputs.append(x)
        yard.append(cr.yard_linear(weights, idx, x, sig))
        ref.append(cr.ref_linear(weights, idx, x, sig))
        x = yard[-1]
    return inputs, yard, ref


# ------------------------------------------------------------------------------------------------ the reference is the real one
def test_f64_chain_and_oracle_reproduce_the_reference_projects_output(golden, weights):
    g = golden('cnn_512')
    frames = synth.synth_frames(int(g['T_all']), int(g['H']), int(g['W']), seed=int(g['frames_seed']))
    X = np.stack([frames[t:t + 5] for t in range(2)])
    np.testing.assert_allclose(cr.ref_forward(weights, X), g['yolo'][:2], atol=CNN_ATOL, rtol=CNN_RTOL)
    np.testing.assert_allclose(orc.cnn_forward(weights, X), g['yolo'][:2], atol=CNN_ATOL, rtol=CNN_RTOL)


def test_batchnorm_edge_weights_agree_between_reference_and_oracle():
    """The edited seed-7 weights (negative gammas, running_var 1e-3 ... 10, 10x conv bias): the f64 reference and the
    oracle's f32 layer agree at f32 scale on every block, so a wrong reference is not what fails on the GPU. Found here:
    |gamma / sqrt(var + eps)| spans 0.25 ... 38, activations stay below 30 through block 7."""
    sd = cr.edge_state_dict(7)
    fr = synth.synth_frames(5, 512, 512, seed=3)
    x = fr[None]
    for i, name in enumerate(cr.NAMES):
        pre = f'ConvNet.{name}.'
        gamma, var = sd[pre + 'batchnorm.weight'], sd[pre + 'batchnorm.running_var']
        co = len(gamma)
        assert abs(int((gamma < 0).sum()) - co / 3) <= 1
        assert np.isclose(var.min(), 1e-3) and np.isclose(var.max(), 10.0)
        base = synth.synth_state_dict(7)[pre + 'conv.bias'] * np.sqrt(var / synth.synth_state_dict(7)[pre + 'batchnorm.running_var'])
        np.testing.assert_allclose(sd[pre + 'conv.bias'], 10 * base, rtol=1e-5)
        ref, yard = cr.ref_block(sd, i, x), cr.yard_block(sd, i, x)
        top = np.abs(ref).max()
        assert np.isfinite(ref).all() and top < 1e3, (i, top)
        assert np.abs(yard - ref).max() < 1e-5 * max(1.0, top), (i, np.abs(yard - ref).max(), top)
        # both signs of the fold reach the output: LeakyReLU's two branches are taken in channels of either sign
        assert (ref[:, gamma < 0] > 0).any() and (ref[:, gamma < 0] < 0).any()
        x = yard


# ------------------------------------------------------------------------------------------------ seeded faults
def _bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def bf16_terms(x, n):
    """The first n terms of the bf16 split x = hi + mid + lo (round to nearest even each time), summed in f32."""
    x = np.ascontiguousarray(x, np.float32)
    rest, total = x.copy(), np.zeros_like(x)
    for _ in range(n):
        t = _bf16(rest)
        total = total + t
        rest = rest - t
    return total


def _block_f32(sd, i, x, weight=None, bias=None, slope=None, pool_shift=0, drop_tap_col0=None):
    """Conv block i in torch f32 with one thing wrong. drop_tap_col0 = channel whose centre tap is missing in column 0."""
    cin, cout, stride, pool = cr.SPECS[i]
    pre = f'ConvNet.{cr.NAMES[i]}.'
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    w = t(sd[pre + 'conv.weight'] if weight is None else weight)
    b = t(sd[pre + 'conv.bias'] if bias is None else bias)
    z = F.conv2d(t(x), w, b, stride=stride, padding=1)
    if drop_tap_col0 is not None:
        w2 = w.clone()
        w2[drop_tap_col0, :, 1, 1] = 0
        z2 = F.conv2d(t(x), w2, b, stride=stride, padding=1)
        z[:, drop_tap_col0, :, 0] = z2[:, drop_tap_col0, :, 0]
    sc = t(sd[pre + 'batchnorm.weight']) / torch.sqrt(t(sd[pre + 'batchnorm.running_var']) + cr.BN_EPS)
    z = (z - t(sd[pre + 'batchnorm.running_mean'])[None, :, None, None]) * sc[None, :, None, None] \
        + t(sd[pre + 'batchnorm.bias'])[None, :, None, None]
    s = torch.full((cout,), cr.SLOPE) if slope is None else t(slope)
    z = torch.where(z >= 0, z, s[None, :, None, None] * z)
    if pool:
        if pool_shift:
            z = torch.cat([z[..., pool_shift:], z[..., -1:].expand(-1, -1, -1, pool_shift)], dim=-1)
        z = F.max_pool2d(z, 2, 2)
    return z.numpy()


def conv_faults(sd, i, x, yard):
    """{name: faulty f32 output of block i}: each fault applied to the yardstick's output, one at a time. Single-channel
    faults replace that channel only (computed by torch f32, itself a correct f32 layer), the others stay the yardstick's."""
    cin, cout, stride, pool = cr.SPECS[i]
    pre = f'ConvNet.{cr.NAMES[i]}.'
    ch, ch2 = 3, cout - 2
    out = {}
    f = yard.copy()
    f[:, ch, :, -1] *= np.float32(1.01)
    out['1 % on the right border column of one channel'] = f
    f = yard.copy()
    f[:, ch] = _block_f32(sd, i, x, drop_tap_col0=ch)[:, ch]
    out['one tap missing on the first column of one channel'] = f
    f = yard.copy()
    f[:, [ch, ch2]] = yard[:, [ch2, ch]]
    out['two output channels swapped'] = f
    if pool:
        out['pool taken one column to the right'] = _block_f32(sd, i, x, pool_shift=1)
    b = np.array(sd[pre + 'conv.bias'], copy=True)
    b[ch] = 0
    f = yard.copy()
    f[:, ch] = _block_f32(sd, i, x, bias=b)[:, ch]
    out["one channel's bias dropped"] = f
    if 2 <= i <= 6:
        sd2 = dict(sd)
        sd2[pre + 'conv.weight'] = bf16_terms(sd[pre + 'conv.weight'], 2)
        out['operands cut to two bf16 terms'] = cr.yard_block(sd2, i, bf16_terms(x, 2))
    slope = np.full(cout, cr.SLOPE, np.float32)
    slope[ch] = 0.01
    f = yard.copy()
    f[:, ch] = _block_f32(sd, i, x, slope=slope)[:, ch]
    out['slope 0.01 instead of 0.1 on one channel'] = f
    return out


@pytest.mark.parametrize('i', range(8))
def test_judge_rejects_every_seeded_fault_of_a_conv_block(chain, weights, i):
    """Every fault lies above the CAPS (8 max or 4 rms), not merely above today's constants: this is what keeps the caps
    honest if a constant is raised later. The yardstick itself and an independent correct f32 layer (torch's) pass at the
    default constants."""
    inputs, yard, ref = chain
    x, y, r = inputs[i], yard[i], ref[i]
    r_max, r_rms = cr.judge(y, r, y, layer=f'block {i} yardstick')
    assert r_max < 1 and r_rms < 1
    cr.judge(_block_f32(weights, i, x), r, y, layer=f'block {i} torch f32')
    faults = conv_faults(weights, i, x, y)
    assert len(faults) == 5 + (1 if cr.SPECS[i][3] else 0) + (1 if 2 <= i <= 6 else 0)
    for name, f in faults.items():
        r_max, r_rms = cr.judge(f, r, y, check=False)
        print(f'block {i}: {name}: max x{r_max:.1f} rms x{r_rms:.1f}')
        assert r_max > cr.CAP_MAX or r_rms > cr.CAP_RMS, (i, name, r_max, r_rms)
        with pytest.raises(cr.LayerMismatch, match=f'block {i} fault'):
            cr.judge(f, r, y, cr.CAP_MAX, cr.CAP_RMS, layer=f'block {i} fault')
    if 2 <= i <= 6:
        # the exact split: three bf16 terms carry all 24 bits, so the layer computed from them is the yardstick itself
        pre = f'ConvNet.{cr.NAMES[i]}.'
        sd3 = dict(weights)
        sd3[pre + 'conv.weight'] = bf16_terms(weights[pre + 'conv.weight'], 3)
        assert np.array_equal(sd3[pre + 'conv.weight'], weights[pre + 'conv.weight']) and np.array_equal(bf16_terms(x, 3), x)
        assert np.abs(cr.yard_block(sd3, i, bf16_terms(x, 3)) - y).max() == 0
        assert np.abs(cr.ref_block(sd3, i, bf16_terms(x, 3)) - r).max() == 0


def test_judge_rejects_every_seeded_fault_of_fc1(chain, weights):
    inputs, yard, ref = chain
    x, y, r = inputs[8], yard[8], ref[8]
    r_max, r_rms = cr.judge(y, r, y, layer='fc1 yardstick')
    assert r_max < 1 and r_rms < 1
    w, b = weights['fcs.1.weight'], weights['fcs.1.bias']
    t32 = (torch.from_numpy(x) @ torch.from_numpy(w).T + torch.from_numpy(b)).sigmoid().numpy()
    cr.judge(t32, r, y, layer='fc1 torch f32')
    n, n2 = 3, 1022
    faults = {}
    f = y.copy(); f[:, n] *= np.float32(1.01)
    faults['1 % on one output'] = f
    k = int(np.argmax(np.abs(x[0])))
    f = y.copy(); f[:, n] = 1 / (1 + np.exp(-(x.astype(np.float64) @ w[n].astype(np.float64) + b[n] - x[:, k].astype(np.float64) * w[n, k])))
    faults['one term of the sum missing in one output'] = f
    f = y.copy(); f[:, [n, n2]] = y[:, [n2, n]]
    faults['two outputs swapped'] = f
    f = y.copy(); f[:, n] = 1 / (1 + np.exp(-(x.astype(np.float64) @ w[n].astype(np.float64))))
    faults["one output's bias dropped"] = f
    for name, f in faults.items():
        r_max, r_rms = cr.judge(f, r, y, check=False)
        print(f'fc1: {name}: max x{r_max:.1f} rms x{r_rms:.1f}')
        assert r_max > cr.CAP_MAX or r_rms > cr.CAP_RMS, (name, r_max, r_rms)
        with pytest.raises(cr.LayerMismatch):
            cr.judge(f, r, y, cr.CAP_MAX, cr.CAP_RMS, layer='fc1 fault')


def test_every_constant_respects_the_caps():
    assert cr.BOUND_DEFAULT[0] <= cr.CAP_MAX and cr.BOUND_DEFAULT[1] <= cr.CAP_RMS
    for key, (c_max, c_rms) in cr.BOUND_OVERRIDES.items():
        assert c_max <= cr.CAP_MAX and c_rms <= cr.CAP_RMS, key
        for c, d in zip((c_max, c_rms), cr.BOUND_DEFAULT):
            assert c == d or (c > d and c == int(c)), key                 # the default, or twice the worst measured ratio rounded up


@pytest.mark.parametrize('i', [1, 3, 5])
def test_border_column_fault_is_invisible_to_the_end_to_end_tolerance(chain, weights, i):
    """Why the layer tests exist: a whole border column of one channel off by 1 % after block 1, 3 or 5, pushed through the
    rest of the net in f64, still passes the end-to-end comparison. If a later change lets the end-to-end test see these,
    this is the assertion to revisit."""
    inputs, yard, ref = chain
    clean = ref[i]
    faulty = clean.copy()
    faulty[:, 3, :, -1] *= 1.01
    assert cr.judge(faulty, clean, yard[i], check=False)[0] > 100
    a, b = cr.ref_tail(weights, i, faulty), cr.ref_tail(weights, i, clean)
    print(f'block {i}: largest change of the final grid {np.abs(a - b).max():.2e}')
    assert np.abs(a - b).max() > 0
    np.testing.assert_allclose(a, b, atol=CNN_ATOL, rtol=CNN_RTOL)


# ------------------------------------------------------------------------------------------------ the driver, on CPU-made buffers
def test_slot_maps_replay_the_chunk_loops():
    held = cr.slots_after_forward(130, 130, 128, 128)
    assert held[0][0] == 128 and held[1][1] == 129 and held[0][2] == 2 and held[0][127] == 127 and 128 not in held[0]
    assert held[3][0] == 128 and held[2][1] == 129 and held[2][5] == 5
    assert all(held[k] == {j: j for j in range(130)} for k in range(4, 10))
    held = cr.slots_after_forward(50, 24, 128, 128)
    for k in range(10):
        assert held[k] == {**{j: 24 + j for j in range(2, 24)}, 0: 48, 1: 49}
    held = cr.slots_after_forward(10, 24, 4, 8)                     # chunk_a < chunk_b < max_batch
    assert held[0] == {0: 8, 1: 9, 2: 6, 3: 7} and held[2] == {0: 8, 1: 9, **{j: j for j in range(2, 8)}}
    assert held[3] == held[2] and held[4] == {j: j for j in range(10)}
    held = cr.slots_after_chunked([(0, 5), (5, 3)], 128, 128)
    assert held[1] == {0: 5, 1: 6, 2: 7, 3: 3, 4: 4} and held[3] == held[1] and held[4] == {j: j for j in range(8)}
    assert held[9] == {j: j for j in range(8)}


@pytest.mark.parametrize('fused', [True, False])
def test_driver_walks_cpu_made_buffers_and_names_a_seeded_fault(chain, weights, fused):
    inputs, yard, ref = chain
    bufs = [a.copy() for a in yard[:10]]
    grid = yard[10].reshape(1, 12, 12, 3)

    def read(which, slot0, n):
        assert not (fused and which == 0), 'the fused front never writes block 0'
        return bufs[which][slot0:slot0 + n]

    held = cr.slots_after_forward(1, 4, 128, 128)
    lines = []
    ratios = cr.walk_layers(read, weights, inputs[0], grid, held, 'f32_direct', fused, 'cpu', log=lines.append)
    assert set(ratios) == ({'fused01'} if fused else {0, 1}) | set(range(2, 11))
    assert all(r[0] < 1 and r[1] < 1 and r[2] == 1 for r in ratios.values()) and len(lines) == len(ratios)
    bufs[3][0, 5, :, -1] *= np.float32(1.01)
    with pytest.raises(cr.LayerMismatch, match=r'conv block 3: .*item 0, channel 5, position \(y \d+, x 63\) of 64x64: map border'):
        cr.walk_layers(read, weights, inputs[0], grid, held, 'f32_direct', fused, 'cpu', log=lines.append)
