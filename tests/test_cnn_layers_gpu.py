"""Every CNN layer's activations against an f64 reference, on the GPU's own input to that layer (tests/cnn_reference.py).

Each case runs a production entry point (detect_frames, detect_axons, front_frames + back), reads back the ten buffers the
pass left in the detector (axt_debug_cnn_activation) and judges block 0 ... 7, fc1, fc2 and the returned grid one by one
at f32-rounding scale. Variants, weights, inputs and batch shapes are crossed so that every variant meets every input kind
and every batch shape, and every weight set meets every arithmetic. Run with -s to see the ratio of every (case, layer).

Items whose input buffer was overwritten by a later chunk of the same pass (batch shapes beyond chunk_a, beyond max_batch)
are judged from the first layer whose input survived (buffers 4-9 layer to layer); blocks 0-3 of those items are the same
kernels on the same inputs as in the cases that fit one chunk."""
import functools

import numpy as np
import pytest
import torch

import cnn_reference as cr
from axtrack_amd import synth
from helpers import cnn_activation, cnn_activation_rc, cnn_chunks
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

AXT_EINVAL = -22
SCATTER = [(0, 0), (1, 1), (2, 2), (0, 2), (2, 0)]          # the tile list of the fused-front test in test_gpu_parity.py
QUAD = [(0, 0), (0, 1), (1, 0), (1, 1)]
VARIANTS = {'winograd_fused': ('f32_winograd', True), 'direct_fused': ('f32_direct', True),
            'bf16x3_fused': ('bf16x3', True), 'winograd_separate': ('f32_winograd', False)}
SHAPES = ['b1_frames', 'b3_noise', 'b3_frames_x1e3', 'b4_edge_stack', 'b8_1024x1024', 'b24_700x904', 'b50_max_batch_24',
          'chunked_5_plus_3_x1e-3', 'chunk_a_700x904', 'chunk_a_plus_2_1100x1032']


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def state_dict(name):
    return cr.edge_state_dict(7) if name == 'edge7' else synth.synth_state_dict(int(name))


_detectors = {}


def detector(name, max_batch=24):
    """One detector per weight set (and batch capacity); arithmetic and front are switched on it."""
    import axtrack_amd
    if (name, max_batch) not in _detectors:
        _detectors[(name, max_batch)] = axtrack_amd.Detector(state_dict(name), max_batch=max_batch)
    return _detectors[(name, max_batch)]


def reader(det):
    return lambda which, slot0, n: cnn_activation(det, which, slot0, n)


def tiles_for(n_items, H, W):
    """A tile list whose length divides n_items, the largest the frame offers."""
    for tiles in (SCATTER, QUAD, [(0, 0), (1, 1)], [(0, 0)]):
        if n_items % len(tiles) == 0 and all(ty * 512 < H and tx * 512 < W for ty, tx in tiles):
            return tiles


@functools.lru_cache(maxsize=2)
def frames_input(T_all, H, W, seed, tiles, scale):
    frames = synth.synth_frames(T_all, H, W, seed=seed) * np.float32(scale)
    X = np.concatenate([orc.frame_tile_stack(frames, t, list(tiles)) for t in range(T_all - 4)])
    return frames, X


def run_frames(det, sd, arith, fused, label, T_all, H, W, seed, tiles, scale=1.0):
    """detect_frames over every detection frame; item = frame * n_tiles + tile (forward_items)."""
    frames, X = frames_input(T_all, H, W, seed, tuple(tiles), scale)
    det.set_arith(arith)
    det.set_fused_front(fused)
    y = det.detect_frames(dev(frames), tiles).cpu().numpy()
    n_items = (T_all - 4) * len(tiles)
    held = cr.slots_after_forward(n_items, det.max_batch, *cnn_chunks())
    return cr.walk_layers(reader(det), sd, X, y.reshape(n_items, 12, 12, 3), held, arith, fused and W % 4 == 0, label)


def run_tensor(det, sd, arith, fused, label, X):
    det.set_arith(arith)
    det.set_fused_front(fused)
    y = det.detect_axons(dev(X)).cpu().numpy()
    held = cr.slots_after_forward(len(X), det.max_batch, *cnn_chunks())
    return cr.walk_layers(reader(det), sd, X, y, held, arith, fused, label)


def edge_stack():
    """The suite's edge inputs (test_cnn_conv_stack_against_oracle_on_edge_inputs): zeros, ones, 50.0 in the four corners
    and the centre, frames x3."""
    X = np.zeros((4, 5, 512, 512), np.float32)
    X[1] = 1.0
    for c, (yy, xx) in enumerate([(0, 0), (0, 511), (511, 0), (511, 511), (255, 256)]):
        X[2, c, yy, xx] = 50.0
    X[3] = synth.synth_frames(5, 512, 512, seed=9) * 3
    return X


@pytest.mark.parametrize('shape,variant', [(s, v) for s in SHAPES for v in VARIANTS])
def test_every_layer_of_every_item(shape, variant):
    arith, fused = VARIANTS[variant]
    sd = state_dict('42')
    chunk_a, chunk_b = cnn_chunks()
    label = f'{shape}/{variant}'
    if shape == 'b1_frames':
        run_frames(detector('42'), sd, arith, fused, label, 5, 512, 512, 11, [(0, 0)])
    elif shape == 'b3_noise':                            # dense signed noise: no zeros, negative pixels
        X = (synth.normal(77, (3, 5, 512, 512)) * 2).astype(np.float32)
        run_tensor(detector('42'), sd, arith, fused, label, X)
    elif shape == 'b3_frames_x1e3':                      # the relative error of the bf16 split / Winograd's transforms at 1e3 ...
        run_frames(detector('42'), sd, arith, fused, label, 7, 512, 512, 12, [(0, 0)], scale=1e3)
    elif shape == 'b4_edge_stack':
        run_tensor(detector('42'), sd, arith, fused, label, edge_stack())
    elif shape == 'b8_1024x1024':                        # 2 frames x 4 tiles: two workgroups per CU in the stride-2 kernels
        run_frames(detector('42'), sd, arith, fused, label, 6, 1024, 1024, 13, QUAD)
    elif shape == 'b24_700x904':                         # tiles cut at the bottom and at the right; exactly max_batch items
        run_frames(detector('42'), sd, arith, fused, label, 10, 700, 904, 14, QUAD)
    elif shape == 'b50_max_batch_24':                    # three groups of max_batch; the buffers hold items 26 ... 49
        ratios = run_frames(detector('42'), sd, arith, fused, label, 14, 1100, 1032, 15, SCATTER)
        assert ratios[5][2] == 24 and ratios[10][2] == 24
    elif shape == 'chunked_5_plus_3_x1e-3':              # ... and at 1e-3, through the chunked API
        frames, X = frames_input(12, 512, 512, 16, ((0, 0),), 1e-3)
        det = detector('42')
        det.set_arith(arith)
        det.set_fused_front(fused)
        fr = dev(frames)
        det.front_frames(fr, [(0, 0)], 0, 5, 0)
        det.front_frames(fr, [(0, 0)], 5, 3, 5)
        y = det.back(8, 1).cpu().numpy().reshape(8, 12, 12, 3)
        held = cr.slots_after_chunked([(0, 5), (5, 3)], chunk_a, chunk_b)
        ratios = cr.walk_layers(reader(det), sd, X, y, held, arith, fused, label)
        # block 2 is judged for the items that buffer 2 and its input, buffer 1, both still hold: with chunks of 5 or more
        # items 3 .. 7, blocks 0-3 of items 0-2 having been overwritten by the second call
        kept = len(set(held[2].values()) & set(held[1].values()))
        assert ratios[10][2] == 8 and ratios[2][2] == kept and (kept == 5 or min(chunk_a, chunk_b) < 5)
    elif shape == 'chunk_a_700x904':                     # exactly one full chunk
        n = chunk_a
        tiles = tiles_for(n, 700, 904)
        ratios = run_frames(detector('42', chunk_a + 2), sd, arith, fused, label, 4 + n // len(tiles), 700, 904, 17, tiles)
        assert ratios[2][2] == n and ratios[10][2] == n
    elif shape == 'chunk_a_plus_2_1100x1032':            # the second chunk lands in slots 0-1 of buffers 0-3, buffers 4-9 hold all
        n = chunk_a + 2
        tiles = tiles_for(n, 1100, 1032)
        ratios = run_frames(detector('42', chunk_a + 2), sd, arith, fused, label, 4 + n // len(tiles), 1100, 1032, 18, tiles)
        assert ratios[10][2] == n and ratios[5][2] == n
        if chunk_a == chunk_b:
            assert ratios[2][2] == n - 2 and ratios[4][2] == n - 2            # items 0, 1: blocks 0-4 not judged here


@pytest.mark.parametrize('name', ['7', '1234', 'edge7'])
def test_every_weight_set_under_every_arithmetic(name):
    """Seeds 7 and 1234, and seed 7 with BatchNorm edges (negative gammas, running_var 1e-3 ... 10, 10x conv bias:
    cnn_reference.edge_state_dict): the sign and the scale of the BN fold, in every arithmetic and both fronts."""
    sd = state_dict(name)
    det = detector(name)
    for arith, fused in [('f32_winograd', True), ('f32_direct', True), ('bf16x3', True), ('f32_winograd', False)]:
        run_frames(det, sd, arith, fused, f'weights_{name}/{arith}/{"fused" if fused else "separate"}', 7, 512, 512, 21, [(0, 0)])


def test_width_not_a_multiple_of_4_takes_the_repitch_path():
    """530 x 701: rows are not 16-byte aligned, so both front settings run the separate stride-2 kernels on a re-pitched
    copy (block 0 is observable in both) and the tiles are cut at the bottom and at the right."""
    sd = state_dict('42')
    det = detector('42')
    for arith, fused in [('f32_winograd', True), ('f32_winograd', False), ('f32_direct', True), ('bf16x3', False)]:
        ratios = run_frames(det, sd, arith, fused, f'repitch_530x701/{arith}/set_{"fused" if fused else "separate"}', 6, 530, 701, 17, QUAD)
        assert 0 in ratios and 'fused01' not in ratios


def test_read_back_refuses_what_it_cannot_deliver():
    """AXT_EINVAL for slots beyond a buffer and for block 0 after a fused pass; never stale data."""
    chunk_a, chunk_b = cnn_chunks()
    det = detector('42')
    frames, X = frames_input(5, 512, 512, 11, ((0, 0),), 1.0)
    det.set_arith('f32_winograd')
    det.set_fused_front(False)
    det.detect_frames(dev(frames), [(0, 0)])
    rc, a0 = cnn_activation_rc(det, 0, 0, 1)
    assert rc == 0 and a0.shape == (1, 20, 256, 256)
    cr.judge(a0, cr.ref_block(state_dict('42'), 0, X), cr.yard_block(state_dict('42'), 0, X), layer='block 0')
    det.set_fused_front(True)
    assert cnn_activation_rc(det, 0, 0, 1)[0] == 0                    # the setting alone changes nothing: the last pass wrote it
    det.detect_frames(dev(frames), [(0, 0)])
    assert cnn_activation_rc(det, 0, 0, 1)[0] == AXT_EINVAL
    assert cnn_activation_rc(det, 1, 0, 1)[0] == 0
    caps = [min(det.max_batch, chunk_a)] * 2 + [min(det.max_batch, chunk_b)] * 2 + [det.max_batch] * 6
    for which in range(1, 10):
        assert cnn_activation_rc(det, which, caps[which] - 1, 1)[0] == 0
        assert cnn_activation_rc(det, which, caps[which] - 1, 2)[0] == AXT_EINVAL
        assert cnn_activation_rc(det, which, caps[which], 1)[0] == AXT_EINVAL
        assert cnn_activation_rc(det, which, -1, 1)[0] == AXT_EINVAL
    assert cnn_activation_rc(det, 10, 0, 1)[0] == AXT_EINVAL and cnn_activation_rc(det, -1, 0, 1)[0] == AXT_EINVAL


def test_entry_points_over_one_body_give_the_same_bytes():
    """axt_cnn_features_frames is axt_cnn_block_features_frames(block = 7), and front_frames + back walk the chunks that
    detect_frames walks: one 512 x 512 tile, the first pair on one item, the second on three items in two front calls."""
    det = detector('42')
    det.set_arith('f32_winograd')
    det.set_fused_front(True)
    frames = dev(synth.synth_frames(7, 512, 512, seed=23))
    tiles = np.zeros((1, 2), np.int32)
    a, b = (torch.full((1, 160 * 16 * 16), float('nan'), device='cuda') for _ in range(2))
    with torch.cuda.device(det.device):
        assert det._lib.axt_cnn_features_frames(det._h, frames.data_ptr(), 5, 512, 512, 0, 1, tiles.ctypes.data, 1, a.data_ptr(), None) == 0
        assert det._lib.axt_cnn_block_features_frames(det._h, frames.data_ptr(), 5, 512, 512, 0, 1, tiles.ctypes.data, 1, 7,
                                                      b.data_ptr(), None) == 0
        torch.cuda.synchronize()
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and bool(a.any())
    whole = det.detect_frames(frames, tiles)
    assert tuple(whole.shape) == (3, 1, 12, 12, 3)
    det.front_frames(frames, tiles, 0, 2, 0)
    det.front_frames(frames, tiles, 2, 1, 2)
    assert torch.equal(det.back(3, 1), whole)
