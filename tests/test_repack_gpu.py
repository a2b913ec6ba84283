"""Device-side weight packing (axtrack_amd/csrc/repack.hip) through the production wrappers:
Detector.load_conv_block / load_linear / load_state_dict and the trainers' export_to.

The contract is byte identity with the host packers. So the reference of every test is a Detector CREATED from the same
tensors (axt_detector_create: pack_conv, pack_wino, pack_bf16x3 and the linear transposes on the host), never the code
under test, and "equal" is torch.equal on three taps of the forward pass -- features_frames(block=7),
trunk_features_frames(block=2) and the YOLO grids -- with no tolerance: the inference kernels are deterministic, so equal
images give equal bytes, and a wrong weight anywhere in a block changes the taps behind it.

Two state dicts, A and B (synth, two seeds), with BatchNorm tensors that make the fold matter: running_var in 0.3..3 and
batchnorm.weight of both signs. One input: a single 512 x 512 tile, 5 frames, one item.

A note on the Winograd image: axt_detector_create always ends in the default arithmetic, so every detector has its Winograd
image from the start and a load refreshes it in place; the image that is still missing at a load, and is packed from the
device copy of the folded weights by a LATER set_arith, is the bf16x3 one. Both orders are tested for it; for Winograd the
detector is created in 'f32_direct', loaded while its Winograd image lies unused, and switched afterwards."""
import time

import numpy as np
import pytest
import torch

import test_entry_conventions_gpu as proto
from axtrack_amd import _lib, hotpath, synth, training
from axtrack_amd.hotpath import Detector, conv_block_key, state_dict_tensor_order

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TILES = [(0, 0)]
ARITHS = ('f32', 'f32_direct', 'bf16x3')
CONV_KEYS = ('conv.weight', 'conv.bias', 'batchnorm.weight', 'batchnorm.bias', 'batchnorm.running_mean',
             'batchnorm.running_var')
FC = ('fcs.1', 'fcs.3', 'fcs.5')


def make_state_dict(seed):
    """synth's state dict with BatchNorm tensors that are far from the identity: var in 0.3..3, gamma of both signs."""
    sd = dict(synth.synth_state_dict(seed))
    rng = np.random.default_rng(seed)
    for i in range(8):
        k = conv_block_key(i)
        co = sd[f'{k}.batchnorm.weight'].shape[0]
        sign = np.where(rng.random(co) < 0.5, -1.0, 1.0)
        sd[f'{k}.batchnorm.weight'] = (sign * rng.uniform(0.5, 1.5, co)).astype(np.float32)
        sd[f'{k}.batchnorm.running_var'] = rng.uniform(0.3, 3.0, co).astype(np.float32)
    return sd


def block_tensors(sd, i):
    return [sd[f'{conv_block_key(i)}.{k}'] for k in CONV_KEYS]


def linear_tensors(sd, layer):
    return [sd[f'{FC[layer]}.weight'], sd[f'{FC[layer]}.bias']]


def on_device(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(sd[k], np.float32)).to(DEV) for k in state_dict_tensor_order()}


def taps(det, frames):
    """The three outputs "equal" is about, in the detector's present arithmetic and front."""
    return (det.features_frames(frames, TILES, block=7).clone(), det.trunk_features_frames(frames, TILES, block=2).clone(),
            det.detect_frames(frames, TILES).clone())


def all_taps(det, frames, fronts=(True, False)):
    """taps() in every arithmetic, with the fused front on and off. Leaves the detector in 'f32' with the fused front."""
    out = {}
    for arith in ARITHS:
        det.set_arith(arith)
        for fused in fronts:
            det.set_fused_front(fused)
            out[arith, fused] = taps(det, frames)
    det.set_arith('f32')
    det.set_fused_front(True)
    return out


def assert_equal(got, ref, what):
    if isinstance(got, dict):
        assert set(got) == set(ref)
        for k in got:
            assert_equal(got[k], ref[k], f'{what} {k}')
        return
    for name, g, r in zip(('features(block=7)', 'trunk_features(block=2)', 'yolo'), got, ref):
        assert g.shape == r.shape and torch.equal(g, r), \
            f'{what}: {name} differs in {int((g != r).sum())} of {g.numel()} values, max |d| = {float((g - r).abs().max())}'


@pytest.fixture(scope='module')
def sds():
    return make_state_dict(11), make_state_dict(12)


@pytest.fixture(scope='module')
def dev_b(sds):
    return on_device(sds[1])


@pytest.fixture(scope='module')
def frames():
    return torch.from_numpy(synth.synth_frames(5, 512, 512, seed=3)).to(DEV)


@pytest.fixture(scope='module')
def reference(frames):
    """all_taps of a detector created on the host from a state dict, computed once per dict."""
    cache = {}

    def get(name, sd):
        if name not in cache:
            cache[name] = all_taps(Detector(sd, max_batch=1, device=DEV), frames)
        return cache[name]
    return get


def load_all(det, dev_sd):
    for i in range(8):
        det.load_conv_block(i, *block_tensors(dev_sd, i))
    for layer in range(3):
        det.load_linear(layer, *linear_tensors(dev_sd, layer))


def test_fixtures_are_what_the_tests_need(sds, frames, reference):
    for sd in sds:
        for i in range(8):
            g, v = sd[f'{conv_block_key(i)}.batchnorm.weight'], sd[f'{conv_block_key(i)}.batchnorm.running_var']
            assert (g > 0).any() and (g < 0).any() and v.min() >= 0.3 and v.max() <= 3.0
    a, b = reference('A', sds[0]), reference('B', sds[1])
    for k in a:                                             # A and B differ in every tap: a load that did nothing shows
        assert all(not torch.equal(x, y) for x, y in zip(a[k], b[k])), k
        assert all(bool(torch.isfinite(x).all()) for x in b[k])


# ------------------------------------------------------------------------------------------------ 1. full device load
def test_full_device_load_equals_a_detector_created_from_the_same_tensors(sds, dev_b, frames, reference):
    det = Detector(sds[0], max_batch=1, device=DEV)
    before = det.device_bytes
    assert_equal(all_taps(det, frames), reference('A', sds[0]), 'before the load')     # every image exists from here on
    with_images = det.device_bytes
    load_all(det, dev_b)
    assert det.state_dict_source is None
    folded = sum(ci * co * 9 * 4 for ci, co in hotpath.CONV_CHANNELS)
    assert det.device_bytes == with_images + folded and with_images > before
    assert_equal(all_taps(det, frames), reference('B', sds[1]), 'after load_conv_block x 8 + load_linear x 3')
    det.load_state_dict(on_device(sds[0]))                  # and back, through load_state_dict: nothing new is allocated
    assert det.device_bytes == with_images + folded
    assert_equal(all_taps(det, frames), reference('A', sds[0]), 'after load_state_dict')


# ------------------------------------------------------------------------------------------------ 2. each block alone
PIECES = [('conv', i) for i in range(8)] + [('linear', l) for l in range(3)]


@pytest.mark.parametrize('kind,i', PIECES, ids=[f'{k}{i}' for k, i in PIECES])
def test_one_block_alone(kind, i, sds, dev_b, frames):
    """conv0: cin 5, stride-2 layout; conv1: cout 40, ngp padded to 12; conv7: cout 160, two Winograd groups, no bf16x3
    image; linear2: 432 outputs in 448 columns. The detector has never been in bf16x3 when the block is loaded, so that
    image is packed afterwards: from the device copy for the loaded block, from the host copy for the others."""
    sd_a, sd_b = sds
    mixed = dict(sd_a)
    keys = [f'{conv_block_key(i)}.{k}' for k in CONV_KEYS] if kind == 'conv' else [f'{FC[i]}.weight', f'{FC[i]}.bias']
    mixed.update({k: sd_b[k] for k in keys})
    det = Detector(sd_a, max_batch=1, device=DEV)
    if kind == 'conv':
        det.load_conv_block(i, *block_tensors(dev_b, i))
    else:
        det.load_linear(i, *linear_tensors(dev_b, i))
    assert det.state_dict_source is None
    ref = all_taps(Detector(mixed, max_batch=1, device=DEV), frames)
    assert_equal(all_taps(det, frames), ref, f'{kind} {i} loaded alone')


# ------------------------------------------------------------------------------------------------ 3. lazy packing
def test_images_packed_after_a_load(sds, dev_b, frames, reference):
    ref = reference('B', sds[1])
    det = Detector(sds[0], max_batch=1, device=DEV)         # never in bf16x3
    bytes0 = det.device_bytes
    load_all(det, dev_b)
    bytes1 = det.device_bytes
    det.set_arith('bf16x3')
    assert det.device_bytes > bytes1 > bytes0
    assert_equal(taps(det, frames), ref['bf16x3', True], 'bf16x3 packed after the load')
    det = Detector(sds[0], max_batch=1, device=DEV, arith='f32_direct')     # its Winograd image has never been used
    load_all(det, dev_b)
    assert_equal(taps(det, frames), ref['f32_direct', True], 'f32_direct right after the load')
    det.set_arith('f32')
    assert_equal(taps(det, frames), ref['f32', True], 'f32 Winograd switched to after the load')


# ------------------------------------------------------------------------------------------------ 4. trainer exports
def _train_inputs(det):
    """Two items (two detection frames of one tile) with a few labels: what the trainers of one case read."""
    frames = torch.from_numpy(synth.synth_frames(6, 512, 512, seed=7)).to(DEV)
    labels = [([100, 300, 420], [80, 256, 400]), ([120, 310], [90, 250])]
    targets = training.yolo_targets(labels, TILES, device=DEV).reshape(-1, hotpath.S, hotpath.S, 4)
    return frames, targets


@pytest.mark.parametrize('which,batch_stats', [('head', False), ('block7', False), ('block7', True), ('trunk8', False),
                                               ('trunk8', True)])
def test_trainer_exports(which, batch_stats, sds, frames):
    sd_a = sds[0]
    det = Detector(sd_a, max_batch=2, device=DEV)
    tframes, targets = _train_inputs(det)
    P = dict(LR=0.01)                                       # large steps: two of them move every tensor visibly
    idx = np.arange(2, dtype=np.int32)
    rows = torch.arange(2, dtype=torch.int32, device=DEV)
    head = training.HeadTrainer(sd_a, P, max_batch=2, device=DEV)
    if which == 'head':
        trunk, table = None, det.features_frames(tframes, TILES)
    elif which == 'block7':
        trunk = training.ConvBlockTrainer(sd_a, training.LAST_CONV_BLOCK, P, max_batch=2, device=DEV, batch_stats=batch_stats)
        table = det.features_frames(tframes, TILES, block=6)
    else:
        trunk = training.ConvTrunkTrainer(sd_a, 0, 8, P, max_batch=2, device=DEV, batch_stats=batch_stats)
        table = hotpath.tile_stacks(tframes, TILES, idx).view(2, -1)
    for _ in range(2):
        feats = trunk.forward(table, rows) if trunk else table
        yolo = head.forward(feats, rows)
        _, dy = head.loss(yolo, targets, idx)
        if trunk:
            dfeat = head.input_grad(dy)
            (trunk.step if which == 'block7' else trunk.backward_and_step)(table, rows, dfeat)
        head.step(feats, rows, dy)
    head.export_to(det)
    if which == 'block7':
        trunk.export_to(det, 7)
    elif trunk:
        trunk.export_to(det)
    assert det.state_dict_source is None
    trained = trunk.state_dict(head.state_dict()) if trunk else head.state_dict()
    changed = [k for k in state_dict_tensor_order() if not np.array_equal(np.asarray(trained[k]), sd_a[k])]
    expect = 6 + (0 if trunk is None else (4 + 2 * batch_stats) * (1 if which == 'block7' else 8))
    assert len(changed) == expect, changed                  # the steps moved every tensor that is exported
    ref = all_taps(Detector(trained, max_batch=1, device=DEV), frames, fronts=(True,))
    assert_equal(all_taps(det, frames, fronts=(True,)), ref, f'{which} exported (batch_stats={batch_stats})')


def test_export_refuses_a_trainer_of_another_shape(sds):
    det = Detector(sds[0], max_batch=1, device=DEV)
    blk = training.ConvBlockTrainer(sds[0], training.LAST_CONV_BLOCK, max_batch=1, device=DEV)
    for block in (6, 0):                                    # 80 -> 160 is neither block 6 (80 -> 80) nor block 0 (stride 2)
        with pytest.raises(ValueError, match='axt_conv_trainer_export'):
            blk.export_to(det, block)
    with pytest.raises(IndexError):
        blk.export_to(det, 8)
    with pytest.raises(TypeError):
        blk.export_to(object())
    assert det.state_dict_source is sds[0]


# ------------------------------------------------------------------------------------------------ 5. side stream, poison
@pytest.fixture(scope='module')
def delay():
    return proto.Delay()


@pytest.mark.parametrize('b3_allocated', [True, False], ids=['bf16x3_image_allocated', 'bf16x3_image_missing'])
def test_load_on_a_side_stream_with_poisoned_allocations(b3_allocated, sds, dev_b, frames, reference, delay, monkeypatch):
    """The side-stream protocol of tests/test_entry_conventions_gpu.py for the loads: the device tensors hold the decoy (A);
    on a non-blocking side stream a delay, a copy of the real tensors (B) into them, and the loads are enqueued in that
    order, then the forward pass. A launch on any other stream runs during the delay and packs the decoy. Allocations are
    poisoned during the calls. With the bf16x3 image missing, the set_arith after the load has to wait for the side stream
    itself before it packs from the device copy."""
    sd_a, sd_b = sds
    ref = reference('B', sd_b)
    det = Detector(sd_a, max_batch=1, device=DEV)
    if b3_allocated:
        det.set_arith('bf16x3')
        det.set_arith('f32')
    bufs = on_device(sd_a)
    load_all(det, bufs)                                     # A into A: the first load's allocations and kernel loads
    assert_equal(taps(det, frames), reference('A', sd_a)['f32', True], 'A loaded into A')
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        delay.enqueue()
        for k in bufs:
            bufs[k].copy_(dev_b[k], non_blocking=True)
        t0 = time.perf_counter()
        with proto.poisoned_allocations(monkeypatch, 1):
            load_all(det, bufs)
        seconds = time.perf_counter() - t0
        busy = not side.query()
        got = taps(det, frames)
        side.synchronize()
    print(f'\n{seconds * 1e3:.2f} ms to enqueue 11 loads behind a delay of {delay.ms:.1f} ms')
    assert busy, 'the loads waited for the stream'
    assert seconds * 1e3 <= delay.ms / proto.MARGIN
    assert_equal(got, ref['f32', True], 'loaded on the side stream')
    det.set_arith('bf16x3')                                 # on the default stream, right behind the side stream's work
    assert_equal(taps(det, frames), ref['bf16x3', True], 'bf16x3 after the side-stream load')


# ------------------------------------------------------------------------------------------------ 6. errors
def test_bad_arguments_raise_before_anything_is_launched(sds, dev_b, frames, reference):
    sd_a = sds[0]
    det = Detector(sd_a, max_batch=1, device=DEV)
    t = block_tensors(dev_b, 3)
    with pytest.raises(IndexError):
        det.load_conv_block(8, *t)
    with pytest.raises(IndexError):
        det.load_linear(3, *linear_tensors(dev_b, 2))
    for pos in range(6):
        for bad in (t[pos].cpu(), t[pos].double(), t[pos][..., None], t[pos].repeat_interleave(2, 0)[::2],
                    t[pos].cpu().numpy()):
            args = list(t)
            args[pos] = bad
            with pytest.raises((ValueError, TypeError)):
                det.load_conv_block(3, *args)
    with pytest.raises(ValueError, match='shape'):
        det.load_conv_block(2, *t)                          # block 3's tensors are not block 2's
    w, b = linear_tensors(dev_b, 2)
    for args in ((w.cpu(), b), (w, b.cpu()), (w.t().contiguous(), b), (w.t().contiguous().t(), b), (w, b[:-1])):
        with pytest.raises(ValueError):
            det.load_linear(2, *args)
    incomplete = dict(dev_b)
    del incomplete['fcs.5.bias']
    with pytest.raises(KeyError):
        det.load_state_dict(incomplete)
    wrong_last = dict(dev_b, **{'fcs.5.bias': dev_b['fcs.5.bias'].cpu()})
    with pytest.raises(ValueError):
        det.load_state_dict(wrong_last)                     # refused before the first block is loaded
    lib = _lib.load()
    p = [x.data_ptr() for x in t]
    assert lib.axt_detector_load_conv_block(det._h, 8, *p, None) == -22 and b'not in 0..7' in lib.axt_last_error()
    assert lib.axt_detector_load_conv_block(det._h, -1, *p, None) == -22
    for pos in range(6):
        assert lib.axt_detector_load_conv_block(det._h, 3, *(p[:pos] + [None] + p[pos + 1:]), None) == -22
    assert lib.axt_detector_load_linear(det._h, 3, w.data_ptr(), b.data_ptr(), None) == -22
    assert lib.axt_detector_load_linear(det._h, 0, None, b.data_ptr(), None) == -22
    assert det.state_dict_source is sd_a                    # nothing was loaded
    assert_equal(taps(det, frames), reference('A', sd_a)['f32', True], 'after the refused calls')
