"""What the device-side weight packing (csrc/repack.hip) rests on, checked without a GPU: the fold formula
the byte tests of tests/test_repack_gpu.py take from the host packers, the declarations, and every refusal that needs no
device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import axtrack_amd
from axtrack_amd import _lib, hotpath, training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = {'axt_detector_load_conv_block', 'axt_detector_load_linear', 'axt_conv_trainer_export', 'axt_head_trainer_export'}
AXT_EINVAL = -22


# ------------------------------------------------------------------------------------------------ the fold formula
def fold(w, b, gamma, beta, mean, var):
    """pack_conv's BatchNorm fold restated: f64, sc = gamma / sqrt(var + 1e-5), w' = w * sc, b' = (b - mean) * sc + beta."""
    w, b, gamma, beta, mean, var = (np.asarray(a, np.float64) for a in (w, b, gamma, beta, mean, var))
    sc = gamma / np.sqrt(var + 1e-5)
    return w * sc[:, None, None, None], (b - mean) * sc + beta


@pytest.mark.parametrize('stride', [1, 2])
def test_fold_formula_is_conv_then_batchnorm_in_eval_mode(stride):
    Co, Ci = 3, 2
    rng = np.random.default_rng(5)
    w, b = rng.normal(size=(Co, Ci, 3, 3)), rng.normal(size=Co)
    gamma = np.array([1.3, -0.7, 0.9])                      # both signs
    beta, mean, var = rng.normal(size=Co), rng.normal(size=Co), np.array([0.3, 1.1, 3.0])
    x = torch.from_numpy(rng.normal(size=(2, Ci, 7, 6)))
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ref = torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, t(w), t(b), stride=stride, padding=1), t(mean), t(var),
                                         t(gamma), t(beta), training=False, eps=1e-5)
    wf, bf = fold(w, b, gamma, beta, mean, var)
    got = torch.nn.functional.conv2d(x, t(wf), t(bf), stride=stride, padding=1)
    assert got.shape == ref.shape and float((got - ref).abs().max()) < 1e-12
    # the formula does matter on this case: the unfolded convolution is far away
    assert float((torch.nn.functional.conv2d(x, t(w), t(b), stride=stride, padding=1) - ref).abs().max()) > 0.1


def test_fold_is_rounded_once():
    """f64 throughout and one rounding to f32: folding in f32 gives other bytes on ordinary values, which is why the device
    kernels compute in f64 like the host."""
    rng = np.random.default_rng(6)
    w = rng.normal(size=(3, 2, 3, 3)).astype(np.float32)
    b, gamma, beta, mean = (rng.normal(size=3).astype(np.float32) for _ in range(4))
    var = rng.uniform(0.3, 3, 3).astype(np.float32)
    wf, bf = fold(w, b, gamma, beta, mean, var)
    sc32 = gamma / np.sqrt(var + np.float32(1e-5))
    assert (wf.astype(np.float32) != w * sc32[:, None, None, None]).any()
    assert np.abs(wf.astype(np.float32) - w * sc32[:, None, None, None]).max() < 1e-6


# ------------------------------------------------------------------------------------------------ declarations
def test_new_header_declares_and_binds_the_new_names():
    header = open(os.path.join(ROOT, 'include', 'axtrack_hip_repack.h')).read()
    assert set(re.findall(r'^int (axt_\w+)\s*\(', header, re.M)) == NEW_NAMES
    main = open(os.path.join(ROOT, 'include', 'axtrack_hip.h')).read()
    assert re.search(r'^#include "axtrack_hip_repack.h"$', main, flags=re.M)
    assert not any(re.search(rf'\b{n}\s*\(', main) for n in NEW_NAMES)
    lib = _lib.load()
    assert lib.axt_abi_version() == 1
    for n in NEW_NAMES:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert 'repack.hip' in open(os.path.join(ROOT, 'axtrack_amd', 'csrc', 'Makefile')).read()


def test_python_surface():
    for cls, names in ((hotpath.Detector, ('load_conv_block', 'load_linear', 'load_state_dict')),
                       (training.HeadTrainer, ('export_to',)), (training.ConvBlockTrainer, ('export_to',)),
                       (training.ConvStageTrainer, ('export_to',)), (training.ConvTrunkTrainer, ('export_to',))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert list(inspect.signature(hotpath.Detector.load_conv_block).parameters) == [
        'self', 'i', 'weight', 'bias', 'bn_weight', 'bn_bias', 'running_mean', 'running_var']
    assert list(inspect.signature(hotpath.Detector.load_linear).parameters) == ['self', 'layer', 'weight', 'bias']
    for f in (axtrack_amd.fine_tune_head, axtrack_amd.fine_tune_detector):
        assert inspect.signature(f).parameters['test_loss'].default is False
    assert hotpath.CONV_CHANNELS[0] == (5, 20) and hotpath.CONV_CHANNELS[7] == (80, 160) and len(hotpath.CONV_CHANNELS) == 8
    assert all(a[1] == b[0] for a, b in zip(hotpath.CONV_CHANNELS, hotpath.CONV_CHANNELS[1:]))
    assert hotpath.LINEAR_SHAPES == ((40960, 1024), (1024, 1024), (1024, 432))


# ------------------------------------------------------------------------------------------------ refusals, no device
def test_entry_points_refuse_bad_arguments_before_any_device_call():
    lib = _lib.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data                                     # (never dereferenced: the checks come first)
    fake = ctypes.c_void_p(p)
    six = [p] * 6
    assert lib.axt_detector_load_conv_block(None, 0, *six, None) == AXT_EINVAL
    assert b'axt_detector_load_conv_block' in lib.axt_last_error()
    for li in (-1, 8, 100):
        assert lib.axt_detector_load_conv_block(fake, li, *six, None) == AXT_EINVAL
        assert b'not in 0..7' in lib.axt_last_error()
    for pos in range(6):
        assert lib.axt_detector_load_conv_block(fake, 0, *(six[:pos] + [None] + six[pos + 1:]), None) == AXT_EINVAL
        assert b'null argument' in lib.axt_last_error()
    assert lib.axt_detector_load_linear(None, 0, p, p, None) == AXT_EINVAL
    assert lib.axt_detector_load_linear(fake, 0, None, p, None) == AXT_EINVAL
    assert lib.axt_detector_load_linear(fake, 0, p, None, None) == AXT_EINVAL
    for layer in (-1, 3):
        assert lib.axt_detector_load_linear(fake, layer, p, p, None) == AXT_EINVAL
        assert b'not in 0..2' in lib.axt_last_error()
    assert lib.axt_conv_trainer_export(None, fake, 0, None) == AXT_EINVAL
    assert lib.axt_conv_trainer_export(fake, None, 0, None) == AXT_EINVAL
    for li in (-1, 8):
        assert lib.axt_conv_trainer_export(fake, fake, li, None) == AXT_EINVAL
        assert b'axt_conv_trainer_export' in lib.axt_last_error()
    assert lib.axt_head_trainer_export(None, fake, None) == AXT_EINVAL
    assert lib.axt_head_trainer_export(fake, None, None) == AXT_EINVAL
    assert b'axt_head_trainer_export' in lib.axt_last_error()
    assert not buf.any()


def _detector_shell(device):
    """A Detector without a handle: the checks of the loads come before the handle is touched."""
    det = hotpath.Detector.__new__(hotpath.Detector)
    det.device = torch.device(device)
    det.state_dict_source = 'unchanged'
    return det


def test_loads_check_their_tensors_before_any_launch():
    det = _detector_shell('cuda:0')
    good = [torch.zeros(80, 80, 3, 3)] + [torch.zeros(80)] * 5
    for i in (8, -1, 1.0, True, None):
        with pytest.raises(IndexError):
            det.load_conv_block(i, *good)
    for layer in (3, -1, False):
        with pytest.raises(IndexError):
            det.load_linear(layer, torch.zeros(432, 1024), torch.zeros(432))
    with pytest.raises(ValueError, match='is on cpu'):      # CPU tensors for a detector on the GPU
        det.load_conv_block(3, *good)
    with pytest.raises(ValueError, match='is on cpu'):
        det.load_linear(2, torch.zeros(432, 1024), torch.zeros(432))
    with pytest.raises(TypeError):
        det.load_conv_block(3, good[0].numpy(), *good[1:])
    # shape, dtype and layout: on a shell that says 'cpu', so that the device check passes and the next ones are reached
    det = _detector_shell('cpu')
    for pos in range(6):
        for bad, what in ((good[pos].double(), 'float32'), (good[pos][..., None], 'shape'), (good[pos][:40], 'shape'),
                          (good[pos].repeat_interleave(2, 0)[::2], 'contiguous')):
            args = list(good)
            args[pos] = bad
            with pytest.raises(ValueError, match=what):
                det.load_conv_block(3, *args)
    with pytest.raises(ValueError, match='shape'):
        det.load_conv_block(7, *good)                       # block 7 is 80 -> 160
    w = torch.zeros(432, 1024)
    for args, what in (((w.t().contiguous(), torch.zeros(432)), 'shape'), ((w, torch.zeros(448)), 'shape'),
                       ((torch.zeros(1024, 432).t(), torch.zeros(432)), 'contiguous'), ((w.half(), torch.zeros(432)), 'float32')):
        with pytest.raises(ValueError, match=what):
            det.load_linear(2, *args)
    with pytest.raises(KeyError, match='state_dict lacks'):
        det.load_state_dict({})
    sd = {}
    for i, (ci, co) in enumerate(hotpath.CONV_CHANNELS):
        for k, t in zip(('conv.weight', 'conv.bias', 'batchnorm.weight', 'batchnorm.bias', 'batchnorm.running_mean',
                         'batchnorm.running_var'), [torch.zeros(co, ci, 3, 3)] + [torch.zeros(co)] * 5):
            sd[f'{hotpath.conv_block_key(i)}.{k}'] = t
    for name, (fin, fout) in zip(('fcs.1', 'fcs.3', 'fcs.5'), ((8, 4), (4, 4), (4, 2))):      # (small stand-ins: refused)
        sd[f'{name}.weight'], sd[f'{name}.bias'] = torch.zeros(fout, fin), torch.zeros(fout)
    assert set(sd) == set(hotpath.state_dict_tensor_order())
    with pytest.raises(ValueError, match='linear 0'):
        det.load_state_dict(sd)                             # the last tensors are wrong: refused before the first block is loaded
    assert det.state_dict_source == 'unchanged'


def test_test_loss_is_refused_without_a_labelled_test_timelapse():
    class Tl:
        frame_sharded = False
        labelled = False

        def __len__(self):
            return 1

    for f in (axtrack_amd.fine_tune_head, axtrack_amd.fine_tune_detector):
        with pytest.raises(ValueError, match='test_loss=True needs a labelled test_timelapse'):
            f(Tl(), [([1], [1])], {}, test_loss=True)
        with pytest.raises(ValueError, match='test_loss=True needs a labelled test_timelapse'):
            f(Tl(), [([1], [1])], {}, test_loss=True, test_timelapse=Tl(), metrics_every=0)
