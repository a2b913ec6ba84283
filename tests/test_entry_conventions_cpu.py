"""What the convention tests of tests/test_entry_conventions_gpu.py rest on, checked without a GPU: the registry of
tests/entry_cases.py covers every entry point of the header that takes a stream, its inputs are what the protocols need
(real and decoy alike in shape and dtype, `other` at another shape, every one of them a valid input), and the allocation
poisoning fills by dtype, leaves torch.zeros alone and is gone after the block."""
import os
import re

import numpy as np
import pytest
import torch

import entry_cases as ec
import test_entry_conventions_gpu as proto
from axtrack_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_entry_points():
    """Every function declared in include/axtrack_hip.h (and the stage header it includes) with a `stream` parameter."""
    src = ''
    for name in ('axtrack_hip.h', 'axtrack_hip_stage.h'):
        with open(os.path.join(ROOT, 'include', name)) as f:
            src += f.read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    found = [m.group(1) for m in re.finditer(r'\b(axt_\w+)\s*\(([^;{]*?)\)\s*;', src)
             if re.search(r'\bvoid\s*\*\s*stream\b', m.group(2))]
    assert len(found) == len(set(found))
    return found


def test_the_parser_finds_the_entry_points():
    names = stream_entry_points()
    assert len(names) >= 40
    for known in ('axt_cnn_forward', 'axt_build_arcs', 'axt_hungarian_pairs', 'axt_maxpool2_backward', 'axt_augment_frames'):
        assert known in names
    for host_only in ('axt_mcf_solve', 'axt_grid_create', 'axt_detector_create', 'axt_head_trainer_read_weights'):
        assert host_only not in names


def test_every_stream_entry_point_has_a_case():
    names = stream_entry_points()
    cases = ec.by_abi()
    assert len(ec.EXCLUDED) <= 3 and all(isinstance(r, str) and r for r in ec.EXCLUDED.values())
    assert not set(ec.EXCLUDED) & set(cases), 'an excluded entry point has a case'
    missing = [n for n in names if n not in cases and n not in ec.EXCLUDED]
    assert not missing, f'no case in tests/entry_cases.py for {missing}'
    unknown = [n for n in list(cases) + list(ec.EXCLUDED) if n not in names]
    assert not unknown, f'cases for {unknown}, which the header does not declare with a stream'
    unbound = [n for n in names if n not in _lib.SIGNATURES]
    assert not unbound, f'{unbound} are not in _lib.SIGNATURES'
    assert len({e.name for e in ec.ENTRIES}) == len(ec.ENTRIES)


def test_the_waiting_entry_points_are_the_listed_ones():
    """The two lists of the GPU module's docstring are the registry's: who waits after its own launches (no `query`
    assertion), and whose wrapper waits before the launch (the side-stream protocol cannot fail there)."""
    assert sorted({e.abi for e in ec.ENTRIES if e.syncs}) == sorted(proto.SYNCING)
    assert sorted({e.abi for e in ec.ENTRIES if e.waits_first}) == sorted(proto.NOT_BEHIND_THE_DELAY)
    assert not set(proto.SYNCING) & set(proto.NOT_BEHIND_THE_DELAY)
    # every case of an entry point agrees on which kind it is
    for abi, cases in ec.by_abi().items():
        assert len({bool(e.waits_first) for e in cases}) == 1, abi


def test_the_conv_trainer_runs_in_both_batchnorm_modes():
    for abi in ('axt_conv_trainer_forward', 'axt_conv_trainer_step', 'axt_conv_trainer_input_grad'):
        assert sorted(e.name.endswith('[batch_stats]') for e in ec.by_abi()[abi]) == [False, True]


@pytest.mark.parametrize('e', ec.ENTRIES, ids=repr)
def test_inputs_are_valid_and_shaped_for_the_protocols(e):
    ec.check_entry(e)
    for why in (e.syncs, e.waits_first):
        assert why is None or (isinstance(why, str) and why)
    assert not (e.syncs and e.waits_first), f'{e}: the wait comes before the first launch or after it, not both'
    assert e.pre_decoy is None or e.prepare is not None
    assert not e.outside or e.promised is not None, f'{e} says what lies outside a promised region it does not declare'
    if e.promised is not None:
        assert e.quotes, f'{e} promises less than the whole output without quoting the sentence that says so'


def test_check_entry_refuses_an_invalid_decoy():
    def make(kind):
        x = np.arange(4 if kind == 'other' else 3, dtype=np.int32) + (kind == 'decoy') * 8
        return ec.Inputs({'x': x}, limits={'x': (0, 10)})
    with pytest.raises(AssertionError, match='leaves'):
        ec.check_entry(ec.Entry('bad', None, make, None))

    def same(kind):
        return ec.Inputs({'x': np.arange(4 if kind == 'other' else 3, dtype=np.int32)})
    with pytest.raises(AssertionError, match='equals the real'):
        ec.check_entry(ec.Entry('same', None, same, None))


# ------------------------------------------------------------------------------------------------ the poisoning
DTYPES = (torch.float32, torch.float64, torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8)


@pytest.mark.parametrize('which', sorted(proto.PATTERNS))
def test_poisoning_fills_by_dtype_and_goes_away(which, monkeypatch):
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    fval, ival = proto.PATTERNS[which]
    pinned = torch.cuda.is_available()                      # pinned host memory needs the runtime; plain host memory does not
    with proto.poisoned_allocations(monkeypatch, which):
        assert torch.empty is not before[0]
        for dt in DTYPES:
            made = [torch.empty((3, 5), dtype=dt), torch.empty(7, dtype=dt), torch.empty_like(torch.zeros(4, dtype=dt)),
                    torch.zeros(2, dtype=dt).new_empty((2, 2))]
            if pinned:
                made.append(torch.empty(6, dtype=dt, pin_memory=True))
                assert made[-1].is_pinned()
            for t in made:
                assert t.dtype == dt
                a = t.numpy()
                assert proto.holds_pattern(a, which)
                if dt.is_floating_point:
                    assert np.isnan(a).all() if which == 1 else (a == a.dtype.type(fval)).all()
                else:
                    assert (a == ival).all()
        assert torch.empty(0).numel() == 0
        assert not torch.zeros(9).any() and not torch.zeros(9, dtype=torch.int32).any()       # torch.zeros is not affected
        assert (torch.full((3,), -1) == -1).all()
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    with pytest.raises(RuntimeError, match='boom'):
        with proto.poisoned_allocations(monkeypatch, which):
            raise RuntimeError('boom')
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before


def test_the_two_patterns_differ_and_stay_in_range():
    (f1, i1), (f2, i2) = (proto.PATTERNS[k] for k in (1, 2))
    assert np.isnan(f1) and np.isfinite(np.float32(f2)) and f2 != 0
    assert i1 != i2 and 0 < i1 < 4 and 0 < i2 < 4           # scratch misread as a count or an index stays in range
    assert not proto.holds_pattern(np.array([1e30], np.float32), 1) and not proto.holds_pattern(np.array([2]), 1)
