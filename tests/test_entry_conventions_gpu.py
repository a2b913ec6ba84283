"""The two conventions at the top of include/axtrack_hip.h -- "calls are asynchronous on `stream`" and "no hidden global
state: all device state lives in a handle or in caller-provided buffers" -- for every entry point that takes a stream,
through the production Python wrappers, on the cases of tests/entry_cases.py.

The values are judged elsewhere against high-precision references. Here the baseline is the wrapper's own result on the
default stream in the order everything else in the suite runs it, and every protocol demands the same BYTES inside the
region the header promises to write (every kernel is documented as deterministic: no tolerance):

  1. the decoy input gives a different result in every output (otherwise protocol 2 could not fail);
  2. side stream: the device inputs hold the decoy; on a non-blocking side stream a delay, a copy of the real input into
     those tensors and the call are enqueued in that order. Whatever the call puts on another stream runs during the delay
     and reads the decoy, or, from a buffer the wrapper has just allocated, whatever the allocator left there: the poison
     of protocol 3 (pattern 1, active here too) is itself enqueued on the side stream, so it makes sure that such a buffer
     is not read before the stream wrote it, and it is not what an early launch sees. Either way the result is wrong.
     The upstream stages of a stage-by-stage call (entry.prepare: track_links before link_paths, the field and its samples
     before target_paths, a trainer's forward before its input_grad) run on the real input BEFORE the delay, so that the
     named entry point is what is launched behind it; an upstream result with a valid decoy (entry.pre_decoy) is treated
     like an input;
  3. poisoned allocations: torch.empty / torch.empty_like / Tensor.new_empty fill what they hand out, NaN then 1e30 for
     floats, 1 then 2 for integers (small on purpose: scratch misread as an index stays in range). Inside `promised` both
     runs equal the baseline, outside it the output holds what the entry says (the pattern = untouched, or the wrapper's fill);
  4. no state between calls: real, other (another shape), real on one handle -- first and third results identical. A step
     changes its trainer by design: there each `real` gets a fresh trainer and the first one also runs `other`;
  5. controls, torch only: an op put on the default stream is reported by protocol 2, an unwritten last element by
     protocol 3.

The delay is a chain of 4096^2 f32 matmuls on the side stream, its length calibrated once per session with events to
about 50 ms and refused above 200 ms. A call that returns with its work still queued must leave the side stream busy
(`side.query()` is False right after it) and must have taken at most a tenth of the delay to enqueue. Two kinds of call
wait for the stream themselves and skip both assertions:
  SYNCING               the entry point, or its wrapper after the launch, reads a result back (entry.syncs says which). The
                        launches up to that wait run behind the delay, those after it do not (phase 2 of the two-phase
                        calls): protocol 2 covers the first part of these entry points;
  NOT_BEHIND_THE_DELAY  the wrapper waits BEFORE the entry point's first launch (entry.waits_first: a pageable upload, the
                        batch index checked on the host). By then the delay is over and the real input in place, so
                        protocol 2 CANNOT fail for these eight entry points whatever stream their launches use; it still
                        runs, and protocols 1, 3 and 4 cover them.
Run with -s to see the calibration and every enqueue time.

Measured on the MI355X (wall clock of the wrappers as they stood before this file, host otherwise idle):
  delay: 54 matmuls of 0.94 ms = 49.3 ms. Enqueue times of the calls that do not wait: 0.05 ms (max-pool, render) to 0.29 ms
  (axt_cnn_forward), and 1.67 ms for hotpath.ided_table, which allocates its pinned table: 10 x 1.67 = 16.7 ms <= 49.3 ms.
  The calls that wait return after 48 to 53 ms, the delay they waited for. No protocol found a difference in any entry.
tests/test_entry_conventions_cpu.py asserts that the two lists below are exactly the registry's."""
import contextlib
import math
import time

import numpy as np
import pytest
import torch

import entry_cases as ec

pytestmark = pytest.mark.gpu

DELAY_TARGET_MS, DELAY_MAX_MS, MARGIN = 50.0, 200.0, 10
PATTERNS = {1: (float('nan'), 1), 2: (1e30, 2)}            # pass -> (floats, every integer and byte type)
_UNPATCHED = (torch.empty, torch.empty_like, torch.Tensor.new_empty)


# ================================================================================================== poisoned allocations
def poison_(t, which):
    """Fill a freshly allocated tensor with pattern `which` by dtype (in place, on the current stream)."""
    fval, ival = PATTERNS[which]
    if t.numel():
        if t.dtype.is_floating_point:
            t.fill_(min(fval, torch.finfo(t.dtype).max))       # (NaN passes through min; 1e30 is clamped for a half)
        elif t.dtype == torch.bool:
            t.fill_(True)
        else:
            t.fill_(ival)
    return t


@contextlib.contextmanager
def poisoned_allocations(monkeypatch, which):
    """For the duration of the block, every tensor torch.empty, torch.empty_like and Tensor.new_empty hand out (device,
    pinned or plain host memory) is allocated as before and then filled with pattern `which`. Built on pytest's monkeypatch:
    the patch is gone when the block ends, however it ends."""
    empty, empty_like, new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty
    with monkeypatch.context() as m:
        m.setattr(torch, 'empty', lambda *a, **k: poison_(empty(*a, **k), which))
        m.setattr(torch, 'empty_like', lambda *a, **k: poison_(empty_like(*a, **k), which))
        m.setattr(torch.Tensor, 'new_empty', lambda self, *a, **k: poison_(new_empty(self, *a, **k), which))
        yield


def holds_pattern(values, which):
    """Whether every element of the array still holds pattern `which`."""
    fval, ival = PATTERNS[which]
    if values.dtype.kind == 'f':
        return bool(np.isnan(values).all()) if math.isnan(fval) else bool((values == values.dtype.type(fval)).all())
    return bool((values == ival).all())


# ================================================================================================== running a case
def upload(inp):
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in inp.dev.items()}


def resolve(outs):
    """The outputs of a call as host arrays; the caller has waited for the stream the call ran on."""
    res = {}
    for k, v in outs.items():
        if callable(v):
            v = v()
        if isinstance(v, torch.Tensor):
            v = v.cpu().numpy()
        res[k] = np.array(v)
    return res


_DETECTOR = {}


def new_handle(e, weights):
    """The handle the case runs on: the module's one detector, or a new grid / trainer from the case's own weights."""
    if e.handle is None:
        return None
    if e.handle == 'detector':
        if 'det' not in _DETECTOR:
            from axtrack_amd import hotpath
            _DETECTOR['det'] = hotpath.Detector(weights, max_batch=4)
        return _DETECTOR['det']
    return e.handle(e.inputs('real').host)


def prepared(e, h, d, host):
    """The upstream stages of the call on these inputs, waited for: what call() gets as `pre` (None without such stages)."""
    if e.prepare is None:
        return None
    pre = e.prepare(h, d, host)
    torch.cuda.synchronize()
    return pre


def call(e, h, d, host, pre):
    return e.call(h, d, host) if e.prepare is None else e.call(h, d, host, pre)


def run(e, h, kind, which=None, monkeypatch=None):
    """call(kind) on the default stream, waited for: {name: host array}. which: the poison pattern active during the call."""
    inp = e.inputs(kind)
    d = upload(inp)
    torch.cuda.synchronize()
    pre = prepared(e, h, d, inp.host)
    with (poisoned_allocations(monkeypatch, which) if which else contextlib.nullcontext()):
        outs = call(e, h, d, inp.host, pre)
    torch.cuda.synchronize()
    return resolve(outs)


_BASE = {}


def baseline(e, weights):
    if e.name not in _BASE:
        res = run(e, new_handle(e, weights), 'real')
        for a in res.values():
            a.setflags(write=False)
        _BASE[e.name] = res
    return _BASE[e.name]


def first_difference(g, b):
    if g.shape != b.shape or g.dtype != b.dtype:
        return f'{g.dtype}{list(g.shape)} instead of {b.dtype}{list(b.shape)}'
    gb, bb = (np.ascontiguousarray(a).reshape(-1).view(np.uint8).reshape(a.size, -1) for a in (g, b))
    bad = np.nonzero((gb != bb).any(axis=1))[0]
    i = np.unravel_index(int(bad[0]), g.shape) if g.ndim else ()
    return f'{len(bad)} of {g.size} elements differ, the first at {tuple(int(v) for v in i)}: {g[i]!r} instead of {b[i]!r}'


def check(e, got, base, what, which=None):
    """Byte equality with the baseline inside `promised`; outside it, what the entry says the output holds."""
    inp = e.inputs('real')
    assert set(got) == set(base), f'{e} ({what}): outputs {sorted(got)} instead of {sorted(base)}'
    masks = e.promised(inp, base) if e.promised else {}
    assert set(e.outside) <= set(masks), f'{e}: `outside` names {sorted(set(e.outside) - set(masks))}, which `promised` does not bound'
    for k in sorted(got, key=lambda k: k in masks):              # the fully promised outputs first: the masks build on them
        g, b = got[k], base[k]
        m = masks.get(k)
        if g.shape != b.shape or g.dtype != b.dtype or m is None:
            assert g.shape == b.shape and g.dtype == b.dtype and g.tobytes() == b.tobytes(), \
                f'{e} ({what}): output {k!r}: {first_difference(g, b)}'
            continue
        assert g[m].tobytes() == b[m].tobytes(), f'{e} ({what}): output {k!r} inside the promised region: ' \
                                                 f'{first_difference(np.where(m, g, 0), np.where(m, b, 0))}'
        rest, spec = g[~m], e.outside.get(k, ec.PATTERN)
        if spec is None or not rest.size:
            continue
        if spec == ec.PATTERN:
            assert which is None or holds_pattern(rest, which), \
                f'{e} ({what}): output {k!r} was written outside the promised region ({e.quotes})'
        else:
            assert (rest == spec).all(), f'{e} ({what}): output {k!r} outside the promised region is not the wrapper\'s {spec}'


# ================================================================================================== the delay
class Delay:
    """A chain of matmuls on the current stream: plain torch work whose length is known, no spinning, no graph."""

    def __init__(self):
        n = 4096
        self.a = torch.eye(n, device='cuda')
        self.x = [torch.rand(n, n, device='cuda'), torch.empty(n, n, device='cuda')]
        self.reps = 8
        self.enqueue()                                           # (the first matmul loads its kernel)
        per_rep = self.measure() / self.reps
        self.reps = max(1, math.ceil(DELAY_TARGET_MS / per_rep))
        self.ms = self.measure()
        print(f'\ndelay: {self.reps} matmuls of 4096^2 f32 = {self.ms:.1f} ms ({per_rep:.3f} ms each)')
        assert self.ms <= DELAY_MAX_MS, f'the delay came out at {self.ms:.0f} ms: refused above {DELAY_MAX_MS:.0f} ms'

    def enqueue(self):
        for i in range(self.reps):
            torch.mm(self.x[i % 2], self.a, out=self.x[1 - i % 2])

    def measure(self):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        self.enqueue()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)


@pytest.fixture(scope='session')
def delay():
    return Delay()


def side_stream_run(e, h, delay, monkeypatch):
    """Protocol 2: ({name: host array}, seconds the call took to enqueue, whether the side stream was still busy after it)."""
    real, decoy = e.inputs('real'), e.inputs('decoy')
    staging, d = upload(real), upload(decoy)
    pre = prepared(e, h, staging, real.host)              # upstream stages: on the real input, before the delay
    pre_staging = {}
    if e.pre_decoy is not None:                           # upstream results that start as a decoy, like the inputs
        pre_staging = {k: pre[k] for k in e.pre_decoy(pre)}
        pre = dict(pre, **{k: v.clone() for k, v in e.pre_decoy(pre).items()})
        assert all(pre[k].shape == v.shape and pre[k].dtype == v.dtype and not torch.equal(pre[k], v) for k, v in pre_staging.items())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        delay.enqueue()
        for k in d:
            d[k].copy_(staging[k], non_blocking=True)
        for k, v in pre_staging.items():
            pre[k].copy_(v, non_blocking=True)
        t0 = time.perf_counter()
        with poisoned_allocations(monkeypatch, 1):
            outs = call(e, h, d, real.host, pre)
        seconds = time.perf_counter() - t0
        busy = not side.query()
        side.synchronize()
        res = resolve(outs)
    torch.cuda.synchronize()
    return res, seconds, busy


# ================================================================================================== the tests
ENTRIES = pytest.mark.parametrize('e', ec.ENTRIES, ids=repr)
# the entry points that wait for the stream after their own first launches, and so skip the `query` assertion
SYNCING = ('axt_preprocess_stats_u16', 'axt_build_arcs', 'axt_hungarian_pairs', 'axt_track_links', 'axt_link_paths',
           'axt_link_cells', 'axt_target_field', 'axt_target_paths', 'axt_segment_flood')
# the entry points whose wrapper waits before their first launch: the side-stream protocol cannot fail for them
NOT_BEHIND_THE_DELAY = ('axt_preprocess_u16_framewise', 'axt_detection_confusion', 'axt_yolo_targets', 'axt_head_trainer_forward',
                        'axt_head_trainer_loss', 'axt_head_trainer_step', 'axt_conv_trainer_forward', 'axt_conv_trainer_step')


@ENTRIES
def test_decoy_gives_another_result_in_every_output(e, weights):
    base = baseline(e, weights)
    got = run(e, new_handle(e, weights), 'decoy')
    assert set(got) == set(base)
    same = [k for k in got if got[k].shape == base[k].shape and got[k].tobytes() == base[k].tobytes()]
    assert not same, f'{e}: the decoy gives the real input\'s {same}: a stale read of the input would go unnoticed there'


@ENTRIES
def test_side_stream(e, weights, delay, monkeypatch):
    base = baseline(e, weights)
    got, seconds, busy = side_stream_run(e, new_handle(e, weights), delay, monkeypatch)
    print(f'\n{e}: enqueued in {seconds * 1e3:.3f} ms, the delay is {delay.ms:.1f} ms, side stream {"busy" if busy else "idle"} after the call'
          + (f' (waits: {e.syncs or e.waits_first})' if e.syncs or e.waits_first else ''))
    if not (e.syncs or e.waits_first):
        assert busy, f'{e}: the side stream was idle right after the call: it waited for the stream, or the delay is too short'
        assert MARGIN * seconds * 1e3 <= delay.ms, f'{e}: {seconds * 1e3:.2f} ms to enqueue leaves the {delay.ms:.0f} ms delay no {MARGIN}x margin'
    check(e, got, base, 'side stream', which=1)


@ENTRIES
@pytest.mark.parametrize('which', sorted(PATTERNS))
def test_poisoned_allocations(e, which, weights, monkeypatch):
    base = baseline(e, weights)
    got = run(e, new_handle(e, weights), 'real', which, monkeypatch)
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == _UNPATCHED, 'the patch outlived the call'
    check(e, got, base, f'allocations poisoned with pattern {which}', which=which)


@ENTRIES
def test_no_state_between_calls(e, weights):
    base = baseline(e, weights)
    h = new_handle(e, weights)
    first = run(e, h, 'real')
    run(e, h, 'other')
    third = run(e, new_handle(e, weights) if e.fresh_handle else h, 'real')
    check(e, first, base, 'first call')
    check(e, third, first, 'real again after another shape')


# ------------------------------------------------------------------------------------------------ controls
def _control_inputs(kind):
    n = 70 if kind == 'other' else 50
    return ec.Inputs({'x': np.random.default_rng(ec.SEED[kind]).random(n, dtype=np.float32)})


def _call_on_default_stream(_, d, p):
    with torch.cuda.stream(torch.cuda.default_stream()):
        return {'y': d['x'] * 2}


def _call_leaving_the_tail(_, d, p):
    y = torch.empty(d['x'].numel(), dtype=torch.float32, device='cuda')
    y[:-1] = d['x'][:-1] * 2
    return {'y': y}


def test_control_side_stream_reports_an_op_on_the_default_stream(weights, delay, monkeypatch):
    good = ec.Entry('control_good', None, _control_inputs, lambda _, d, p: {'y': d['x'] * 2})
    got, _, busy = side_stream_run(good, None, delay, monkeypatch)
    assert busy
    check(good, got, baseline(good, weights), 'side stream', which=1)
    bad = ec.Entry('control_default_stream', None, _control_inputs, _call_on_default_stream)
    got, _, _ = side_stream_run(bad, None, delay, monkeypatch)
    with pytest.raises(AssertionError, match='control_default_stream'):
        check(bad, got, baseline(bad, weights), 'side stream', which=1)
    assert np.array_equal(got['y'], bad.inputs('decoy').dev['x'] * 2), 'the op on the default stream should have read the decoy'


def test_control_poison_reports_an_unwritten_element(weights, monkeypatch):
    bad = ec.Entry('control_tail', None, _control_inputs, _call_leaving_the_tail)
    base = baseline(bad, weights)
    reported = 0
    for which in sorted(PATTERNS):
        got = run(bad, None, 'real', which, monkeypatch)
        assert holds_pattern(got['y'][-1:], which) and np.array_equal(got['y'][:-1], base['y'][:-1])
        try:
            check(bad, got, base, f'pattern {which}', which=which)
        except AssertionError:
            reported += 1
    # one pattern may happen to be what the baseline's allocation held; two different ones cannot both be
    assert reported >= 1


# ------------------------------------------------------------------------------------------------ host copies
def test_to_host_waits_for_the_callers_stream(delay):
    """hotpath.to_host stages through module-global pinned buffers and waits for the current stream of the tensors' device:
    behind a delay on a side stream it must still return what the stream wrote last, for two dtypes at once, and a second
    call at another size must not disturb the first one's copy once that has been taken."""
    from axtrack_amd import hotpath
    rng = np.random.default_rng(5)
    real = [rng.random(3000, dtype=np.float32), rng.integers(0, 1 << 30, 500).astype(np.int64)]
    decoy = [np.zeros(3000, np.float32), np.ones(500, np.int64)]
    staging, d = [torch.from_numpy(a).cuda() for a in real], [torch.from_numpy(a).cuda() for a in decoy]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        delay.enqueue()
        for t, s in zip(d, staging):
            t.copy_(s, non_blocking=True)
        got = [a.copy() for a in hotpath.to_host(*d)]
        again = [a.copy() for a in hotpath.to_host(d[0][:7], d[1][:9])]
    torch.cuda.synchronize()
    assert all(np.array_equal(g, r) for g, r in zip(got, real))
    assert np.array_equal(again[0], real[0][:7]) and np.array_equal(again[1], real[1][:9])
