"""Every route of render.hip, through axt_render_frames itself, on the cases of tests/render_cases.py: the runs of frames
(chunk 1, chunk > 1 with a short last run, more than 512 tiles), the trail cursor with gaps in ts, the strided loops over
more than 256 trail cells and primitives, the 16-byte and the byte store path at every row alignment, the rounding and
background edges, and the clipping of every primitive. tests/test_render_routes_cpu.py proves on the CPU that each case
reaches the route its facts claim; here the kernel renders them.

The lists are binned with the production render._bin / render._csr. The output lies inside a larger buffer filled with a
sentinel, at the case's byte offset behind a 16-byte-aligned address. Everything is compared byte for byte with the
per-pixel reference of the cases file: no tolerance, no pixel left out; a failure names the first differing (frame, y, x),
its tile and its run, and the case's route. The bytes around the output must stay untouched.

Differences observed on the MI355X: none. The NaN, negative and > 1 pixels, the glyph codes -1 and 95 and the mask bytes 2
and 255 come out as DESIGN.md 6.8b and the reference painter have them (NaN -> 0, no glyph, mask set)."""
import numpy as np
import pytest
import torch

import render_cases as rc
from axtrack_amd import _lib, render
from axtrack_amd.hotpath import _stream
from render_cases import RT

pytestmark = pytest.mark.gpu

CASES = rc.all_cases()
AXT_OK, AXT_EINVAL = 0, -22
SENTINEL, PAD = 0xA5, 256
_RUNS, _REFS = {}, {}


def dev(a):
    a = np.ascontiguousarray(a)
    if a.size == 0:                                                   # (an empty tensor has no address)
        a = np.zeros((1,) + a.shape[1:], a.dtype)
    return torch.from_numpy(a).cuda()


def reference_of(case):
    if case.name not in _REFS:
        _REFS[case.name] = rc.reference(case)
        _REFS[case.name].setflags(write=False)
    return _REFS[case.name]


def call(case, lists, ts=None, **change):
    """axt_render_frames on the case: (return code, u8 [n_out, Ho, Wo, 3], the sentinel bytes before, those after)."""
    ts = case.ts if ts is None else ts
    _, H, W = case.frames.shape
    ymin, xmin, Ho, Wo = case.slice
    ts_dev = dev(ts.astype(np.int32))
    arg = dict(d_ts=ts_dev.data_ptr(), n_out=len(ts), H=H, W=W, ymin=ymin, xmin=xmin, Ho=Ho, Wo=Wo, grid=case.grid)
    keep = [dev(case.frames), None if case.mask is None else dev(case.mask), dev(case.trail_col), dev(rc.TABLES)] + [dev(a) for a in lists]
    frames, mask, trail_col, tables, trail_ptr, trail, prim_ptr, prims = keep
    n = len(ts) * Ho * Wo * 3
    buf = torch.full((PAD + 16 + case.out_offset + n + PAD,), SENTINEL, dtype=torch.uint8, device='cuda')
    start = (-buf.data_ptr()) % 16 + PAD + case.out_offset
    assert (buf.data_ptr() + start - case.out_offset) % 16 == 0
    arg.update(change)
    code = _lib.load().axt_render_frames(
        frames.data_ptr(), _lib.dptr(mask), case.mask_stride, arg['d_ts'], arg['n_out'], arg['H'], arg['W'], arg['ymin'], arg['xmin'], arg['Ho'],
        arg['Wo'], arg['grid'], int(case.bg), trail_ptr.data_ptr(), trail.data_ptr(), trail_col.data_ptr(), prim_ptr.data_ptr(),
        prims.data_ptr(), tables.data_ptr(), buf.data_ptr() + start, _stream())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    del keep, ts_dev
    return code, host[start:start + n].reshape(len(ts), Ho, Wo, 3), host[:start], host[start + n:]


def rendered(case):
    """The kernel's bytes for the case with the production binning, once per session (the sentinel is checked here too)."""
    if case.name not in _RUNS:
        code, out, before, after = call(case, rc.binned(case, render._bin, render._csr))
        assert code == AXT_OK, f'{case.route}: axt_render_frames returned {code}'
        check_sentinel(before, after, case)
        out.setflags(write=False)
        _RUNS[case.name] = out
    return _RUNS[case.name]


def check_sentinel(before, after, case):
    for name, part in (('before', before), ('after', after)):
        bad = np.nonzero(part != SENTINEL)[0]
        if len(bad):
            at = int(bad[0]) - len(part) if name == 'before' else int(bad[0])
            raise AssertionError(f'{case.route}: {len(bad)} bytes {name} the output were written, the first {at} bytes from the output\'s '
                                 f'{"first" if name == "before" else "last"} byte')


def check_bytes(got, want, case, what, first_frame=0):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    if np.array_equal(got, want):
        return
    d = np.argwhere((got != want).any(-1))
    i, y, x = (int(v) for v in d[0])
    ntx, _, _, chunk, _ = rc.launch(case, len(got))
    raise AssertionError(f'{case.route}: {what}: {len(d)} pixels differ, first at (frame {first_frame + i}, y {y}, x {x}), tile '
                         f'{(y // RT) * ntx + x // RT} (row {y // RT}, column {x // RT}), run {i // chunk} of chunk {chunk}: kernel '
                         f'{got[i, y, x].tolist()}, reference {want[i, y, x].tolist()}')


def test_tile_size():
    assert _lib.load().axt_render_tile_size() == RT


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_kernel_equals_the_per_pixel_reference(case):
    check_bytes(rendered(case), reference_of(case), case, 'kernel against the reference')


def relisted(case):
    """Every trail cell in every tile (by frame, equal frames in their order), every primitive in every tile of its frame."""
    ntiles, n_out = rc.launch(case)[2], len(case.ts)
    cells = case.trail[np.argsort(case.trail[:, 0], kind='stable')].astype(np.int32)
    trail = np.tile(cells, (ntiles, 1))
    trail_ptr = (np.arange(ntiles + 1) * len(cells)).astype(np.int32)
    blocks, counts = [], []
    for i in range(n_out):
        mine = np.zeros((int((case.prims[:, 0] == i).sum()), 8), np.int32)
        mine[:, :6] = case.prims[case.prims[:, 0] == i, 1:7]
        blocks.append(np.tile(mine, (ntiles, 1)))
        counts += [len(mine)] * ntiles
    prim_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return trail_ptr, trail, prim_ptr, np.concatenate(blocks)


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_clipping_belongs_to_the_kernel_not_to_the_binning(case):
    code, out, before, after = call(case, relisted(case))
    assert code == AXT_OK
    check_sentinel(before, after, case)
    check_bytes(out, rendered(case), case, 'everything listed in every tile against the binned render')


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_a_second_call_gives_equal_bytes(case):
    first = rendered(case)
    code, out, before, after = call(case, rc.binned(case, render._bin, render._csr))
    assert code == AXT_OK
    check_sentinel(before, after, case)
    check_bytes(out, first, case, 'second call against the first')


@pytest.mark.parametrize('case', [c for c in CASES if len(c.ts) > 1], ids=repr)
def test_render_of_a_tail_of_ts_equals_the_tail_of_the_render(case):
    """ts[1:] starts inside the first run wherever chunk > 1: its first frame needs the whole trail history."""
    ts, prims = rc.tail_inputs(case, 1)
    code, out, before, after = call(case, rc.binned(case, render._bin, render._csr, ts, prims), ts)
    assert code == AXT_OK
    check_sentinel(before, after, case)
    check_bytes(out, rendered(case)[1:], case, 'render of ts[1:] against frames 1.. of the render of ts', first_frame=1)


@pytest.mark.parametrize('change,code', [(dict(n_out=0), AXT_OK), (dict(ymin=1 << 20), AXT_EINVAL), (dict(Wo=1 << 20), AXT_EINVAL),
                                         (dict(xmin=-1), AXT_EINVAL), (dict(grid=-1), AXT_EINVAL), (dict(d_ts=None), AXT_EINVAL)],
                         ids=['n_out_0', 'slice_below_the_frame', 'slice_wider_than_the_frame', 'negative_xmin', 'negative_grid', 'null_ts'])
def test_return_codes(change, code):
    case = next(c for c in CASES if c.name == 'wo17')
    got, out, before, after = call(case, rc.binned(case, render._bin, render._csr), **change)
    assert got == code
    assert (out == SENTINEL).all() and (before == SENTINEL).all() and (after == SENTINEL).all(), 'a refused or empty call wrote to the buffer'
