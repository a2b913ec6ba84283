"""Deflate TIFF strips written on the GPU (csrc/tiff_deflate.hip, csrc/axt_tiff_deflate.h, tiff.write_tiff,
interface.process_timelapse; DESIGN.md 6.8h "TIFF output"). Deflating is integer work and the parse is a function of the
strip's bytes alone: every device stream must be byte-identical to the one the host program (tests/tiff_deflate_host.cpp,
the same core with one worker) writes, and inflate through zlib to the strip. Files are read back by read_tiff on both
inflate routes, by zlib strip by strip over tiff_info's tables, and by Pillow / libtiff where that is available."""
import os
import time
import zlib

import numpy as np
import pytest
import torch

import test_entry_conventions_gpu as proto
import test_tiff_gpu as tg
import test_tiff_inflate_gpu as tig
import tiff_deflate_cases as dc
import tiff_inflate_cases as ic
import axtrack_amd
from axtrack_amd import _lib, hotpath, params, synth, tiff
from axtrack_amd.tiff import TIFF_SEGMENT_DTYPE, read_tiff, write_tiff

pytestmark = pytest.mark.gpu
DEV = tg.DEV
CANARY, FILL = 4096, 0xA5
OK, OVERRUN, BAD_SEGMENT = 0, 3, 4


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """{case name: the host program's stream}, and the program for further strips."""
    tmp = tmp_path_factory.mktemp('deflate_host')
    cases = dc.deflate_cases()
    exe = dc.build_host_program(tmp, sanitize=False)
    res, streams = dc.run_host_program(exe, cases, tmp)
    assert res.returncode == 0, res.stdout[-2000:]
    return {c.name: s for c, (_, s, _) in zip(cases, streams)}, exe, tmp


class Launch:
    """Strips for one launch (one W, one predictor): their samples `gap` elements apart between two canaries, their slots
    -- of the all-stored bound, or of `caps` -- `gap` bytes apart between two canaries, everything pre-filled."""

    def __init__(self, strips, W, caps=None, gap=64):
        self.strips, self.W = strips, W
        n = len(strips)
        self.rec = np.zeros(n, TIFF_SEGMENT_DTYPE)
        self.caps = [dc.bound(a.size * 2) for a in strips] if caps is None else list(caps)
        pos, at = CANARY, CANARY + 1                                      # (the first slot at an odd address)
        for k, a in enumerate(strips):
            assert a.shape[1] == W
            self.rec[k] = (at, self.caps[k], pos, a.shape[0], 0)
            pos += a.size + gap
            at += self.caps[k] + gap
        self.in_len, self.slots_len = pos - gap + CANARY, at - gap + CANARY
        self.samples = np.full(self.in_len, 0x5AA5, np.uint16)
        for k, a in enumerate(strips):
            p = int(self.rec['dst_offset'][k])
            self.samples[p:p + a.size] = a.ravel()

    def run(self, predictor):
        d_in = torch.from_numpy(self.samples.view(np.int16).copy()).to(DEV)
        slots = torch.full((self.slots_len,), FILL, dtype=torch.uint8, device=DEV)
        n = len(self.strips)
        nbytes = torch.full((n,), -7, dtype=torch.int64, device=DEV)
        status = torch.full((n,), 77, dtype=torch.int32, device=DEV)
        d_segs = torch.from_numpy(self.rec.view(np.uint8).copy()).to(DEV)
        lib = _lib.load()
        rc = lib.axt_tiff_deflate_u16(d_in.data_ptr(), d_in.numel(), d_segs.data_ptr(), n, self.W, predictor, slots.data_ptr(),
                                      slots.numel(), nbytes.data_ptr(), status.data_ptr(), None)
        assert rc == 0, lib.axt_last_error()
        packed = torch.full((self.slots_len,), FILL, dtype=torch.uint8, device=DEV)
        offsets = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
        rc = lib.axt_tiff_compact_streams(slots.data_ptr(), d_segs.data_ptr(), nbytes.data_ptr(), n, packed.data_ptr(), packed.numel(),
                                          offsets.data_ptr(), None)
        assert rc == 0, lib.axt_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(d_in.cpu().numpy().view(np.uint16), self.samples), 'the input was written'
        return slots.cpu().numpy(), nbytes.cpu().numpy(), status.cpu().numpy(), packed.cpu().numpy(), offsets.cpu().numpy()

    def check(self, result, predictor, want_status=None, want_streams=None):
        """Statuses and lengths; every good stream inflates through zlib to its strip and equals want_streams[k]; nothing
        outside the slots of the accepted descriptors is written; the compaction is the exclusive scan and the gather."""
        slots, nbytes, status, packed, offsets = result
        n = len(self.strips)
        want_status = [OK] * n if want_status is None else want_status
        assert status.tolist() == want_status
        touched = np.zeros(self.slots_len, bool)
        streams = []
        for k, a in enumerate(self.strips):
            o, cap = int(self.rec['src_offset'][k]), int(self.rec['src_bytes'][k])
            if want_status[k] != BAD_SEGMENT:
                touched[o:o + cap] = True
            if want_status[k] != OK:
                assert nbytes[k] == 0
                streams.append(b'')
                continue
            raw = dc.stored_bytes(a, predictor)
            assert 8 <= nbytes[k] <= min(cap, dc.bound(len(raw))), k
            s = slots[o:o + int(nbytes[k])].tobytes()
            assert zlib.decompress(s) == raw, k
            if want_streams is not None:
                assert s == want_streams[k], f'strip {k}: the device stream is not the host program\'s'
            streams.append(s)
        assert (slots[~touched] == FILL).all(), 'a write outside the slots'
        assert not touched[:CANARY].any() and not touched[-CANARY:].any()
        lengths = np.array([len(s) for s in streams], np.int64)
        assert offsets.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
        total = int(offsets[-1])
        assert packed[:total].tobytes() == b''.join(streams) and (packed[total:] == FILL).all()
        return streams


def test_the_whole_battery(host):
    """Every case of the battery, one launch per (W, predictor), the strips in the battery's order. In the larger groups
    two descriptors are out of range among good ones (a negative field; samples one element past in_len): status 4, nothing
    of their slots written, left out of the compaction. Every stream is byte-identical to the host program's."""
    by_name, _, _ = host
    groups = {}
    for c in dc.deflate_cases():
        groups.setdefault((c.a.shape[1], c.predictor), []).append(c)
    assert len(groups[(512, 1)]) >= 8 and len(groups[(80, 1)]) >= 4
    for (W, predictor), cs in groups.items():
        la = Launch([c.a for c in cs], W)
        want = [OK] * len(cs)
        if len(cs) >= 4:
            la.rec['src_offset'][1] = -1
            la.rec['dst_offset'][len(cs) - 2] = la.in_len - cs[-2].a.size + 1
            want[1] = want[len(cs) - 2] = BAD_SEGMENT
        la.check(la.run(predictor), predictor, want, [by_name[c.name] for c in cs])


def test_size_conditions_on_the_device_streams():
    """Conditions, not tolerances, each one zlib level 1 itself satisfies (seed-0 frames of 32 x 512): every stream within
    the all-stored bound (Launch.check); sparse, blobs and zeros smaller than zlib's Z_HUFFMAN_ONLY stream of the same
    bytes -- the matcher finds matches --; camera smaller than zlib's level-1 Z_FIXED stream -- the dynamic codes work --;
    noise comes out stored, at exactly the bound."""
    kinds = ('sparse', 'blobs', 'zeros', 'camera', 'noise')
    frames = [dc.FRAME_KINDS[k]((32, 512), 0) for k in kinds]
    for predictor in (1, 2):
        la = Launch(frames, 512)
        streams = dict(zip(kinds, la.check(la.run(predictor), predictor)))
        raw = {k: dc.stored_bytes(a, predictor) for k, a in zip(kinds, frames)}
        print(predictor, {k: len(s) for k, s in streams.items()})
        for k in ('sparse', 'blobs', 'zeros'):
            assert len(streams[k]) < len(ic.deflate(raw[k], strategy=zlib.Z_HUFFMAN_ONLY)), k
        assert len(streams['camera']) < len(ic.deflate(raw['camera'], 1, zlib.Z_FIXED))
        assert ic.first_block_type(streams['noise']) == 0 and len(streams['noise']) == dc.bound(32768)


def test_slots_one_byte_too_small(host):
    """Every slot one byte shorter than the stream it is to receive: status 3, length 0, nothing outside the slot written
    (the gaps and canaries hold); among them two slots that fit, whose streams are whole."""
    by_name, _, _ = host
    cs = [c for c in dc.deflate_cases() if c.a.shape[1] == 80 and c.predictor == 1]
    caps = [len(by_name[c.name]) - 1 for c in cs]
    want = [OVERRUN] * len(cs)
    caps[0] += 1
    caps[-1] += 1
    want[0] = want[-1] = OK
    la = Launch([c.a for c in cs], 80, caps=caps)
    la.check(la.run(1), 1, want, [by_name[c.name] for c in cs])


def test_more_strips_than_blocks(host):
    """2049 strips of one row: the grid of 2048 blocks strides, block 0 deflates strip 0 and then strip 2048 with the same
    LDS -- a noise row (stored) and then a flat row (matches), the other order on block 1's pair; a hash-table entry or a
    staged bit left over from the first strip would show in the second. Byte-identical to the host program; the
    compaction's scan carries over eight tiles of 256."""
    _, exe, tmp = host
    W = 80
    rows = [np.ascontiguousarray(r) for r in dc.sparse_frame((2049, 1, W), 301, density=0.2)]
    noise_row, flat_row = np.random.default_rng(302).integers(0, 65536, (1, W)).astype(np.uint16), np.full((1, W), 0x4141, np.uint16)
    rows[0], rows[2048], rows[1] = noise_row, flat_row, flat_row
    for predictor in (1, 2):
        cases = [dc.DeflateCase(f's{k}', a, predictor) for k, a in enumerate(rows)]
        res, streams = dc.run_host_program(exe, cases, tmp, f'rows{predictor}')
        assert res.returncode == 0
        la = Launch(rows, W, gap=8)
        la.check(la.run(predictor), predictor, None, [s for _, s, _ in streams])


def test_deflate_on_a_side_stream_with_poisoned_allocations(monkeypatch):
    """The side-stream protocol of tests/test_entry_conventions_gpu.py: the sample buffer holds a decoy; on a non-blocking
    side stream a delay, the copy of the real samples and the launches (deflate, compaction) are enqueued in that order. A
    launch on any other stream runs during the delay and deflates the decoy. Allocations are poisoned during the call."""
    delay = proto.Delay()
    real, decoy = dc.blobs_frame((40, 80), 311), dc.blobs_frame((40, 80), 312)
    segs = np.zeros(5, TIFF_SEGMENT_DTYPE)
    segs['rows'], segs['dst_offset'] = 8, np.arange(5) * 8 * 80
    segs['src_bytes'] = dc.bound(8 * 80 * 2)
    segs['src_offset'] = np.arange(5) * dc.bound(8 * 80 * 2)
    total = 5 * dc.bound(8 * 80 * 2)

    def run(samples, slots, table, status, packed):
        d_segs = hotpath.tiff_deflate_launch(samples, segs, 80, 2, slots, table[:5], status)
        hotpath.tiff_compact_launch(slots, d_segs, table[:5], 5, packed, table[5:11])
        return d_segs

    def buffers():
        return (torch.full((total,), FILL, dtype=torch.uint8, device=DEV), torch.full((11,), -7, dtype=torch.int64, device=DEV),
                torch.full((5,), 77, dtype=torch.int32, device=DEV), torch.full((total,), FILL, dtype=torch.uint8, device=DEV))

    to_dev = lambda a: torch.from_numpy(a.view(np.int16).copy()).to(DEV)
    base = buffers()
    run(to_dev(real), *base)
    torch.cuda.synchronize()
    off = base[1][5:11].cpu().numpy()
    assert base[2].tolist() == [0] * 5 and off[0] == 0
    for k in range(5):
        assert zlib.decompress(base[3][int(off[k]):int(off[k + 1])].cpu().numpy().tobytes()) == dc.stored_bytes(real[8 * k:8 * k + 8], 2)
    samples, staging = to_dev(decoy), to_dev(real)
    out = buffers()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        delay.enqueue()
        samples.copy_(staging, non_blocking=True)
        t0 = time.perf_counter()
        with proto.poisoned_allocations(monkeypatch, 1):
            keep = run(samples, *out)
        seconds = time.perf_counter() - t0
        busy = not side.query()
        side.synchronize()
    print(f'\n{seconds * 1e3:.2f} ms to enqueue the launches behind a delay of {delay.ms:.1f} ms')
    assert busy, 'the launch waited for the stream'
    assert seconds * 1e3 <= delay.ms / proto.MARGIN
    assert torch.equal(out[1], base[1]) and torch.equal(out[2], base[2]) and torch.equal(out[3], base[3])
    del keep


# ------------------------------------------------------------------------------------------------ files
def pillow_pages(path):
    """The file's pages through Pillow / libtiff, or None where that is not available."""
    try:
        from PIL import Image, features
    except ImportError:
        return None
    if not features.check('libtiff'):
        return None
    pages = []
    with Image.open(path) as im:
        for k in range(getattr(im, 'n_frames', 1)):
            im.seek(k)
            pages.append(np.array(im).astype(np.uint16))
    return np.stack(pages)


STACKS = {'5x48x80': lambda: dc.blobs_frame((5 * 48, 80), 321).reshape(5, 48, 80),
          '3x70x77': lambda: np.concatenate([dc.sparse_frame((2, 70, 77), 322, 0.1), dc.camera_frame((1, 70, 77), 323)])}


@pytest.mark.parametrize('route', ['device', 'host'])
@pytest.mark.parametrize('which', sorted(STACKS))
def test_written_files_read_back(which, route, tmp_path, monkeypatch):
    """write_tiff with predictor 1 and 2, classic and BigTIFF, RowsPerStrip 1, the default (the whole page at these sizes)
    and 16 (a short last strip), on either route. Each file is read back by read_tiff on both inflate routes, by zlib strip
    by strip over tiff_info's tables, and by Pillow where it has libtiff (extra; the others always run); its size is
    header + strips + IFDs; the strips of a page follow one another."""
    stack = STACKS[which]()
    T, H, W = stack.shape
    skipped = None
    for predictor in (1, 2):
        for big in (False, True):
            for rps in (1, None, 16):
                path = str(tmp_path / f'{predictor}_{big}_{rps}.tif')
                src = torch.from_numpy(stack.view(np.int16)).to(DEV) if predictor == 1 else stack       # a device tensor, a host array
                w = write_tiff(path, src, rows_per_strip=rps, predictor=predictor, bigtiff=big, deflate=route, level=1)
                info = tiff.tiff_info(path)
                assert info.shape == stack.shape and info.bigtiff == big and info.predictor == predictor
                assert info.compression == tiff.COMPRESSION_ADOBE_DEFLATE and info.byteorder == '<' and not info.imagej
                per = -(-H // (rps or H))
                assert info.n_segments == T * per
                assert np.array_equal(tig.read_both_routes(path, monkeypatch), stack)
                data = open(path, 'rb').read()
                for k in range(info.n_segments):
                    o, n = int(info.src_offset[k]), int(info.src_bytes[k])
                    t, r0, r = int(info.frame[k]), int(info.row0[k]), int(info.rows[k])
                    assert zlib.decompress(data[o:o + n]) == dc.stored_bytes(stack[t, r0:r0 + r], predictor)
                o, n = info.src_offset.reshape(T, per), info.src_bytes.reshape(T, per)
                assert (o[:, 1:] == o[:, :-1] + n[:, :-1]).all()
                assert len(data) == (16 if big else 8) + w.strip_bytes + w.ifd_bytes and w.strip_bytes == int(info.src_bytes.sum())
                pages = pillow_pages(path)
                if pages is None:
                    skipped = 'Pillow with libtiff is not available: its comparison was skipped'
                else:
                    assert np.array_equal(pages, stack)
    if skipped:
        print(skipped)


def test_routing_chunks_and_a_two_dimensional_page(tmp_path, monkeypatch):
    """deflate=None asks deflate_on_device with every chunk's strip count; more frames than one chunk; [H,W] is one page;
    bigtiff=None writes classic TIFF for a small file; a description lands in page 0."""
    asked = []
    monkeypatch.setattr(tiff, 'deflate_on_device', lambda n: asked.append(n) or n > 100)
    stack = dc.sparse_frame((70, 8, 16), 331, 0.2)
    path = str(tmp_path / 't.tif')
    w = write_tiff(path, stack, rows_per_strip=3, description='seventy frames')
    assert asked == [192, 18] and w.pages == 70 and not w.big
    assert np.array_equal(read_tiff(path, device='cpu'), stack)
    assert b'seventy frames\0' in open(path, 'rb').read()
    write_tiff(path, torch.from_numpy(stack[3].view(np.int16)).to(DEV), deflate='device')
    assert tiff.tiff_info(path).shape == (1, 8, 16) and np.array_equal(read_tiff(path, device='cpu')[0], stack[3])
    assert tiff.choose_bigtiff(9000, 512, 512) and not tiff.choose_bigtiff(256, 512, 512)


def test_process_timelapse_against_the_numpy_restatement(tmp_path):
    """Notebook 01 on a written file: time slice, saturating offset, two masks, padding with an even and an odd difference
    (one short, as the notebook pads), slices, and the saved .npy; and a run with nothing asked for."""
    rng = np.random.default_rng(341)
    stack = (dc.camera_frame((6, 40, 52), 342).astype(np.int64) + dc.blobs_frame((6 * 40, 52), 343).reshape(6, 40, 52)).astype(np.uint16)
    stack[0, 0, 0], stack[1, 3, 3] = 65535, 40000                         # (above the int16 range)
    src = str(tmp_path / 'rec_compr.deflate.tif')
    write_tiff(src, stack, predictor=2)
    mask, second = rng.random((40, 52)) < 0.7, rng.random((40, 52)) < 0.9
    np.save(tmp_path / 'mask.npy', mask)
    runs = [dict(timeslice=(1, 5), offset=121, mask=str(tmp_path / 'mask.npy'), second_mask=second, to_shape=(48, 61),
                 H_slice=(2, 44), W_slice=(1, 59)),
            dict(offset=135, mask=mask, to_shape=(45, 52), H_slice=(3, 40)),
            dict()]
    for k, kw in enumerate(runs):
        dest = str(tmp_path / f'out{k}')
        got, got_mask = axtrack_amd.process_timelapse(src, dest, device=DEV, deflate='device', **kw)
        ref_kw = dict(kw)
        ts = ref_kw.pop('timeslice', None)
        if isinstance(ref_kw.get('mask'), str):
            ref_kw['mask'] = np.load(ref_kw['mask'])
        want, want_mask = dc.ref_process(stack if ts is None else stack[ts[0]:ts[1]], **ref_kw)
        assert got.dtype == torch.int16 and got.is_cuda and np.array_equal(got.cpu().numpy().view(np.uint16), want)
        assert np.array_equal(read_tiff(dest + '.tif', device='cpu'), want)
        if 'mask' in kw:
            assert got_mask.dtype == bool and np.array_equal(got_mask, want_mask) and np.array_equal(np.load(dest + '.npy'), want_mask)
        else:
            assert got_mask is None and not os.path.exists(dest + '.npy')
    assert dc.ref_process(stack, to_shape=(45, 52))[0].shape == (6, 44, 52)     # the odd difference ends one short
    with pytest.raises(ValueError, match='smaller'):
        axtrack_amd.process_timelapse(src, str(tmp_path / 'no'), to_shape=(30, 52), device=DEV)


def test_prepare_input_data_on_a_written_file(tmp_path):
    raw = tg.raw_counts(synth.synth_frames(7, 96, 130, seed=351))
    np.save(tmp_path / 't.npy', raw)
    write_tiff(str(tmp_path / 't.tif'), raw, rows_per_strip=8, deflate='device')
    P = params.load_parameters()
    P['DEVICE'] = DEV
    meta = {'intensity_offset': 121, 'clip_intensity': 55, 'pad': 3}
    a, b = (axtrack_amd.prepare_input_data(name, P, str(tmp_path), str(tmp_path), params.DEPLOYED_STND_SCALER,
                                           use_cached_datasets=None, input_metadata=meta) for name in ('t.tif', 't.npy'))
    assert a.frames.shape == (7, 102, 136) and torch.equal(a.frames, b.frames) and float(a.frames.abs().max()) > 0
