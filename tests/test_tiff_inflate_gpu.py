"""Deflate TIFF strips inflated on the GPU (csrc/tiff_inflate.hip, csrc/axt_tiff_inflate.h). Inflating is
integer work: every comparison is exact equality with the array the strip or file was made from, every status that of the
reference inflater of tests/tiff_inflate_cases.py, which tests/test_tiff_inflate_cpu.py holds against zlib and whose
battery the host program has run under the sanitizers. Files come from the test writer in tmp_path or from
tests/golden/tiff (Pillow / libtiff)."""
import glob
import os
import time
import zlib

import numpy as np
import pytest
import torch

import test_entry_conventions_gpu as proto
import test_tiff_gpu as tg
import tiff_cases as tc
import tiff_inflate_cases as ic
import axtrack_amd
from axtrack_amd import _lib, hotpath, params, synth, tiff
from axtrack_amd.tiff import TiffError, read_tiff

pytestmark = pytest.mark.gpu
DEV = tg.DEV
PATTERN = tg.PATTERN


@pytest.fixture(scope='module')
def cases():
    return ic.inflate_cases()


class Launch(tg.Launch):
    """The launch layout and the checks of tests/test_tiff_gpu.py (canaries on both ends, gaps between the segments,
    everything pre-filled), through axt_tiff_inflate_u16."""

    def run(self, predictor=1, big_endian=False, src_len=None):
        d_src = torch.from_numpy(self.blob.copy()).to(DEV)
        out = torch.full((self.out_len,), PATTERN, dtype=torch.int16, device=DEV)
        status = torch.full((len(self.segs),), 77, dtype=torch.int32, device=DEV)
        lib = _lib.load()
        d_segs = torch.from_numpy(self.rec.view(np.uint8).copy()).to(DEV)
        rc = lib.axt_tiff_inflate_u16(d_src.data_ptr(), d_src.numel() if src_len is None else src_len, d_segs.data_ptr(),
                                      len(self.segs), self.W, predictor, int(big_endian), out.data_ptr(), out.numel(),
                                      status.data_ptr(), None)
        assert rc == 0, lib.axt_last_error()
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint16), status.cpu().numpy()


def test_the_whole_battery(cases):
    """Every case of the battery, one launch per (W, predictor, byte order) -- what a launch fixes --, the segments in the
    battery's order, so the malformed strips of W = 80 sit among good ones; two descriptors that are out of range stand
    among them. Statuses are the reference's, the good segments' samples equal theirs, and every element outside the
    segments' ranges, and inside the refused descriptors', is unchanged."""
    groups = {}
    for c in cases:
        groups.setdefault((c.W, c.predictor, c.big_endian), []).append(c)
    assert len(groups[(80, 1, False)]) > 40 and sum(len(g) for g in groups.values()) == len(cases)
    for (W, predictor, big_endian), segs in groups.items():
        want = [c.status for c in segs]
        la = Launch(segs, W)
        if len(segs) > 40:
            good = [k for k, c in enumerate(segs) if c.status == ic.OK and c.rows]
            k0, k1 = good[3], good[len(good) // 2]
            la.rec['src_offset'][k0] = -1                                 # a negative field
            la.rec['dst_offset'][k1] = la.out_len - segs[k1].rows * W + 1     # one element past out_len
            want[k0] = want[k1] = ic.BAD_SEGMENT
        out, status = la.run(predictor, big_endian)
        la.check(out, status, want)


def test_malformed_segments_between_good_ones_raise_through_the_wrapper(cases):
    by_name = {c.name: c for c in cases}
    sp = tc.sparse((16, 80), 0.1, 131)
    good = [ic._case(f'good{i}', ic.deflate(ic.raw_of(a)), a) for i, a in enumerate((sp, tc.noise((16, 80), 132), sp[::-1].copy()))]
    segs = [good[0], by_name['cut_default_2_of_4'], good[1], by_name['wrong_adler'], by_name['symbol_286'], good[2],
            by_name['literal_after_completion']]
    la = Launch(segs, 80)
    want = [0, 1, 0, 5, 2, 0, 3]
    la.check(*la.run(), want)
    d_src = torch.from_numpy(la.blob.copy()).to(DEV)
    o = torch.full((la.out_len,), PATTERN, dtype=torch.int16, device=DEV)
    frame, row0 = np.arange(7) // 2, (np.arange(7) % 2) * 16
    with pytest.raises(TiffError, match=r'frame 0, row 16 \(segment 1\).*status 1; 4 of 7 segments fail'):
        hotpath.tiff_decode_u16(d_src, la.rec, 80, tc.ADOBE_DEFLATE, 1, False, o, frame, row0)
    la.check(o.cpu().numpy().view(np.uint16), np.array(want), want)
    la = Launch([good[0], by_name['wrong_adler'], good[1]], 80)
    with pytest.raises(TiffError, match=r'segment 1 does not decode: checksum.*status 5; 1 of 3 segments fail'):
        hotpath.tiff_decode_u16(torch.from_numpy(la.blob.copy()).to(DEV), la.rec, 80, tc.DEFLATE, 1, False,
                                torch.full((la.out_len,), PATTERN, dtype=torch.int16, device=DEV))


def test_more_segments_than_blocks(cases):
    """2049 strips of one row: the grid of 2048 blocks strides, block 0 inflates segment 0 and then segment 2048 with the
    same LDS. Segment 0 is a dynamic block with a long code set (286 codes of 8 and 9 bits over a row of noise; zlib
    itself stores so short a row, so the block is hand-assembled), segment 2048 a dynamic block with two 1-bit codes,
    then in the other order on block 1's pair (1 and -- in a second launch of 4097 -- 2049); a table entry or ring byte
    left over from the first strip would show in the second."""
    W = 80
    noise_row, flat_row = tc.noise((1, W), 141), np.full((1, W), 0x4141, np.uint16)
    blk = ic.dynamic_block(ic.BitWriter(), ic.complete_lengths(286), [1], final=1).literals(ic.raw_of(noise_row)).end()
    long_set = ic._case('long', blk.bw.finish(ic.raw_of(noise_row)), noise_row)
    two = [0] * 0x41 + [1] + [0] * (256 - 0x42) + [1]                       # 1-bit codes for the byte 0x41 and end-of-block
    blk = ic.dynamic_block(ic.BitWriter(), two, [0], final=1).literals(ic.raw_of(flat_row)).end()
    short_set = ic._case('short', blk.bw.finish(ic.raw_of(flat_row)), flat_row)
    for c in (long_set, short_set):
        assert ic.first_block_type(c.src) == 2 and zlib.decompress(c.src) == ic.raw_of(c.expect)
    kinds = [dict(), dict(level=6, strategy=zlib.Z_FIXED), dict(level=0), dict(strategy=zlib.Z_RLE)]
    rows = tc.sparse((4097, 1, W), 0.2, 142)
    segs = [ic._case(f's{k}', ic.deflate(ic.raw_of(rows[k]), **kinds[k % 4]), rows[k]) for k in range(4097)]
    segs[0], segs[2048], segs[4096] = long_set, short_set, long_set
    segs[1], segs[2049] = short_set, long_set
    for n in (2049, 4097):
        la = Launch(segs[:n], W, gap=8)
        la.check(*la.run())


def test_inflate_on_a_side_stream_with_poisoned_allocations(monkeypatch):
    """The side-stream protocol of tests/test_entry_conventions_gpu.py, as tests/test_tiff_gpu.py applies it to the other
    codecs: the source buffer holds a decoy (another valid strip); on a non-blocking side stream a delay, the copy of the
    real bytes and the launch are enqueued in that order. A launch on any other stream runs during the delay and
    inflates the decoy. Allocations are poisoned during the call."""
    delay = proto.Delay()
    real = ic._case('real', ic.deflate(ic.raw_of(tc.sparse((40, 80), 0.1, 151), 2, True)), tc.sparse((40, 80), 0.1, 151), 2, True)
    decoy_src = ic.deflate(ic.raw_of(tc.sparse((40, 80), 0.1, 152), 2, True))
    n = max(len(real.src), len(decoy_src))
    la = Launch([real], 80)
    rec = la.rec.copy()
    rec['src_offset'], rec['src_bytes'] = 0, n                             # (bytes behind the checksum are ignored)
    pad = lambda b: torch.from_numpy(np.frombuffer(bytes(b).ljust(n, b'\0'), np.uint8).copy())

    def run(d_src, out, status):
        return hotpath.tiff_decode_launch(d_src, rec, 80, tc.ADOBE_DEFLATE, 2, True, out, status)

    base = torch.full((la.out_len,), PATTERN, dtype=torch.int16, device=DEV)
    st = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    run(pad(real.src).to(DEV), base, st)
    torch.cuda.synchronize()
    la.check(base.cpu().numpy().view(np.uint16), st.cpu().numpy())
    d_src = pad(decoy_src).to(DEV)
    staging = pad(real.src).to(DEV)
    out = torch.full((la.out_len,), PATTERN, dtype=torch.int16, device=DEV)
    st2 = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        delay.enqueue()
        d_src.copy_(staging, non_blocking=True)
        t0 = time.perf_counter()
        with proto.poisoned_allocations(monkeypatch, 1):
            keep = run(d_src, out, st2)
        seconds = time.perf_counter() - t0
        busy = not side.query()
        side.synchronize()
    print(f'\n{seconds * 1e3:.2f} ms to enqueue the launch behind a delay of {delay.ms:.1f} ms')
    assert busy, 'the launch waited for the stream'
    assert seconds * 1e3 <= delay.ms / proto.MARGIN
    assert torch.equal(out, base) and int(st2[0]) == 0
    del keep


# ------------------------------------------------------------------------------------------------ files
def read_both_routes(path, monkeypatch, **kw):
    """read_tiff with every pack inflated on the device, then on the host; both asked for, both identical."""
    got = {}
    for route in (True, False):
        asked = []
        monkeypatch.setattr(tiff, 'inflate_on_device', lambda n, route=route: asked.append(n) or route)
        got[route] = read_tiff(path, device=DEV, **kw)
        assert asked, 'the packer did not ask inflate_on_device'
    assert got[True].dtype == torch.int16 and got[True].is_contiguous() and torch.equal(got[True], got[False])
    return got[True].cpu().numpy().view(np.uint16)


@pytest.fixture(scope='module')
def stack50():
    return tc.sparse((3, 50, 77), 0.1, 161)


@pytest.mark.parametrize('kw', [
    dict(compression=tc.ADOBE_DEFLATE, rows_per_strip=16), dict(compression=tc.DEFLATE, rows_per_strip=16),
    dict(compression=tc.ADOBE_DEFLATE, rows_per_strip=1, byteorder='>'),
    dict(compression=tc.DEFLATE, rows_per_strip=7, byteorder='>', predictor=2, odd_offsets=True, bigtiff=True),
    dict(compression=tc.ADOBE_DEFLATE, predictor=2, odd_offsets=True), dict(compression=tc.DEFLATE, bigtiff=True),
    dict(compression=tc.ADOBE_DEFLATE, rows_per_strip=7, predictor=2, byteorder='>'),
], ids=lambda kw: '-'.join(f'{v}' for v in kw.values()))
def test_read_tiff_on_writer_variants(kw, stack50, tmp_path, monkeypatch):
    """Compression 8 and 32946, both byte orders, BigTIFF, predictor 2 at W = 77, strips at odd file offsets, RowsPerStrip
    1, 7, 16 (short last strips) and the whole page."""
    path = str(tmp_path / 't.tif')
    tc.write_tiff(path, stack50, **kw)
    assert np.array_equal(read_both_routes(path, monkeypatch), stack50)


@pytest.mark.parametrize('fname', sorted(os.path.basename(f) for f in glob.glob(os.path.join(tc.GOLDEN, '*deflate*.tif'))))
def test_golden_deflate_files(fname, monkeypatch):
    src = np.load(os.path.join(tc.GOLDEN, fname[:fname.index('_', fname.index('x'))] + '.npy'))
    assert np.array_equal(read_both_routes(os.path.join(tc.GOLDEN, fname), monkeypatch), src)


def test_golden_deflate_set():
    assert len(glob.glob(os.path.join(tc.GOLDEN, '*deflate*.tif'))) == 4


def test_default_route_frame_ranges_and_a_corrupted_strip(tmp_path):
    """No routing forced: read_tiff as users call it. More frames than one chunk of 64 (192 strips and then 18: the
    device, then the host); a frame range; device='cpu'; a strip whose second half is zeroed raises TiffError with that
    strip's frame and row, from the status read at the end where the pack is the device's (100 strips), from zlib where
    it is the host's (40)."""
    path = str(tmp_path / 't.tif')
    long = tc.sparse((70, 8, 16), 0.2, 171)
    tc.write_tiff(path, long, compression=tc.ADOBE_DEFLATE, rows_per_strip=3)
    assert tiff.inflate_on_device(192) and not tiff.inflate_on_device(18)
    got = read_tiff(path, device=DEV)
    assert np.array_equal(got.cpu().numpy().view(np.uint16), long)
    assert np.array_equal(read_tiff(path, frames=range(65, 69), device='cpu'), long[65:69])
    five = tc.noise((5, 20, 33), 172)
    layout = tc.write_tiff(path, five, compression=tc.ADOBE_DEFLATE, rows_per_strip=1, predictor=2)
    data = bytearray(open(path, 'rb').read())
    o, n = layout[2][0][8], layout[2][1][8]
    data[o + n // 2:o + n] = b'\0' * (n - n // 2)
    open(path, 'wb').write(data)
    assert tiff.inflate_on_device(100) and not tiff.inflate_on_device(40)
    with pytest.raises(TiffError, match=r'frame 2, row 8 \(segment 48\) does not decode.*1 of 100 segments fail'):
        read_tiff(path, device=DEV)
    with pytest.raises(TiffError, match=r'frame 2, row 8 at offset \d+ does not inflate'):
        read_tiff(path, frames=range(1, 3), device=DEV)
    assert np.array_equal(read_tiff(path, frames=range(0, 2), device='cpu'), five[:2])     # the frames before it still read


def test_from_tiff_and_prepare_input_data_on_a_deflate_file(tmp_path):
    raw = tg.raw_counts(synth.synth_frames(7, 96, 130, seed=181))
    np.save(tmp_path / 't.npy', raw)
    tc.write_tiff(str(tmp_path / 't.tif'), raw, compression=tc.ADOBE_DEFLATE, rows_per_strip=8, bigtiff=True)     # 84 strips: the device
    assert tiff.inflate_on_device(tiff.tiff_info(str(tmp_path / 't.tif')).n_segments)
    P = params.load_parameters()
    P['DEVICE'] = DEV
    meta = {'intensity_offset': 121, 'clip_intensity': 55, 'pad': 3}
    a, b = (axtrack_amd.prepare_input_data(name, P, str(tmp_path), str(tmp_path), params.DEPLOYED_STND_SCALER,
                                           use_cached_datasets=None, input_metadata=meta) for name in ('t.tif', 't.npy'))
    assert a.frames.shape == (7, 102, 136) and torch.equal(a.frames, b.frames) and float(a.frames.abs().max()) > 0
    scale = params.DEPLOYED_STND_SCALER[1][0]
    small = tg.raw_counts(synth.synth_frames(150, 40, 64, seed=182, n_blobs=4))
    spath = str(tmp_path / 's.tif')
    tc.write_tiff(spath, small, compression=tc.DEFLATE, rows_per_strip=16, byteorder='>', predictor=2)
    x = axtrack_amd.Timelapse.from_tiff(spath, scale=scale, chunk_frames=40).make_resident()
    y = axtrack_amd.Timelapse.from_host_u16(small, scale=scale, chunk_frames=40).make_resident()
    assert not x._pending and torch.equal(x.frames, y.frames) and float(x.frames.abs().max()) > 0
