"""TIFF strips decoded on the GPU (csrc/tiff.hip, include/axtrack_hip_tiff.h). Decoding is integer work:
every comparison is exact equality with the array the file or strip was made from. The strip cases are those of
tiff_cases.decode_cases(), which the host program of tests/test_tiff_cpu.py has run under the sanitizers; files come
from the test writer in tmp_path or from tests/golden/tiff (Pillow / libtiff)."""
import glob
import os
import time

import numpy as np
import pytest
import torch

import scaler_reference as sr
import test_entry_conventions_gpu as proto
import tiff_cases as tc
import axtrack_amd
from axtrack_amd import _lib, hotpath, params, synth, tiff
from axtrack_amd.tiff import TIFF_SEGMENT_DTYPE, TiffError, read_tiff

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CANARY, PATTERN = 4096, 0x5AA5
AXT_EINVAL = -22


@pytest.fixture(scope='module')
def cases():
    return {c.name: c for c in tc.decode_cases()}


class Launch:
    """Segments for one launch: their bytes packed back to back behind one pad byte (so offsets come out odd and even),
    their output ranges `gap` elements apart between two canaries, everything pre-filled with PATTERN."""

    def __init__(self, segs, W, gap=64):
        self.segs, self.W = segs, W
        self.rec = np.zeros(len(segs), TIFF_SEGMENT_DTYPE)
        blob, pos = bytearray(b'\xee'), CANARY
        for k, c in enumerate(segs):
            self.rec[k] = (len(blob), len(c.src), pos, c.rows, 0)
            blob += c.src
            pos += c.rows * W + gap
        self.out_len = pos - gap + CANARY
        self.blob = np.frombuffer(bytes(blob), np.uint8)

    def run(self, compression, predictor=1, big_endian=False, src_len=None):
        d_src = torch.from_numpy(self.blob.copy()).to(DEV)
        out = torch.full((self.out_len,), PATTERN, dtype=torch.int16, device=DEV)
        status = torch.full((len(self.segs),), 77, dtype=torch.int32, device=DEV)
        lib = _lib.load()
        d_segs = torch.from_numpy(self.rec.view(np.uint8).copy()).to(DEV)
        rc = lib.axt_tiff_decode_u16(d_src.data_ptr(), d_src.numel() if src_len is None else src_len, d_segs.data_ptr(),
                                     len(self.segs), self.W, compression, predictor, int(big_endian), out.data_ptr(), out.numel(),
                                     status.data_ptr(), None)
        assert rc == 0, lib.axt_last_error()
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint16), status.cpu().numpy()

    def check(self, out, status, expect_status=None):
        """Statuses, the good segments' samples, and everything that must be untouched: both canaries, the gaps between
        the segments, and the range of a segment whose descriptor was refused."""
        want = [c.status for c in self.segs] if expect_status is None else expect_status
        assert status.tolist() == want
        touched = np.zeros(self.out_len, bool)
        for k, c in enumerate(self.segs):
            a0 = int(self.rec['dst_offset'][k])
            n = c.rows * self.W
            if want[k] == tc.OK:
                assert np.array_equal(out[a0:a0 + n].reshape(c.rows, self.W), c.expect), c.name
            if want[k] != tc.BAD_SEGMENT:
                touched[a0:a0 + n] = True
        assert (out[~touched] == PATTERN).all(), 'a write outside the segments'
        assert not touched[:CANARY].any() and not touched[-CANARY:].any()


GOOD = ['lzw_noise_64x80', 'lzw_sparse_256x160', 'lzw_zeros_64x80', 'lzw_no_leading_clear', 'lzw_no_eoi', 'lzw_big_endian_pred2_w77',
        'lzw_pred2_w300', 'packbits_handmade', 'packbits_sparse_50x77', 'packbits_noise_be_pred2', 'raw_big_endian_pred2_w77',
        'raw_big_endian_w300', 'raw_little_endian_pred2', 'one_sample', 'empty_segment']


@pytest.mark.parametrize('name', GOOD)
def test_one_segment(name, cases):
    """n_segs = 1, each mechanism at the smallest size at which it can fail: >4094 codes (all four widths, a table reset),
    an output beyond 64 KiB with strings of hundreds of bytes and self-referencing codes, the longest strings (all zero),
    no leading Clear, no EOI, PackBits' run lengths 1 / 2 / 128 and its no-op header, odd row bytes with the predictor's
    carry across a 64-lane chunk (W = 77) and over several chunks (W = 300), both byte orders."""
    c = cases[name]
    la = Launch([c], c.W)
    la.check(*la.run(c.compression, c.predictor, c.big_endian))


def test_good_list_is_every_good_case(cases):
    assert sorted(GOOD) == sorted(n for n, c in cases.items() if c.status == tc.OK)


def test_malformed_segments_among_good_ones(cases):
    """A truncated strip (1), a code above the next free entry (2), a strip that decodes to more than its rows (3) and a
    descriptor past src_len (4), each between good segments of the same launch: the good ones decode, every status is
    the reference decoder's, nothing outside the segments' own ranges is written, and the refused descriptor's range is
    not written at all. The wrapper raises TiffError naming the first failing segment's frame and row."""
    sp = tc.sparse((16, 80), 0.1, 31)
    good = [tc._good(f'good{i}', a, tc.LZW) for i, a in enumerate((sp, tc.noise((8, 80), 32), np.zeros((16, 80), np.uint16), sp[::-1].copy()))]
    past = tc._good('descriptor_past_src_len', sp, tc.LZW)
    segs = [good[0], cases['lzw_truncated'], good[1], cases['lzw_code_above_next'], good[2], cases['lzw_too_many_rows'], good[3], past]
    la = Launch(segs, 80)
    assert int(la.rec['src_offset'][-1] + la.rec['src_bytes'][-1]) == len(la.blob)
    want = [0, 1, 0, 2, 0, 3, 0, 4]
    out, status = la.run(tc.LZW, src_len=len(la.blob) - 1)                # the last segment ends one byte past src_len
    la.check(out, status, want)
    # the wrapper: statuses read once, the first failing segment named by frame and row
    d_src = torch.from_numpy(la.blob.copy()).to(DEV)[:len(la.blob) - 1]
    o = torch.full((la.out_len,), PATTERN, dtype=torch.int16, device=DEV)
    frame, row0 = np.arange(8) // 2, (np.arange(8) % 2) * 16
    with pytest.raises(TiffError, match=r'frame 0, row 16 \(segment 1\).*status 1; 4 of 8 segments fail'):
        hotpath.tiff_decode_u16(d_src.contiguous(), la.rec, 80, tc.LZW, 1, False, o, frame, row0)
    la.check(o.cpu().numpy().view(np.uint16), np.array(want), want)
    # a descriptor whose output would pass out_len, and negative fields
    rec = la.rec.copy()
    la.rec['dst_offset'][6] = la.out_len - 16 * 80 + 1
    la.rec['src_offset'][4] = -1
    out, status = la.run(tc.LZW, src_len=len(la.blob) - 1)
    assert status.tolist() == [0, 1, 0, 2, 4, 3, 4, 4]
    la.rec = rec
    touched = np.zeros(la.out_len, bool)
    for k in (0, 1, 2, 3, 5):
        a0 = int(rec['dst_offset'][k])
        touched[a0:a0 + segs[k].rows * 80] = True
    assert (out[~touched] == PATTERN).all()


def test_every_malformed_case_gives_its_status(cases):
    """Each malformed stream the host program has decoded under the sanitizers, alone in a launch: the status is the
    reference decoder's and nothing outside the segment's own rows * W samples is written."""
    bad = [c for c in cases.values() if c.status != tc.OK]
    assert len(bad) >= 8
    for c in bad:
        la = Launch([c], c.W)
        la.check(*la.run(c.compression, c.predictor, c.big_endian))


def test_entry_point_refuses_bad_arguments_before_any_launch(cases):
    c = cases['lzw_zeros_64x80']
    la = Launch([c], c.W)
    lib = _lib.load()
    d_src = torch.from_numpy(la.blob.copy()).to(DEV)
    d_segs = torch.from_numpy(la.rec.view(np.uint8).copy()).to(DEV)
    out = torch.full((la.out_len,), PATTERN, dtype=torch.int16, device=DEV)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    good = [d_src.data_ptr(), d_src.numel(), d_segs.data_ptr(), 1, c.W, tc.LZW, 1, 0, out.data_ptr(), out.numel(), status.data_ptr(), None]
    for pos, value in ((0, None), (2, None), (8, None), (10, None), (1, -1), (3, -1), (4, -1), (9, -1), (5, 7), (5, 8), (5, 0),
                       (6, 0), (6, 3)):
        args = list(good)
        args[pos] = value
        assert lib.axt_tiff_decode_u16(*args) == AXT_EINVAL
        assert lib.axt_last_error().startswith(b'axt_tiff_decode_u16: ')
    torch.cuda.synchronize()
    assert (out == PATTERN).all() and int(status[0]) == 77


# ------------------------------------------------------------------------------------------------ files
def assert_reads(path, stack, **kw):
    got = read_tiff(path, device=DEV, **kw)
    assert got.dtype == torch.int16 and got.is_cuda and got.is_contiguous() and tuple(got.shape) == stack.shape
    assert np.array_equal(got.cpu().numpy().view(np.uint16), stack)


@pytest.fixture(scope='module')
def stack50():
    return tc.sparse((3, 50, 77), 0.1, 41)


@pytest.mark.parametrize('kw', [
    dict(compression=tc.LZW, rows_per_strip=16), dict(compression=tc.LZW, rows_per_strip=1),
    dict(compression=tc.LZW, rows_per_strip=16, byteorder='>', predictor=2, odd_offsets=True),
    dict(compression=tc.LZW, predictor=2), dict(compression=tc.PACKBITS, rows_per_strip=16, odd_offsets=True),
    dict(compression=tc.PACKBITS, byteorder='>', predictor=2, rows_per_strip=1),
    dict(compression=tc.NONE), dict(compression=tc.NONE, rows_per_strip=16, odd_offsets=True),
    dict(compression=tc.NONE, byteorder='>', predictor=2, rows_per_strip=16, odd_offsets=True),
    dict(compression=tc.NONE, predictor=2), dict(compression=tc.LZW, bigtiff=True, byteorder='>', rows_per_strip=7),
    dict(compression=tc.ADOBE_DEFLATE, rows_per_strip=16), dict(compression=tc.DEFLATE, byteorder='>', predictor=2, odd_offsets=True),
], ids=lambda kw: '-'.join(f'{v}' for v in kw.values()))
def test_read_tiff_on_writer_variants(kw, stack50, tmp_path):
    """H = 50 with RowsPerStrip 16 (a short last strip) and 1, both byte orders with predictor 2 at W = 77, strips at odd
    file offsets, BigTIFF, the plain-copy route (little-endian, uncompressed, no predictor), Deflate through the host."""
    path = str(tmp_path / 't.tif')
    tc.write_tiff(path, stack50, **kw)
    assert_reads(path, stack50)


def test_read_tiff_w300_many_segments_imagej_and_frame_ranges(tmp_path):
    path = str(tmp_path / 't.tif')
    wide = tc.noise((2, 9, 300), 42)
    tc.write_tiff(path, wide, compression=tc.LZW, byteorder='>', predictor=2, rows_per_strip=4)
    assert_reads(path, wide)
    # 3000 segments of 16 samples: more segments than blocks, the grid strides
    many = tc.sparse((30, 100, 16), 0.3, 43)
    tc.write_tiff(path, many, compression=tc.LZW, rows_per_strip=1)
    assert tiff.tiff_info(path).n_segments == 3000
    assert_reads(path, many)
    # ImageJ's single-IFD layout, images=5, big-endian as ImageJ writes, and little-endian (one plain copy)
    five = tc.noise((5, 20, 33), 44)
    for bo in '><':
        tc.write_tiff(path, five, imagej=True, byteorder=bo, odd_offsets=True)
        assert tiff.tiff_info(path).imagej
        assert_reads(path, five)
    # frames: a range or a slice of pages; device='cpu': a numpy array by the same route
    tc.write_tiff(path, five, compression=tc.LZW, rows_per_strip=8)
    got = read_tiff(path, frames=range(1, 3), device=DEV)
    assert np.array_equal(got.cpu().numpy().view(np.uint16), five[1:3])
    got = read_tiff(path, frames=slice(3, None), device='cpu')
    assert isinstance(got, np.ndarray) and got.dtype == np.uint16 and np.array_equal(got, five[3:])
    with pytest.raises(IndexError):
        read_tiff(path, frames=range(4, 6), device=DEV)
    # more frames than one chunk of 64
    long = tc.sparse((70, 8, 16), 0.2, 45)
    tc.write_tiff(path, long, compression=tc.PACKBITS)
    assert_reads(path, long)
    # a strip that does not decode: TiffError with the frame and the row, raised by read_tiff
    layout = tc.write_tiff(path, five, compression=tc.LZW, rows_per_strip=8)
    data = bytearray(open(path, 'rb').read())
    o, n = layout[2][0][1], layout[2][1][1]
    data[o + n // 2:o + n] = b'\xff' * (n - n // 2)
    open(path, 'wb').write(data)
    with pytest.raises(TiffError, match='frame 2, row 8'):
        read_tiff(path, device=DEV)


@pytest.mark.parametrize('fname', sorted(os.path.basename(f) for f in glob.glob(os.path.join(tc.GOLDEN, '*.tif'))))
def test_golden_files(fname):
    src = np.load(os.path.join(tc.GOLDEN, fname[:fname.index('_', fname.index('x'))] + '.npy'))
    assert_reads(os.path.join(tc.GOLDEN, fname), src)


# ------------------------------------------------------------------------------------------------ conventions
@pytest.fixture(scope='module')
def delay():
    return proto.Delay()


def test_decode_on_a_side_stream_with_poisoned_allocations(cases, delay, monkeypatch):
    """The side-stream protocol of tests/test_entry_conventions_gpu.py: the source buffer holds a decoy (another valid
    strip); on a non-blocking side stream a delay, the copy of the real bytes and the decode are enqueued in that order.
    A launch on any other stream runs during the delay and decodes the decoy. Allocations are poisoned during the call."""
    real = tc._good('real', tc.sparse((40, 80), 0.1, 51), tc.LZW, 2, True)
    decoy_src = tc.encode_strip(tc.sparse((40, 80), 0.1, 52), tc.LZW, 2, True)
    n = max(len(real.src), len(decoy_src))
    la = Launch([real], 80)
    rec = la.rec.copy()
    rec['src_offset'], rec['src_bytes'] = 0, n
    pad = lambda b: torch.from_numpy(np.frombuffer(bytes(b).ljust(n, b'\0'), np.uint8).copy())

    def run(d_src, out, status):
        return hotpath.tiff_decode_launch(d_src, rec, 80, tc.LZW, 2, True, out, status)

    # default stream: the baseline
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
    print(f'\n{seconds * 1e3:.2f} ms to enqueue the decode behind a delay of {delay.ms:.1f} ms')
    assert busy, 'the decode waited for the stream'
    assert seconds * 1e3 <= delay.ms / proto.MARGIN
    assert torch.equal(out, base) and int(st2[0]) == 0
    del keep


# ------------------------------------------------------------------------------------------------ end to end
def raw_counts(f0):
    scale = params.DEPLOYED_STND_SCALER[1][0]
    return np.clip((2.0 ** (f0 * scale) - 1.0) * 65535.0 + 121.0 * (f0 > 0), 0, 65535).astype(np.uint16)


def test_prepare_input_data_reads_a_tif_without_tifffile(tmp_path):
    raw = raw_counts(synth.synth_frames(7, 96, 130, seed=61))
    np.save(tmp_path / 't.npy', raw)
    tc.write_tiff(str(tmp_path / 't.tif'), raw, compression=tc.LZW, rows_per_strip=16, byteorder='>', predictor=2)
    P = params.load_parameters()
    P['DEVICE'] = DEV
    meta = {'intensity_offset': 121, 'clip_intensity': 55, 'pad': 3}
    a, b = (axtrack_amd.prepare_input_data(name, P, str(tmp_path), str(tmp_path), params.DEPLOYED_STND_SCALER,
                                           use_cached_datasets=None, input_metadata=meta) for name in ('t.tif', 't.npy'))
    assert a.frames.shape == (7, 102, 136) and torch.equal(a.frames, b.frames) and float(a.frames.abs().max()) > 0
    # read_tiff's output goes into preprocess and estimate_stnd_scaler as it is
    d = read_tiff(str(tmp_path / 't.tif'), device=DEV)
    from axtrack_amd.timelapse import preprocess, estimate_stnd_scaler
    assert torch.equal(preprocess(d, offset=121, clip=55), preprocess(raw, offset=121, clip=55))
    assert estimate_stnd_scaler(d)[0] == estimate_stnd_scaler(raw)[0]
    # a file the reader refuses, where tifffile is absent: the refusal names what the file uses
    tc.write_tiff(str(tmp_path / 'f.tif'), raw, tags_override={339: (3, [3])})
    try:
        import tifffile  # noqa: F401
    except ImportError:
        with pytest.raises(tiff.TiffUnsupported, match='SampleFormat 3'):
            axtrack_amd.prepare_input_data('f.tif', P, str(tmp_path), str(tmp_path), params.DEPLOYED_STND_SCALER, use_cached_datasets=None)
    # segment_mask takes the file name too
    img = synth.transmission_image(synth.corridor_mask(96, 128, 24, 48), seed=3)
    tc.write_tiff(str(tmp_path / 'm.tif'), img[None], compression=tc.PACKBITS)
    assert np.array_equal(axtrack_amd.segment_mask(str(tmp_path / 'm.tif'), (60, 10)), axtrack_amd.segment_mask(img, (60, 10)))


def test_from_tiff_streams_to_the_same_detections(weights, tmp_path):
    """Timelapse.from_tiff through AxonDetections.detect_dataset() against from_host_u16 of the same array: frames, YOLO
    grids, detections and identities identical (T = 12, 512 x 512, LZW)."""
    raw = raw_counts(synth.synth_frames(12, 512, 512, seed=62))
    path = str(tmp_path / 't.tif')
    layout = tc.write_tiff(path, raw, compression=tc.LZW, rows_per_strip=64)
    model = axtrack_amd.Detector(weights, max_batch=16)
    P = params.load_parameters()
    scale = params.DEPLOYED_STND_SCALER[1][0]
    host = axtrack_amd.Timelapse.from_host_u16(raw, name='x', offset=121, clip=55, scale=scale, chunk_frames=7)
    ref = axtrack_amd.inference(host, model, None, P, None, None, None)
    tl = axtrack_amd.Timelapse.from_tiff(path, name='x', offset=121, clip=55, scale=scale, chunk_frames=7)
    assert tl._pending and len(tl) == 8
    ad = axtrack_amd.inference(tl, model, None, P, None, None, None)
    assert not tl._pending and torch.equal(tl.frames, host.frames)
    assert ad.tile_yx == ref.tile_yx and torch.equal(ad._yolo, ref._yolo)
    for a, b in zip(ad._host_dets(), ref._host_dets()):
        assert np.array_equal(a, b)
    assert np.array_equal(ad._track_flat, ref._track_flat) and ad.mcf_total_cost == ref.mcf_total_cost
    # more than one piece of the stream, the last one short, frames smaller than a tile: the resident frames are the host path's
    small = raw_counts(synth.synth_frames(150, 40, 64, seed=64, n_blobs=4))
    spath = str(tmp_path / 's.tif')
    tc.write_tiff(spath, small, compression=tc.PACKBITS, rows_per_strip=16, byteorder='>')
    a = axtrack_amd.Timelapse.from_tiff(spath, scale=scale, chunk_frames=40).make_resident()
    b = axtrack_amd.Timelapse.from_host_u16(small, scale=scale, chunk_frames=40).make_resident()
    assert not a._pending and torch.equal(a.frames, b.frames) and float(a.frames.abs().max()) > 0
    # a strip that does not decode is reported once, after the last chunk
    data = bytearray(open(path, 'rb').read())
    o, n = layout[9][0][3], layout[9][1][3]
    data[o + n // 2:o + n] = b'\xff' * (n - n // 2)
    open(path, 'wb').write(data)
    with pytest.raises(TiffError, match='frame 9, row 192'):
        axtrack_amd.Timelapse.from_tiff(path, name='x', scale=scale).make_resident()


def test_prepare_training_data_reads_a_tif(tmp_path):
    T, H, W = 14, 40, 64
    raw = raw_counts(synth.synth_frames(T, H, W, seed=63, n_blobs=6))
    mask = np.zeros((H, W), np.uint16)
    mask[4:36, 8:60] = 300                                             # 0 / non-0 samples
    tc.write_tiff(str(tmp_path / 't.tif'), raw, compression=tc.PACKBITS, rows_per_strip=16)
    tc.write_tiff(str(tmp_path / 'm.tif'), mask[None], compression=tc.LZW)
    labels = str(tmp_path / 'labels.csv')
    x = np.arange(T, dtype=np.float64)[:, None] % W + np.zeros((1, 2))
    sr.write_labels_csv(labels, ['Axon_000', 'Axon_001'], x, x * 0 + 5)
    P = dict(LABELS_FILE=labels, TRAIN_TIMEPOINTS=[3, 4, 5, 6], TEST_TIMEPOINTS=[9, 10], OFFSET=121, CLIP_LOWERLIM=55,
             PAD=[0, 0, 0, 0], LOG_CORRECT=True, STANDARDIZE=('zscore', None), STANDARDIZE_FRAMEWISE=False, TEMPORAL_CONTEXT=2,
             TILESIZE=512, CACHE=None, DEVICE=DEV)
    a = axtrack_amd.prepare_training_data(P, TIMELAPSE_FILE=str(tmp_path / 't.tif'), MASK_FILE=str(tmp_path / 'm.tif'))
    b = axtrack_amd.prepare_training_data(P, TIMELAPSE_FILE=raw, MASK_FILE=mask != 0)
    for x, y in zip(a, b):
        assert torch.equal(x.frames, y.frames) and x.stnd_scaler == y.stnd_scaler and float(x.frames.abs().max()) > 0
        assert np.array_equal(x.mask2d, y.mask2d)
