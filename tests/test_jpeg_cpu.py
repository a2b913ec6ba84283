"""The JPEG / MJPEG output (axtrack_amd/jpeg.py, csrc/jpeg_encode.h) as far as it goes without a GPU: the
tables and the header against the reference's and Pillow's, the reference's streams in an independent decoder (Pillow's
libjpeg) and its quality against Pillow's own encoder, the encoder's arithmetic as a host program under AddressSanitizer
and UBSan, the AVI container through a RIFF parser of the test's own, and the bookkeeping of the new header."""
import inspect
import io
import os
import re
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import axtrack_amd
from axtrack_amd import _lib, hotpath, jpeg, render

import jpeg_cases as jc
import jpeg_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXT_EINVAL = -22
QUALITIES = (1, 25, 50, 75, 90, 100)
# decoded PSNR against the source, ours minus Pillow's own encoder with the same tables at 4:4:4: the issue's bound. The
# margin is for another integer DCT's rounding and nothing else.
PSNR_MARGIN_DB = 0.25


# ------------------------------------------------------------------------------------------------ tables and header
@pytest.mark.parametrize('quality', QUALITIES)
def test_tables_equal_the_references_and_pillows(quality):
    ours = jpeg.quant_tables(quality)
    assert ours.dtype == np.uint8 and ours.shape == (2, 64)
    assert tuple(map(tuple, ours.tolist())) == ref.quant_tables(quality)             # (itself checked against Pillow's file)
    header = jpeg.jpeg_header(13, 21, quality)
    assert header == ref.header(13, 21, quality)
    im = Image.open(io.BytesIO(header + b'\x00' * 8 + jpeg.EOI))                     # Pillow reads the header's tables back
    assert im.size == (21, 13) and im.mode == 'RGB'
    assert [list(im.quantization[k]) for k in (0, 1)] == ours.tolist()
    assert ref.dht_tables(header) == ref.huffman_specs()                             # the DHT of Pillow's optimize=False file
    assert {i: (list(b), list(v)) for i, b, v in jpeg.HUFFMAN} == ref.huffman_specs()


def test_header_layout():
    segs, end = ref.segments(jpeg.jpeg_header(100, 257, 90))
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert end == len(jpeg.jpeg_header(100, 257, 90))
    by = dict((m, p) for m, p in segs if m in (0xC0, 0xDD, 0xDA, 0xE0))
    assert by[0xE0][:5] == b'JFIF\x00'
    assert by[0xC0] == struct.pack('>BHHB', 8, 100, 257, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])   # 4:4:4
    assert by[0xDD] == struct.pack('>H', 33)                                         # one MCU row: ceil(257 / 8)
    assert by[0xDA] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert inspect.signature(jpeg.jpeg_header).parameters['quality'].default == 90
    assert inspect.signature(jpeg.jpeg_encode).parameters['quality'].default == 90
    for bad in (0, 101, -3):
        with pytest.raises(ValueError, match='quality'):
            jpeg.quant_tables(bad)
    for H, W in ((0, 5), (5, 0), (65536, 5), (5, 65536)):
        with pytest.raises(ValueError, match='65535'):
            jpeg.jpeg_header(H, W)


def test_launch_constants_are_the_kernels():
    src = open(os.path.join(ROOT, 'axtrack_amd', 'csrc', 'jpeg.hip')).read()
    val = lambda name: int(re.search(rf'constexpr int {name} = (\d+);', src).group(1))
    assert val('kJpegThreads') == jc.THREADS and val('kJpegMcusPerThread') == jc.MCUS_PER_THREAD
    assert val('kJpegStuffBytesPerThread') == jc.STUFF_BYTES_PER_THREAD
    assert 'kJpegStuffChunk = kJpegThreads * kJpegStuffBytesPerThread' in src
    assert src.count('__shared__') == 4 and all(s in src for s in ('__shared__ int part[kJpegThreads / 64]',
                                                                    '__shared__ long long part[kJpegThreads / 64]'))


# ------------------------------------------------------------------------------------------------ validity
def test_every_case_reaches_its_route():
    jc.check_facts()


@pytest.mark.parametrize('name', jc.case_names())
def test_reference_streams_open_in_pillow(name):
    _, rgb, quality, _ = next(c for c in jc.cases() if c[0] == name)
    for k, frame in enumerate(rgb):
        data = ref.header(frame.shape[0], frame.shape[1], quality) + jc.reference(name)[k][0] + b'\xff\xd9'
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (frame.shape[1], frame.shape[0]) and im.mode == 'RGB'
        assert np.asarray(im).shape == frame.shape


def pillow_psnr(rgb, quality):
    """PSNR of Pillow's own encoder with the same quantisation tables, 4:4:4, standard Huffman tables."""
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, 'JPEG', qtables=[list(t) for t in ref.quant_tables(quality)], subsampling=0, optimize=False)
    im = Image.open(io.BytesIO(buf.getvalue()))
    assert [list(im.quantization[k]) for k in (0, 1)] == [list(t) for t in ref.quant_tables(quality)]
    return ref.psnr(np.asarray(im), rgb)


@pytest.mark.parametrize('name', ['scene', 'noise_q100'])
def test_quality_matches_pillows_encoder(name):
    _, rgb, quality, _ = next(c for c in jc.cases() if c[0] == name)
    data = ref.header(rgb.shape[1], rgb.shape[2], quality) + jc.reference(name)[0][0] + b'\xff\xd9'
    ours = ref.psnr(np.asarray(Image.open(io.BytesIO(data))), rgb[0])
    theirs = pillow_psnr(rgb[0], quality)
    print(f'{name}: quality {quality}: {ours:.3f} dB, Pillow {theirs:.3f} dB, difference {ours - theirs:+.3f} dB')
    assert ours >= theirs - PSNR_MARGIN_DB


# ------------------------------------------------------------------------------------------------ the arithmetic, on the host
def test_encoder_core_on_the_host(tmp_path):
    """csrc/jpeg_encode.h -- colour, DCT, quantisation, the Huffman codes, padding, stuffing, markers: the functions the
    kernels run -- in a stand-alone program with its own main, built with AddressSanitizer and UBSan, on every case, pixels
    and output in heap blocks of their exact size."""
    case_file, exe = tmp_path / 'cases.bin', tmp_path / 'jpeg_encode_host'
    jc.write_case_file(str(case_file))
    subprocess.check_call(['/opt/rocm/bin/hipcc', '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g',
                           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                           f'-I{os.path.join(ROOT, "axtrack_amd", "csrc")}', os.path.join(ROOT, 'tests', 'jpeg_encode_host.cpp'),
                           '-o', str(exe)])
    res = subprocess.run([str(exe), str(case_file)], capture_output=True, text=True)
    print(res.stdout[-3000:], res.stderr[-3000:])
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    assert 'FAILED' not in res.stdout and 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    frames = sum(c[1].shape[0] for c in jc.cases())
    assert res.stdout.strip().endswith(f'{len(jc.cases())} cases, {frames} frames, 0 failures')


# ------------------------------------------------------------------------------------------------ the AVI container
@pytest.mark.parametrize('fps, scale, rate', [(6, 1, 6), (12.5, 2, 25)])
def test_avi_structure(fps, scale, rate, tmp_path):
    assert render._delay(fps) == (scale, rate)
    _, rgb, quality, _ = next(c for c in jc.cases() if c[0] == 'three_frames_strided')
    jpegs = [ref.encode(f, quality) for f in rgb]
    assert {len(j) & 1 for j in jpegs} == {0, 1}                                     # odd and even frames: the padding is used
    path = str(tmp_path / 'v.avi')
    assert jpeg.write_mjpeg_avi(path, jpegs, 10, 13, fps) == path
    data = open(path, 'rb').read()
    frames = jc.check_avi(data, 3, 10, 13, scale, rate)
    assert frames == jpegs
    for f, src in zip(frames, rgb):
        im = Image.open(io.BytesIO(f))
        im.load()
        assert im.size == (13, 10) and im.format == 'JPEG'


def test_avi_of_no_frames_and_the_size_refusal(tmp_path):
    path = str(tmp_path / 'v.avi')
    jpeg.write_mjpeg_avi(path, [], 8, 8, 6)
    jc.check_avi(open(path, 'rb').read(), 0, 8, 8, 1, 6)

    class Stub:                                             # a frame that only says how long it is
        def __len__(self):
            return 1 << 28

        def __bytes__(self):
            raise AssertionError('the size is checked before a byte is written')
    os.remove(path)
    with pytest.raises(ValueError, match=r'(?s)would take \d{10} bytes.*t_y_x_slice.*quality'):
        jpeg.write_mjpeg_avi(path, [Stub()] * 8, 8, 8, 6)
    assert not os.path.exists(path)
    assert jpeg.AVI_MAX_BYTES == 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ declarations
NEW_NAMES = {'axt_jpeg_scan_bound', 'axt_jpeg_scratch_bytes', 'axt_jpeg_encode_rgb8'}


def test_new_header_declares_and_binds_the_new_names():
    header = open(os.path.join(ROOT, 'include', 'axtrack_hip_jpeg.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert set(re.findall(r'\b(axt_\w+)\s*\(', code)) == NEW_NAMES
    main = open(os.path.join(ROOT, 'include', 'axtrack_hip.h')).read()
    assert re.search(r'^#include "axtrack_hip_jpeg.h"$', main, flags=re.M)
    for other in ('axtrack_hip.h', 'axtrack_hip_stage.h', 'axtrack_hip_trunk.h', 'axtrack_hip_repack.h', 'axtrack_hip_tiff.h'):
        text = open(os.path.join(ROOT, 'include', other)).read()
        assert not any(re.search(rf'\b{n}\s*\(', text) for n in NEW_NAMES), other
    lib = _lib.load()
    assert lib.axt_abi_version() == 1
    for n in NEW_NAMES:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    res, args = _lib.SIGNATURES['axt_jpeg_encode_rgb8']
    assert res is _lib.c_int and len(args) == 13 and [i for i, a in enumerate(args) if a is _lib.c_int64] == [4, 7, 11]
    assert _lib.SIGNATURES['axt_jpeg_scan_bound'] == (_lib.c_int64, [_lib.c_int] * 2)
    assert _lib.SIGNATURES['axt_jpeg_scratch_bytes'] == (_lib.c_int64, [_lib.c_int] * 3)
    mk = open(os.path.join(ROOT, 'axtrack_amd', 'csrc', 'Makefile')).read()
    assert 'jpeg.hip' in mk and 'jpeg_encode.h' in mk and 'axtrack_hip_jpeg.h' in mk


def test_size_queries():
    lib = _lib.load()
    for H, W in ((1, 1), (8, 8), (7, 9), (512, 512), (2920, 5764), (65535, 65535)):
        bh, bw = -(-H // 8), -(-W // 8)
        raw = -(-bw * 4978 // 8)                            # 20 + 22 + 22 bits of DC, 3 x 63 x 26 of AC per MCU
        assert lib.axt_jpeg_scan_bound(H, W) == bh * 2 * raw + 2 * (bh - 1)
        assert hotpath.jpeg_scan_bound(H, W) == lib.axt_jpeg_scan_bound(H, W)
    assert lib.axt_jpeg_scratch_bytes(0, 8, 8) == 0
    one = lib.axt_jpeg_scratch_bytes(1, 512, 512)
    assert 4096 * 1000 <= one <= 4096 * 1100               # 384 + 6 + 622 bytes per MCU and the rows' counters and lib.axt_jpeg_scratch_bytes(7, 512, 512) <= 7 * one
    for name in jc.case_names():                            # the bound holds for every case, the noise included
        _, rgb, _, _ = next(c for c in jc.cases() if c[0] == name)
        assert all(len(s) <= lib.axt_jpeg_scan_bound(rgb.shape[1], rgb.shape[2]) for s, _ in jc.reference(name))
    for bad in ((0, 8), (8, 0), (65536, 8), (8, 65536), (-1, 8)):
        assert lib.axt_jpeg_scan_bound(*bad) == AXT_EINVAL and b'axt_jpeg_scan_bound' in lib.axt_last_error()
        assert lib.axt_jpeg_scratch_bytes(1, *bad) == AXT_EINVAL and b'axt_jpeg_scratch_bytes' in lib.axt_last_error()
    assert lib.axt_jpeg_scratch_bytes(-1, 8, 8) == AXT_EINVAL


def test_entry_point_refuses_bad_arguments_before_any_device_call():
    lib = _lib.load()
    buf = np.zeros(1 << 16, np.int64)
    p = buf.ctypes.data                                     # (never dereferenced: the checks come first)
    assert p % 16 == 0

    def call(d_rgb=p, n_frames=1, H=16, W=24, stride=3 * 16 * 24, quality=90, d_scan=p, capacity=64, d_bytes=p, d_status=p,
             d_scratch=p, scratch=None):
        scratch = lib.axt_jpeg_scratch_bytes(max(n_frames, 0), 16, 24) if scratch is None else scratch
        return lib.axt_jpeg_encode_rgb8(d_rgb, n_frames, H, W, stride, quality, d_scan, capacity, d_bytes, d_status, d_scratch,
                                        scratch, None)

    for kw in (dict(d_rgb=None), dict(d_scan=None), dict(d_bytes=None), dict(d_status=None), dict(d_scratch=None)):
        assert call(**kw) == AXT_EINVAL
        assert lib.axt_last_error() == b'axt_jpeg_encode_rgb8: null argument'
    for kw in (dict(n_frames=-1), dict(stride=-1), dict(capacity=-1), dict(scratch=-1)):
        assert call(**kw) == AXT_EINVAL
        assert b'axt_jpeg_encode_rgb8: negative size' in lib.axt_last_error()
    for kw in (dict(H=0), dict(W=0), dict(H=65536, stride=1 << 40), dict(W=65536, stride=1 << 40), dict(H=-4)):
        assert call(**kw) == AXT_EINVAL
        assert b'axt_jpeg_encode_rgb8: H' in lib.axt_last_error() and b'outside 1..65535' in lib.axt_last_error()
    for q in (0, 101, -1):
        assert call(quality=q) == AXT_EINVAL
        assert b'axt_jpeg_encode_rgb8: quality' in lib.axt_last_error()
    assert call(stride=3 * 16 * 24 - 1) == AXT_EINVAL
    assert b'axt_jpeg_encode_rgb8: frame_stride' in lib.axt_last_error()
    assert call(scratch=lib.axt_jpeg_scratch_bytes(1, 16, 24) - 1) == AXT_EINVAL
    assert b'axt_jpeg_encode_rgb8: scratch' in lib.axt_last_error()
    assert call(d_scratch=p + 4) == AXT_EINVAL
    assert b'axt_jpeg_encode_rgb8: d_scratch is not 16-byte aligned' in lib.axt_last_error()
    # 2^31 blocks: 32768 frames of 2048 x 2048 pixels (65536 blocks each); one fewer frame passes this check and stops
    # at the next, the scratch
    assert call(n_frames=32768, H=2048, W=2048, stride=3 << 22, scratch=1 << 62) == AXT_EINVAL
    assert b'axt_jpeg_encode_rgb8: 2147483648 blocks' in lib.axt_last_error()
    assert call(n_frames=32767, H=2048, W=2048, stride=3 << 22, scratch=1 << 20) == AXT_EINVAL
    assert b'axt_jpeg_encode_rgb8: scratch' in lib.axt_last_error()
    assert call(n_frames=0) == 0                            # nothing to do, nothing launched
    assert not buf.any()


def test_python_surface():
    assert axtrack_amd.jpeg_encode is jpeg.jpeg_encode and axtrack_amd.write_mjpeg_avi is jpeg.write_mjpeg_avi
    assert 'jpeg_encode' in axtrack_amd.__all__ and 'write_mjpeg_avi' in axtrack_amd.__all__
    assert list(inspect.signature(jpeg.write_mjpeg_avi).parameters) == ['path', 'jpegs', 'H', 'W', 'fps']
    sig = inspect.signature(axtrack_amd.render_inference).parameters
    assert sig['video'].default is False and sig['quality'].default == 90 and sig['animated'].default is False
    assert all(callable(getattr(hotpath, n)) for n in ('jpeg_scan_bound', 'jpeg_scratch_bytes', 'jpeg_encode_launch'))
    with pytest.raises(TypeError):
        jpeg.jpeg_encode(np.zeros((8, 8, 3), np.uint8))
    import torch
    with pytest.raises(ValueError, match='GPU'):
        jpeg.jpeg_encode(torch.zeros((8, 8, 3), dtype=torch.uint8))


def test_video_and_animated_together_raise_before_rendering():
    class Untouchable:                                      # any attribute access would be the start of rendering
        def __getattr__(self, name):
            raise AssertionError(f'render_inference touched the detections ({name}) before refusing')

        def __len__(self):
            raise AssertionError('render_inference touched the detections before refusing')
    with pytest.raises(ValueError, match='video=True.*animated=True'):
        axtrack_amd.render_inference(Untouchable(), dest_dir='/nonexistent/never/made', video=True, animated=True)
    assert not os.path.exists('/nonexistent')
    for q in (0, 101):
        with pytest.raises(ValueError, match='quality'):
            axtrack_amd.render_inference(Untouchable(), dest_dir='/nonexistent/never/made', video=True, quality=q)
    with pytest.raises(NotImplementedError):                # as before
        axtrack_amd.visualize_inference(None)


def test_package_imports_no_pillow():
    pkg = os.path.join(ROOT, 'axtrack_amd')
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith('.py'):
            text = open(os.path.join(pkg, fn)).read()
            assert not re.search(r'^\s*(import|from)\s+(oracle|PIL)\b', text, re.M), fn
    assert not re.search(r'\bPIL\b|\bjpeg_reference\b|\bjpeg_cases\b', open(os.path.join(pkg, 'jpeg.py')).read())
    text = open(os.path.join(ROOT, 'tests', 'jpeg_reference.py')).read()
    assert not re.search(r'^\s*(import|from)\s+axtrack_amd\b', text, re.M)        # the reference stands on its own
