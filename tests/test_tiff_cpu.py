"""The native TIFF reader (axtrack_amd/tiff.py, csrc/tiff_decode.h) as far as it goes without a GPU: the
container parser on every variant the test writer makes and on files from Pillow / libtiff, every refusal, the reference
decoder of tests/tiff_cases.py against the arrays the golden files were made from, the decoder core of the kernels as a
host program under AddressSanitizer and UBSan, and the bookkeeping of the new header."""
import glob
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import axtrack_amd
from axtrack_amd import _lib, hotpath, tiff
from axtrack_amd.tiff import TiffError, TiffUnsupported, tiff_info

import tiff_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXT_EINVAL = -22
GOLDEN_FILES = sorted(os.path.basename(f) for f in glob.glob(os.path.join(tc.GOLDEN, '*.tif')))


@pytest.fixture(scope='module')
def stack():
    return tc.sparse((3, 50, 77), 0.1, 1)


# ------------------------------------------------------------------------------------------------ the parser, our writer
VARIANTS = [dict(byteorder=bo, bigtiff=big, rows_per_strip=rps, compression=comp, predictor=pred, odd_offsets=odd)
            for bo in '<>' for big in (False, True) for rps, comp, pred, odd in (
                (None, tc.NONE, 1, False), (16, tc.NONE, 2, True), (1, tc.LZW, 1, True), (16, tc.LZW, 2, False),
                (16, tc.PACKBITS, 1, True), (7, tc.ADOBE_DEFLATE, 2, False), (50, tc.DEFLATE, 1, True))]


@pytest.mark.parametrize('kw', VARIANTS, ids=lambda kw: '-'.join(str(v) for v in kw.values()))
def test_parser_on_every_writer_variant(kw, stack, tmp_path):
    path = str(tmp_path / 't.tif')
    layout = tc.write_tiff(path, stack, **kw)
    info = tiff_info(path)
    T, H, W = stack.shape
    assert info.shape == (T, H, W) and info.byteorder == kw['byteorder'] and info.bigtiff == kw['bigtiff']
    assert info.compression == kw['compression'] and info.predictor == kw['predictor'] and not info.imagej
    rps = kw['rows_per_strip'] or H
    n = -(-H // rps)
    assert info.n_segments == T * n
    assert [a.dtype for a in (info.src_offset, info.src_bytes, info.frame, info.row0, info.rows)] == [
        np.int64, np.int64, np.int32, np.int32, np.int32]
    assert info.src_offset.tolist() == [o for offs, _ in layout for o in offs]
    assert info.src_bytes.tolist() == [c for _, cnts in layout for c in cnts]
    assert info.frame.tolist() == [t for t in range(T) for _ in range(n)]
    assert info.row0.tolist() == [r for _ in range(T) for r in range(0, H, rps)]
    assert info.rows.tolist() == [min(rps, H - r) for _ in range(T) for r in range(0, H, rps)]
    if kw['odd_offsets']:
        assert (info.src_offset % 2 == 1).all()
    assert np.array_equal(tc.ref_read(path, info), stack)


def test_parser_details(stack, tmp_path):
    path = str(tmp_path / 't.tif')
    tc.write_tiff(path, stack, omit_rows_per_strip=True, compression=tc.LZW)          # absent RowsPerStrip: one strip
    info = tiff_info(path)
    assert info.n_segments == 3 and info.rows.tolist() == [50] * 3
    tc.write_tiff(path, stack, reduced_copies=True, rows_per_strip=16)                 # NewSubfileType bit 0: skipped
    info = tiff_info(path)
    assert info.shape == stack.shape and info.n_segments == 12
    tc.write_tiff(path, stack, tags_override={339: None, 262: (3, [0])})               # SampleFormat absent, Photometric 0
    assert np.array_equal(tc.ref_read(path, tiff_info(path)), stack)                   # (not inverted, as tifffile returns it)
    for bo in '<>':
        for big in (False, True):
            layout = tc.write_tiff(path, stack, imagej=True, byteorder=bo, bigtiff=big, odd_offsets=True)
            info = tiff_info(path)
            first = layout[0][0][0]
            assert info.imagej and info.shape == stack.shape and info.n_segments == 3
            assert info.src_offset.tolist() == [first + k * 50 * 77 * 2 for k in range(3)]
            assert info.src_bytes.tolist() == [50 * 77 * 2] * 3 and info.rows.tolist() == [50] * 3
            assert np.array_equal(tc.ref_read(path, info), stack)


@pytest.mark.parametrize('fname', GOLDEN_FILES)
def test_parser_and_reference_decoder_on_golden_files(fname):
    """Files from Pillow / libtiff 4.7.1 (tests/golden/make_golden_tiff.py): the parser's table, and the reference decoder
    of tiff_cases.py -- which every GPU comparison leans on -- against the arrays the files were made from."""
    src = np.load(os.path.join(tc.GOLDEN, fname[:fname.index('_', fname.index('x'))] + '.npy'))
    info = tiff_info(os.path.join(tc.GOLDEN, fname))
    assert info.shape == src.shape and info.byteorder == '<' and not info.bigtiff and not info.imagej
    want = {'raw': 1, 'tiff_lzw': 5, 'packbits': 32773, 'tiff_adobe_deflate': 8}
    assert info.compression == next(v for k, v in want.items() if f'_{k}' in fname)
    assert info.predictor == (2 if 'pred2' in fname else 1)
    T, H, W = src.shape
    if fname.startswith('sparse') and info.compression != 1:
        assert info.n_segments == 12 and info.rows.tolist() == [16, 16, 16, 2] * 3 and info.row0.tolist() == [0, 16, 32, 48] * 3
    else:
        assert info.n_segments == 3 and info.rows.tolist() == [H] * 3
    size = os.path.getsize(os.path.join(tc.GOLDEN, fname))
    assert size < 65536 and (info.src_offset + info.src_bytes <= size).all()
    assert np.array_equal(tc.ref_read(os.path.join(tc.GOLDEN, fname), info), src)


def test_golden_set_is_complete():
    for name in ('noise_64x80', 'sparse_50x77'):
        assert os.path.exists(os.path.join(tc.GOLDEN, name + '.npy'))
        for comp in ('raw', 'tiff_lzw', 'packbits', 'tiff_adobe_deflate', 'tiff_lzw_pred2', 'tiff_adobe_deflate_pred2'):
            assert f'{name}_{comp}.tif' in GOLDEN_FILES


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('override, words', [
    ({322: (3, [16])}, 'TileWidth'), ({324: (4, [8])}, 'TileOffsets'),
    ({258: (3, [8])}, 'BitsPerSample 8'), ({258: (3, [32])}, 'BitsPerSample 32'),
    ({339: (3, [3])}, 'SampleFormat 3'), ({339: (3, [2])}, 'SampleFormat 2'),
    ({277: (3, [3]), 258: (3, [16, 16, 16]), 262: (3, [2])}, 'SamplesPerPixel 3'),
    ({262: (3, [3])}, 'PhotometricInterpretation 3'),
    ({259: (3, [7])}, 'Compression 7'), ({259: (3, [50000])}, 'Compression 50000'),
    ({317: (3, [3])}, 'Predictor 3'),
], ids=lambda v: v if isinstance(v, str) else '')
def test_unsupported_features_are_named(override, words, stack, tmp_path):
    path = str(tmp_path / 't.tif')
    tc.write_tiff(path, stack, tags_override=override)
    with pytest.raises(TiffUnsupported, match=words):
        tiff_info(path)
    assert issubclass(TiffUnsupported, ValueError) and issubclass(TiffError, ValueError)


def test_old_style_lzw_and_mixed_pages_are_refused(stack, tmp_path):
    path = str(tmp_path / 't.tif')
    layout = tc.write_tiff(path, stack, compression=tc.LZW)
    data = bytearray(open(path, 'rb').read())
    o = layout[1][0][0]
    data[o:o + 2] = b'\x00\x01'                                 # libtiff's test: first byte 0, low bit of the second set
    open(path, 'wb').write(data)
    with pytest.raises(TiffUnsupported, match=f'LSB-first.*frame 1 at offset {o}'):
        tiff_info(path)
    # a page of another width behind the first: the IFD chain of one file spliced onto another is more than this needs --
    # ImageWidth of the second IFD is patched in place
    layout = tc.write_tiff(path, stack[:2], compression=tc.LZW)
    data = bytearray(open(path, 'rb').read())
    hits = [m.start() for m in re.finditer(re.escape(struct.pack('<HHII', 256, 4, 1, 77)), bytes(data))]
    assert len(hits) == 2
    data[hits[1] + 8:hits[1] + 12] = struct.pack('<I', 78)
    open(path, 'wb').write(data)
    with pytest.raises(TiffUnsupported, match='page 1 .* is 78 x 50'):
        tiff_info(path)


def test_truncated_and_inconsistent_files_name_the_offset(stack, tmp_path):
    path = str(tmp_path / 't.tif')
    tc.write_tiff(path, stack, rows_per_strip=16, compression=tc.PACKBITS)
    data = open(path, 'rb').read()
    size = len(data)
    first_ifd = struct.unpack_from('<I', data, 4)[0]

    def parse(blob):
        open(path, 'wb').write(blob)
        return tiff_info(path)

    with pytest.raises(TiffError, match='offset 0'):
        parse(b'')
    with pytest.raises(TiffError, match='offset 0'):
        parse(data[:6])
    with pytest.raises(TiffError, match='byte-order mark at offset 0'):
        parse(b'XX' + data[2:])
    with pytest.raises(TiffError, match='magic number 44 at offset 2'):
        parse(data[:2] + struct.pack('<H', 44) + data[4:])
    with pytest.raises(TiffError, match=f'IFD at offset {size + 10} .* outside the file of {size} bytes'):
        parse(data[:4] + struct.pack('<I', size + 10) + data[8:])                     # an IFD offset past the end
    with pytest.raises(TiffError, match=f'outside the file of {first_ifd + 20} bytes'):
        parse(data[:first_ifd + 20])                                                  # cut inside the first IFD
    with pytest.raises(TiffError, match='loops back to offset'):
        blob = bytearray(data)
        n = struct.unpack_from('<H', data, first_ifd)[0]
        blob[first_ifd + 2 + 12 * n:first_ifd + 6 + 12 * n] = struct.pack('<I', first_ifd)
        parse(bytes(blob))
    tc.write_tiff(path, stack, rows_per_strip=16, tags_override={278: (4, [10])})     # 4 strips listed, 5 needed
    with pytest.raises(TiffError, match='needs 5 strips'):
        tiff_info(path)
    tc.write_tiff(path, stack, tags_override={279: (4, [50 * 77 * 2 - 2])})           # an uncompressed strip that is short
    with pytest.raises(TiffError, match='uncompressed strip of frame 0, row 0 at offset'):
        tiff_info(path)


def test_strip_past_the_end_of_the_file(stack, tmp_path):
    """The table is checked against the file size before anything is read: the last strip's byte count is patched up."""
    path = str(tmp_path / 't.tif')
    layout = tc.write_tiff(path, stack, compression=tc.LZW, bigtiff=True, byteorder='>')
    size = os.path.getsize(path)
    o, c = layout[2][0][0], layout[2][1][0]
    tc.write_tiff(path, stack, compression=tc.LZW, bigtiff=True, byteorder='>')
    data = bytearray(open(path, 'rb').read())
    hit = bytes(data).rindex(struct.pack('>HHQQ', 279, 16, 1, c))
    data[hit + 12:hit + 20] = struct.pack('>Q', size - o + 1)
    open(path, 'wb').write(data)
    with pytest.raises(TiffError, match=f'frame 2, row 0 at offset {o} .{size - o + 1} bytes. lies outside the file of {size} bytes'):
        tiff_info(path)


# ------------------------------------------------------------------------------------------------ the decoder core, on the host
def test_decoder_core_on_the_host(tmp_path):
    """csrc/tiff_decode.h -- the bit reader, the width schedule, Clear / EOI, the table update, the PackBits parser and every
    bounds check, the code the kernels run -- in a stand-alone program with its own main, built with AddressSanitizer and
    UBSan, on every case of tiff_cases.decode_cases(), the malformed ones included, each in heap blocks of its exact size."""
    cases = tc.decode_cases()
    assert {c.status for c in cases} == {0, 1, 2, 3} and sum(c.status != 0 for c in cases) >= 8
    case_file, exe = tmp_path / 'cases.bin', tmp_path / 'tiff_decode_host'
    tc.write_case_file(str(case_file), cases)
    subprocess.check_call(['/opt/rocm/bin/hipcc', '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g',
                           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                           f'-I{os.path.join(ROOT, "axtrack_amd", "csrc")}', os.path.join(ROOT, 'tests', 'tiff_decode_host.cpp'),
                           '-o', str(exe)])
    res = subprocess.run([str(exe), str(case_file)], capture_output=True, text=True)
    print(res.stdout[-3000:], res.stderr[-3000:])
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    assert 'FAILED' not in res.stdout and 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    assert res.stdout.strip().endswith(f'{len(cases)} cases, {len(tc.DESCRIPTOR_CASES)} descriptors, 0 failures')


def test_lzw_case_crosses_every_width_and_a_table_reset():
    """What the noise case is for: more than 4094 codes, all four widths, a Clear in mid-stream."""
    _, codes = tc.lzw_encode(tc.noise((64, 80), 11).tobytes(), return_codes=True)
    assert len(codes) > 4094 and {w for _, w in codes} == {9, 10, 11, 12}
    assert sum(c == tc.CLEAR for c, _ in codes) >= 3
    first_clear = [i for i, (c, _) in enumerate(codes) if c == tc.CLEAR][1]
    assert first_clear == 1 + (4094 - 258)                                  # the specification's Clear at 4094 entries
    # the sparse case: long strings and self-referencing codes
    data = tc.sparse((256, 160), 0.02, 12).tobytes()
    _, codes = tc.lzw_encode(data, return_codes=True)
    assert len(data) > 65536 and len(data) / len(codes) > 20


# ------------------------------------------------------------------------------------------------ declarations
def test_new_header_declares_and_binds_the_new_name():
    header = open(os.path.join(ROOT, 'include', 'axtrack_hip_tiff.h')).read()
    assert set(re.findall(r'^int (axt_\w+)\s*\(', header, re.M)) == {'axt_tiff_decode_u16'}
    main = open(os.path.join(ROOT, 'include', 'axtrack_hip.h')).read()
    assert re.search(r'^#include "axtrack_hip_tiff.h"$', main, flags=re.M)
    for other in ('axtrack_hip.h', 'axtrack_hip_stage.h', 'axtrack_hip_trunk.h', 'axtrack_hip_repack.h'):
        assert not re.search(r'\baxt_tiff_decode_u16\s*\(', open(os.path.join(ROOT, 'include', other)).read())
    lib = _lib.load()
    assert lib.axt_abi_version() == 1
    assert 'axt_tiff_decode_u16' in _lib.SIGNATURES and hasattr(lib, 'axt_tiff_decode_u16')
    res, args = _lib.SIGNATURES['axt_tiff_decode_u16']
    assert res is _lib.c_int and len(args) == 12 and args[1] is _lib.c_int64 and args[9] is _lib.c_int64
    assert tiff.TIFF_SEGMENT_DTYPE.itemsize == 32
    assert [tiff.TIFF_SEGMENT_DTYPE.fields[n][1] for n in ('src_offset', 'src_bytes', 'dst_offset', 'rows', 'reserved')] == [0, 8, 16, 24, 28]
    mk = open(os.path.join(ROOT, 'axtrack_amd', 'csrc', 'Makefile')).read()
    assert 'tiff.hip' in mk and 'tiff_decode.h' in mk and 'axtrack_hip_tiff.h' in mk


def test_entry_point_refuses_bad_arguments_before_any_device_call():
    lib = _lib.load()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data                                     # (never dereferenced: the checks come first)

    def call(d_src=p, src_len=8, d_segs=p, n_segs=1, W=4, compression=5, predictor=1, d_out=p, out_len=4, d_status=p):
        return lib.axt_tiff_decode_u16(d_src, src_len, d_segs, n_segs, W, compression, predictor, 0, d_out, out_len, d_status, None)

    for kw in (dict(d_src=None), dict(d_segs=None), dict(d_out=None), dict(d_status=None)):
        assert call(**kw) == AXT_EINVAL
        assert lib.axt_last_error() == b'axt_tiff_decode_u16: null argument'
    for kw in (dict(src_len=-1), dict(n_segs=-1), dict(W=-1), dict(out_len=-1)):
        assert call(**kw) == AXT_EINVAL
        assert b'axt_tiff_decode_u16: negative size' in lib.axt_last_error()
    for c in (0, 2, 7, 8, 32946, -5):                       # (Deflate is inflated on the host: the device never sees 8)
        assert call(compression=c) == AXT_EINVAL
        assert b'axt_tiff_decode_u16: compression' in lib.axt_last_error()
    for pr in (0, 3, -1):
        assert call(predictor=pr) == AXT_EINVAL
        assert b'axt_tiff_decode_u16: predictor' in lib.axt_last_error()
    assert call(n_segs=0) == 0                              # nothing to do, nothing launched
    assert not buf.any()


def test_python_surface():
    assert axtrack_amd.read_tiff is tiff.read_tiff and axtrack_amd.tiff_info is tiff_info
    assert axtrack_amd.TiffError is TiffError and axtrack_amd.TiffUnsupported is TiffUnsupported
    assert list(inspect.signature(tiff.read_tiff).parameters) == ['path', 'frames', 'device']
    assert inspect.signature(tiff.read_tiff).parameters['device'].default == 'cuda:0'
    sig = inspect.signature(axtrack_amd.Timelapse.from_tiff).parameters
    host = inspect.signature(axtrack_amd.Timelapse.from_host_u16).parameters
    assert list(sig)[1:] == list(host)[1:] and sig['chunk_frames'].default == 96
    assert all(sig[k].default == host[k].default for k in list(sig)[1:-1])
    assert callable(hotpath.tiff_decode_u16)
    assert tiff._frame_list(None, 7) == (0, 7) and tiff._frame_list(range(1, 3), 7) == (1, 3)
    assert tiff._frame_list(slice(2, None), 7) == (2, 7)
    with pytest.raises(IndexError):
        tiff._frame_list(range(5, 9), 7)
    with pytest.raises(TypeError):
        tiff._frame_list(range(0, 6, 2), 7)
    with pytest.raises(TypeError):
        tiff._frame_list([1, 2], 7)


def test_package_reads_tiff_with_its_own_code_only():
    """axtrack_amd/ imports neither the checker nor Pillow, and tifffile only behind TiffUnsupported."""
    pkg = os.path.join(ROOT, 'axtrack_amd')
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith('.py'):
            text = open(os.path.join(pkg, fn)).read()
            assert not re.search(r'^\s*(import|from)\s+(oracle|PIL)\b', text, re.M), fn
            if fn != 'tiff.py':
                assert 'tifffile import' not in text and 'import tifffile' not in text, fn
    text = open(os.path.join(pkg, 'tiff.py')).read()
    assert text.count('from tifffile import imread') == 1 and text.index('except TiffUnsupported') < text.index('from tifffile')
