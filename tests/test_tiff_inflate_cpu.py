"""Deflate TIFF strips (csrc/tiff_inflate.h, csrc/tiff_inflate.hip) as far as they go without a GPU: the
reference inflater of tests/tiff_inflate_cases.py against zlib over the whole battery, the inflate core of the kernel as a
host program under AddressSanitizer and UBSan, the entry point's refusals, where it is declared and bound, and what
SegmentPacker packs for a Deflate file on either route."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from axtrack_amd import _lib, hotpath, tiff

import tiff_cases as tc
import tiff_inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXT_EINVAL = -22


@pytest.fixture(scope='module')
def cases():
    return ic.inflate_cases()


# ------------------------------------------------------------------------------------------------ the reference against zlib
def test_reference_inflater_agrees_with_zlib_on_every_case(cases):
    """Status 0 exactly where zlib.decompress succeeds AND returns rows * W * 2 bytes, and then the same bytes; a non-zero
    status where zlib raises or returns another length. No case is exempt."""
    for c in cases:
        n = c.rows * c.W * 2
        status, got = ic.ref_inflate(c.src, n)
        assert status == c.status, c.name
        try:
            want = zlib.decompress(c.src)
        except zlib.error:
            want = None
        if want is not None and len(want) == n:
            assert status == ic.OK and got == want, c.name
        else:
            assert status != ic.OK and got is None, c.name


def test_battery_holds_what_it_claims(cases):
    by_name = {c.name: c for c in cases}
    # the first block of zlib's own streams: stored, fixed, dynamic
    first = {n: ic.first_block_type(by_name[f'{n}_sparse_7x77'].src) for n in ('stored', 'fixed', 'huffman_only', 'rle')}
    assert first == {'stored': 0, 'fixed': 1, 'huffman_only': 2, 'rle': 2}
    assert ic.first_block_type(by_name['default_sparse_256x80'].src) == 2 and ic.first_block_type(by_name['rle_sparse_256x80'].src) == 2
    assert by_name['wbits9_sparse_7x77'].src[0] == 0x18                                # a 512-byte window in the header
    assert by_name['full_flush_sparse_256x80'].src.count(b'\x00\x00\xff\xff') >= 4     # empty stored blocks in mid-stream
    assert {c.status for c in cases} == {0, 1, 2, 3, 5}
    assert sum(c.status != 0 for c in cases) >= 12 and sum(c.status == 0 for c in cases) >= 30
    assert {(c.rows, c.W) for c in cases} >= {(7, 77), (16, 80), (256, 80), (1, 1), (1, 2), (1, 3), (0, 80)}
    assert {(c.predictor, c.big_endian) for c in cases if c.status == 0} == {(1, False), (1, True), (2, False), (2, True)}
    for name in ('hand_window_32768_and_wrap', 'hand_matches_across_the_wrap', 'hand_all_zero_distance_set', 'hand_one_code_distance_set',
                 'hand_single_code_end_of_block_set', 'hand_stored_0_and_65535', 'hand_empty_final_fixed_block',
                 'hand_empty_final_stored_block', 'trailing_bytes_after_the_checksum'):
        assert by_name[name].status == 0
    assert by_name['wrong_adler'].status == 5 and by_name['literal_after_completion'].status == 3


def test_adler_and_canonical_codes_of_the_reference():
    data = bytes(tc.noise((64, 80), 5).tobytes())
    assert ic.adler32(data) == zlib.adler32(data) and ic.adler32(b'') == 1
    codes = ic.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4])                                # the example of RFC 1951 3.2.2
    assert [format(codes[s][1], f'0{codes[s][0]}b') for s in range(8)] == ['010', '011', '100', '101', '110', '00', '1110', '1111']


# ------------------------------------------------------------------------------------------------ the shared core, on the host
def test_inflate_core_on_the_host(cases, tmp_path):
    """csrc/tiff_inflate.h -- the bit buffer, the three block types, the table building, every bounds check, the Adler-32,
    the code the kernel runs -- in a stand-alone program with its own main, built with AddressSanitizer and UBSan, on
    every case of the battery, the malformed ones included: the reference's status and samples, within
    axt_tiff_inflate_max_steps steps, the input in a heap block of its exact size, the output between guard samples."""
    case_file, exe = tmp_path / 'cases.bin', tmp_path / 'tiff_inflate_host'
    ic.write_case_file(str(case_file), cases)
    subprocess.check_call(['/opt/rocm/bin/hipcc', '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g',
                           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                           f'-I{os.path.join(ROOT, "axtrack_amd", "csrc")}', os.path.join(ROOT, 'tests', 'tiff_inflate_host.cpp'),
                           '-o', str(exe)])
    res = subprocess.run([str(exe), str(case_file)], capture_output=True, text=True)
    print(res.stdout[-3000:], res.stderr[-3000:])
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    assert 'FAILED' not in res.stdout and 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    assert res.stdout.count(': ok\n') == len(cases)
    assert res.stdout.strip().endswith(f'{len(cases)} cases, 0 failures')


# ------------------------------------------------------------------------------------------------ the entry point
def test_entry_point_refuses_bad_arguments_before_any_device_call():
    lib = _lib.load()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data                                     # (never dereferenced: the checks come first)

    def call(d_src=p, src_len=8, d_segs=p, n_segs=1, W=4, predictor=1, d_out=p, out_len=4, d_status=p):
        return lib.axt_tiff_inflate_u16(d_src, src_len, d_segs, n_segs, W, predictor, 0, d_out, out_len, d_status, None)

    for kw in (dict(d_src=None), dict(d_segs=None), dict(d_out=None), dict(d_status=None)):
        assert call(**kw) == AXT_EINVAL
        assert lib.axt_last_error() == b'axt_tiff_inflate_u16: null argument'
    for kw in (dict(src_len=-1), dict(n_segs=-1), dict(W=-1), dict(out_len=-1)):
        assert call(**kw) == AXT_EINVAL
        assert b'axt_tiff_inflate_u16: negative size' in lib.axt_last_error()
    for pr in (0, 3, -1):
        assert call(predictor=pr) == AXT_EINVAL
        assert b'axt_tiff_inflate_u16: predictor' in lib.axt_last_error()
    assert call(n_segs=0) == 0                              # nothing to do, nothing launched
    assert not buf.any()


def test_where_the_entry_point_is_declared_and_bound():
    """Exported and bound, declared under csrc/, and not (yet) in the public ABI: neither under include/ nor in SIGNATURES,
    whose contract table (tests/contract_cases.py) lists every prototype of include/."""
    lib = _lib.load()
    assert hasattr(lib, 'axt_tiff_inflate_u16')
    assert 'axt_tiff_inflate_u16' in _lib.INTERNAL_SIGNATURES and 'axt_tiff_inflate_u16' not in _lib.SIGNATURES
    assert not set(_lib.INTERNAL_SIGNATURES) & set(_lib.SIGNATURES)
    res, args = _lib.INTERNAL_SIGNATURES['axt_tiff_inflate_u16']
    assert res is _lib.c_int and len(args) == 11 and args[1] is _lib.c_int64 and args[8] is _lib.c_int64
    assert lib.axt_tiff_inflate_u16.argtypes == args and lib.axt_tiff_inflate_u16.restype is res
    for name in os.listdir(os.path.join(ROOT, 'include')):
        assert 'axt_tiff_inflate_u16' not in open(os.path.join(ROOT, 'include', name)).read(), name
    header = open(os.path.join(ROOT, 'axtrack_amd', 'csrc', 'axt_tiff_inflate.h')).read()
    assert set(re.findall(r'^int (axt_\w+)\s*\(', header, re.M)) == {'axt_tiff_inflate_u16'}
    for n in range(6):
        assert re.search(rf'^ \*   {n}  ', header, re.M), f'status {n} is not in the table'
    mk = open(os.path.join(ROOT, 'axtrack_amd', 'csrc', 'Makefile')).read()
    assert 'tiff_inflate.hip' in mk and 'tiff_inflate.h' in mk and 'tiff_rows.h' in mk and 'axt_tiff_inflate.h' in mk
    assert 5 in hotpath.TIFF_STATUS_TEXT and 'checksum' in hotpath.TIFF_STATUS_TEXT[5]
    # the kernel and tiff.hip share one row pass
    csrc = os.path.join(ROOT, 'axtrack_amd', 'csrc')
    stated = [n for n in sorted(os.listdir(csrc)) if n.endswith(('.hip', '.h')) and 'void tiff_finish_rows(' in open(os.path.join(csrc, n)).read()]
    assert stated == ['tiff_rows.h']


# ------------------------------------------------------------------------------------------------ the packer
@pytest.mark.parametrize('compression', [tc.ADOBE_DEFLATE, tc.DEFLATE])
def test_packer_ships_deflate_strips_compressed(compression, tmp_path):
    stack = tc.sparse((3, 50, 77), 0.1, 91)
    path = str(tmp_path / 't.tif')
    layout = tc.write_tiff(path, stack, compression=compression, rows_per_strip=16, odd_offsets=True, predictor=2)
    data = open(path, 'rb').read()
    info = tiff.tiff_info(path)
    strips = [data[o:o + n] for offs, cnts in layout for o, n in zip(offs, cnts)]
    for packer in (tiff.SegmentPacker(info, inflate='device'),):
        view, host, segs, total = packer.pack(0, 3, pinned=False)
        assert packer.device_compression == compression
        assert total == int(info.src_bytes.sum()) == sum(len(s) for s in strips)
        assert bytes(view) == b''.join(strips)
        assert segs['src_bytes'].tolist() == info.src_bytes.tolist()
        assert segs['src_offset'].tolist() == np.concatenate([[0], np.cumsum(info.src_bytes)[:-1]]).tolist()
        assert segs['rows'].tolist() == [16, 16, 16, 2] * 3
        assert segs['dst_offset'].tolist() == [(t * 50 + r) * 77 for t in range(3) for r in (0, 16, 32, 48)]
    view, _, segs, total = tiff.SegmentPacker(info, inflate='device').pack(1, 2, pinned=False)      # a frame range
    assert bytes(view) == b''.join(strips[4:8]) and segs['dst_offset'].tolist() == [r * 77 for r in (0, 16, 32, 48)]
    packer = tiff.SegmentPacker(info, inflate='host')
    view, host, segs, total = packer.pack(0, 3, pinned=False)
    assert packer.device_compression == tiff.COMPRESSION_NONE
    assert total == stack.size * 2 and bytes(view) == b''.join(zlib.decompress(s) for s in strips)
    assert segs['src_bytes'].tolist() == [r * 77 * 2 for r in (16, 16, 16, 2)] * 3
    with pytest.raises(ValueError, match='inflate'):
        tiff.SegmentPacker(info, inflate='gpu')
    # the default: inflate_on_device decides per pack, by the measured threshold; 12 strips are the host's
    assert not tiff.inflate_on_device(tiff.INFLATE_ON_DEVICE_FROM - 1) and tiff.inflate_on_device(tiff.INFLATE_ON_DEVICE_FROM)
    assert tiff.INFLATE_ON_DEVICE_FROM > 12 and tiff.inflate_on_device(4096)
    packer = tiff.SegmentPacker(info)
    assert packer.pack(0, 3, pinned=False)[3] == stack.size * 2 and packer.device_compression == tiff.COMPRESSION_NONE


def test_packer_asks_inflate_on_device_for_every_pack(tmp_path, monkeypatch):
    stack = tc.sparse((2, 20, 33), 0.2, 92)
    path = str(tmp_path / 't.tif')
    tc.write_tiff(path, stack, compression=tc.ADOBE_DEFLATE, rows_per_strip=5)
    info = tiff.tiff_info(path)
    asked = []
    monkeypatch.setattr(tiff, 'inflate_on_device', lambda n: asked.append(n) or n > 4)
    packer = tiff.SegmentPacker(info)
    _, _, _, total = packer.pack(0, 2, pinned=False)        # 8 strips: the device
    assert packer.device_compression == tc.ADOBE_DEFLATE and total == int(info.src_bytes.sum())
    _, _, _, total = packer.pack(1, 2, pinned=False)        # 4 strips: the host
    assert packer.device_compression == tiff.COMPRESSION_NONE and total == 20 * 33 * 2
    assert asked == [8, 4]
    tc.write_tiff(path, stack, compression=tc.LZW, rows_per_strip=5)                # other codecs never ask
    packer = tiff.SegmentPacker(tiff.tiff_info(path))
    packer.pack(0, 2, pinned=False)
    assert asked == [8, 4] and packer.device_compression == tc.LZW
