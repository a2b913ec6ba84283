"""Deflate TIFF output (csrc/tiff_deflate.h, csrc/tiff_deflate.hip, tiff.write_tiff, DESIGN.md 6.8h "TIFF output") as far
as it goes without a GPU: the encoder core of the kernel as a host program under AddressSanitizer and UBSan over the whole
battery of tests/tiff_deflate_cases.py, its streams against zlib.decompress and the textbook inflater, the entry points'
refusals, where they are declared and bound, and the container -- header, IFDs, strip tables, the 4 GiB decision -- as pure
functions read back with tiff_info."""
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from axtrack_amd import _lib, tiff

import tiff_deflate_cases as dc
import tiff_inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXT_EINVAL = -22


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """The battery through the host program, twice: (cases, process result, [(status, stream, batches)], the same again)."""
    tmp = tmp_path_factory.mktemp('deflate_host')
    cases = dc.deflate_cases()
    exe = dc.build_host_program(tmp, sanitize=True)
    res, streams = dc.run_host_program(exe, cases, tmp)
    _, again = dc.run_host_program(exe, cases, tmp, 'b')
    return cases, res, streams, again


# ------------------------------------------------------------------------------------------------ the shared core, on the host
def test_deflate_core_on_the_host(host):
    """csrc/tiff_deflate.h -- the parse, the three block types, the length-limited code sets, the bit emission, the
    Adler-32: the code the kernel runs -- in a stand-alone program with its own main, built with AddressSanitizer and
    UBSan: every strip in a heap block of its exact size, every slot between guard bytes, every case encoded twice in one
    process with the work area filled differently (identical streams), and once into a slot one byte too small (status 3,
    guards intact)."""
    cases, res, streams, _ = host
    print(res.stdout[-4000:], res.stderr[-3000:])
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    assert 'FAILED' not in res.stdout and 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr
    assert res.stdout.count(': ok\n') == len(cases)
    assert res.stdout.strip().endswith(f'{len(cases)} cases, 0 failures')
    assert all(status == 0 for status, _, _ in streams)


def test_every_stream_inflates_to_the_strip_exactly(host):
    cases, _, streams, _ = host
    for c, (status, stream, batches) in zip(cases, streams):
        raw = dc.stored_bytes(c.a, c.predictor)
        assert zlib.decompress(stream) == raw, c.name
        assert stream[:2] == b'\x78\x01' and (stream[0] * 256 + stream[1]) % 31 == 0, c.name
        assert len(stream) <= dc.bound(len(raw)), c.name
        assert batches <= len(raw) // 64 + 1, c.name
        st, got = ic.ref_inflate(stream, len(raw))                        # the textbook inflater, with this project's statuses
        assert st == ic.OK and got == raw, c.name


def test_a_second_run_gives_identical_bytes(host):
    _, _, streams, again = host
    assert [s for _, s, _ in streams] == [s for _, s, _ in again]


def test_block_types(host):
    """Noise comes out stored (first block type 0; more than 65535 bytes: two stored pieces and nothing else), the Fibonacci
    and the all-values strips contain a dynamic block -- whose lengths the walk has checked against 15 and 7 bits --, and
    the strip that fills the token buffer several times has blocks of more than one type."""
    cases, _, streams, _ = host
    by_name = {c.name: s for c, (_, s, _) in zip(cases, streams)}
    for name in ('noise_16x80_p1', 'noise_16x80_p2', 'noise_66x512_p1'):
        assert ic.first_block_type(by_name[name]) == 0, name
    assert dc.block_types(by_name['noise_66x512_p1']) == [0, 0]
    assert len(by_name['noise_66x512_p1']) == dc.bound(66 * 512 * 2) and len(by_name['noise_16x80_p1']) == dc.bound(2560)
    for name in ('fibonacci_p1', 'all_values_p1'):
        assert 2 in dc.block_types(by_name[name]), name
    for name in ('half_noise_half_zeros_40x512_p1', 'half_noise_half_zeros_40x512_p2'):
        assert len(set(dc.block_types(by_name[name]))) > 1, name
    assert len(dc.block_types(by_name['camera_32x512_p1'])) > 1              # the token buffer filled more than once
    assert dc.block_types(zlib.compress(b'abc' * 100, 6)) == [1] and dc.block_types(zlib.compress(b'abc', 0)) == [0]


def test_the_limiting_has_to_act_on_the_fibonacci_strip(host):
    """An unrestricted Huffman code of the Fibonacci strip's byte frequencies is deeper than 15 bits, so the strip tests
    what it claims; its stream holds a dynamic block (whose lengths block_types checks against 15 and 7) and inflates."""
    import heapq
    cases, _, streams, _ = host
    k = [c.name for c in cases].index('fibonacci_p1')
    raw = dc.stored_bytes(cases[k].a)
    freq = np.bincount(np.frombuffer(raw, np.uint8), minlength=256)
    heap = [(int(f), 0) for f in freq if f]                               # (weight, depth of the subtree)
    assert sorted(f for f, _ in heap)[:17] == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597]
    heapq.heapify(heap)
    while len(heap) > 1:
        (f1, d1), (f2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (f1 + f2, max(d1, d2) + 1))
    assert heap[0][1] > 15
    assert 2 in dc.block_types(streams[k][1]) and zlib.decompress(streams[k][1]) == raw


def test_size_conditions_on_the_host_streams(host):
    """What tests/test_tiff_deflate_gpu.py asserts on the device streams (which are these, byte for byte): smaller than
    zlib's Z_HUFFMAN_ONLY stream where there are matches to find, smaller than zlib's level-1 Z_FIXED stream on the
    camera frame, where only dynamic codes get there."""
    cases, _, streams, _ = host
    by_name = {c.name: (c, s) for c, (_, s, _) in zip(cases, streams)}
    for kind in ('sparse', 'blobs', 'zeros'):
        for pr in (1, 2):
            c, s = by_name[f'{kind}_32x512_p{pr}']
            assert len(s) < len(ic.deflate(dc.stored_bytes(c.a, pr), strategy=zlib.Z_HUFFMAN_ONLY)), (kind, pr)
    for pr in (1, 2):
        c, s = by_name[f'camera_32x512_p{pr}']
        assert len(s) < len(ic.deflate(dc.stored_bytes(c.a, pr), 1, zlib.Z_FIXED)), pr


# ------------------------------------------------------------------------------------------------ the entry points
def test_entry_points_refuse_bad_arguments_before_any_device_call():
    lib = _lib.load()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data                                     # (never dereferenced: the checks come first)

    def deflate(d_in=p, in_len=8, d_segs=p, n_segs=1, W=4, predictor=1, d_slots=p, slots_len=64, d_bytes=p, d_status=p):
        return lib.axt_tiff_deflate_u16(d_in, in_len, d_segs, n_segs, W, predictor, d_slots, slots_len, d_bytes, d_status, None)

    for kw in (dict(d_in=None), dict(d_segs=None), dict(d_slots=None), dict(d_bytes=None), dict(d_status=None)):
        assert deflate(**kw) == AXT_EINVAL
        assert lib.axt_last_error() == b'axt_tiff_deflate_u16: null argument'
    for kw in (dict(in_len=-1), dict(n_segs=-1), dict(W=-1), dict(slots_len=-1)):
        assert deflate(**kw) == AXT_EINVAL
        assert b'axt_tiff_deflate_u16: negative size' in lib.axt_last_error()
    for pr in (0, 3, -1):
        assert deflate(predictor=pr) == AXT_EINVAL
        assert b'axt_tiff_deflate_u16: predictor' in lib.axt_last_error()
    assert deflate(n_segs=0) == 0                           # nothing to do, nothing launched

    def compact(d_slots=p, d_segs=p, d_bytes=p, n_segs=1, d_packed=p, packed_len=8, d_offsets=p):
        return lib.axt_tiff_compact_streams(d_slots, d_segs, d_bytes, n_segs, d_packed, packed_len, d_offsets, None)

    for kw in (dict(d_slots=None), dict(d_segs=None), dict(d_bytes=None), dict(d_packed=None), dict(d_offsets=None)):
        assert compact(**kw) == AXT_EINVAL
        assert lib.axt_last_error() == b'axt_tiff_compact_streams: null argument'
    for kw in (dict(n_segs=-1), dict(packed_len=-1)):
        assert compact(**kw) == AXT_EINVAL
        assert b'axt_tiff_compact_streams: negative size' in lib.axt_last_error()
    assert compact(n_segs=0) == 0
    assert not buf.any()
    for raw in (0, 1, 2560, 65535, 65536, 131070, 131071, 1 << 33):
        assert lib.axt_tiff_deflate_bound(raw) == dc.bound(raw) == tiff.stored_bound(raw)
    assert lib.axt_tiff_deflate_bound(-5) == dc.bound(0)


def test_where_the_entry_points_are_declared_and_bound():
    lib = _lib.load()
    names = {'axt_tiff_deflate_bound', 'axt_tiff_deflate_u16', 'axt_tiff_compact_streams'}
    for name in names:
        assert hasattr(lib, name) and name in _lib.INTERNAL_SIGNATURES and name not in _lib.SIGNATURES
        res, args = _lib.INTERNAL_SIGNATURES[name]
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
        for inc in os.listdir(os.path.join(ROOT, 'include')):
            assert name not in open(os.path.join(ROOT, 'include', inc)).read(), inc
    assert not set(_lib.INTERNAL_SIGNATURES) & set(_lib.SIGNATURES)
    assert _lib.INTERNAL_SIGNATURES['axt_tiff_deflate_bound'] == (_lib.c_int64, [_lib.c_int64])
    assert len(_lib.INTERNAL_SIGNATURES['axt_tiff_deflate_u16'][1]) == 11 and len(_lib.INTERNAL_SIGNATURES['axt_tiff_compact_streams'][1]) == 8
    header = open(os.path.join(ROOT, 'axtrack_amd', 'csrc', 'axt_tiff_deflate.h')).read()
    assert set(re.findall(r'^(?:int|int64_t) (axt_\w+)\s*\(', header, re.M)) == names
    for n in (0, 3, 4):
        assert re.search(rf'^ \*   {n}  ', header, re.M), f'status {n} is not in the table'
    assert 'REVERSED' in header
    mk = open(os.path.join(ROOT, 'axtrack_amd', 'csrc', 'Makefile')).read()
    assert 'tiff_deflate.hip' in mk and ' tiff_deflate.h' in mk and 'axt_tiff_deflate.h' in mk
    # the core is plain C++: no inline assembly, nothing that prints or traps
    for name in ('tiff_deflate.h', 'tiff_deflate.hip'):
        code = open(os.path.join(ROOT, 'axtrack_amd', 'csrc', name)).read()
        for word in ('asm', 'printf', 'assert(', '__builtin_trap', 'abort('):
            assert word not in code, (name, word)


def test_the_package_exports_the_writer():
    import axtrack_amd
    assert axtrack_amd.write_tiff is tiff.write_tiff and callable(axtrack_amd.process_timelapse)
    assert {'write_tiff', 'process_timelapse'} <= set(axtrack_amd.__all__)
    assert not tiff.deflate_on_device(tiff.DEFLATE_ON_DEVICE_FROM - 1) and tiff.deflate_on_device(tiff.DEFLATE_ON_DEVICE_FROM)
    with pytest.raises(ValueError, match='deflate'):
        tiff.write_tiff('nowhere.tif', np.zeros((1, 4, 4), np.uint16), deflate='gpu')
    with pytest.raises(TypeError, match='uint16'):
        tiff.write_tiff('nowhere.tif', np.zeros((1, 4, 4), np.float32))
    with pytest.raises(ValueError, match='rows_per_strip'):
        tiff.write_tiff('nowhere.tif', np.zeros((1, 4, 4), np.uint16), rows_per_strip=5)
    assert not os.path.exists('nowhere.tif')


# ------------------------------------------------------------------------------------------------ the container
def read_ifd_tags(buf, at, big):
    """[(tag, type, count)] of the IFD at `at`, in file order, and the offset of the next: an independent little reader."""
    if big:
        n = struct.unpack_from('<Q', buf, at)[0]
        ents = [struct.unpack_from('<HHQ', buf, at + 8 + 20 * k) for k in range(n)]
        return ents, struct.unpack_from('<Q', buf, at + 8 + 20 * n)[0]
    n = struct.unpack_from('<H', buf, at)[0]
    ents = [struct.unpack_from('<HHI', buf, at + 2 + 12 * k) for k in range(n)]
    return ents, struct.unpack_from('<I', buf, at + 2 + 12 * n)[0]


@pytest.mark.parametrize('big', [False, True], ids=['classic', 'bigtiff'])
@pytest.mark.parametrize('predictor', [1, 2])
def test_container_reads_back(big, predictor, tmp_path):
    """TiffWriter over pages of the battery's arrays, the strips deflated by zlib: tiff_info finds every strip where it
    was put, strip by strip zlib.decompress gives the pages back, the tags are in ascending order, the offsets even, the
    strips of a page contiguous, and the file is header + strips + IFDs to the byte. rows_per_strip 1, the default, H."""
    pages = [c.a for c in dc.deflate_cases() if c.a.shape == (16, 80) and c.predictor == 1]
    assert len(pages) >= 3
    H, W = 16, 80
    for rps in (1, None, 7, H):
        path = str(tmp_path / f'{rps}.tif')
        with tiff.TiffWriter(path, H, W, rps, predictor, big, b'pages of the battery') as w:
            eff, row0, rows = w.rps, w.row0, w.rows
            for a in pages:
                stored = tiff.apply_predictor(a, predictor)
                assert stored.astype('<u2').tobytes() == dc.stored_bytes(a, predictor)
                w.add_page([zlib.compress(stored[r0:r0 + r].astype('<u2').tobytes(), 1) for r0, r in zip(row0, rows)])
        assert eff == {1: 1, None: 16, 7: 7, H: H}[rps] and rows.sum() == H
        info = tiff.tiff_info(path)
        assert info.shape == (len(pages), H, W) and info.bigtiff == big and info.predictor == predictor
        assert info.compression == tiff.COMPRESSION_ADOBE_DEFLATE and info.byteorder == '<'
        assert info.n_segments == len(pages) * len(rows)
        assert info.rows.tolist() == rows.tolist() * len(pages) and info.row0.tolist() == row0.tolist() * len(pages)
        data = open(path, 'rb').read()
        for k in range(info.n_segments):
            o, n = int(info.src_offset[k]), int(info.src_bytes[k])
            t, r0, r = int(info.frame[k]), int(info.row0[k]), int(info.rows[k])
            assert zlib.decompress(data[o:o + n]) == dc.stored_bytes(pages[t][r0:r0 + r], predictor)
        per = len(rows)
        for t in range(len(pages)):                                       # a page's strips follow one another
            o, n = info.src_offset[t * per:(t + 1) * per], info.src_bytes[t * per:(t + 1) * per]
            assert (o[1:] == o[:-1] + n[:-1]).all()
        assert len(data) == (16 if big else 8) + w.strip_bytes + w.ifd_bytes and w.strip_bytes == int(info.src_bytes.sum())
        assert w.pages == len(pages)
        # the IFD chain, read independently
        assert data[:4] == (b'II\x2b\x00' if big else b'II\x2a\x00')
        at = struct.unpack_from('<Q', data, 8)[0] if big else struct.unpack_from('<I', data, 4)[0]
        seen = 0
        while at:
            assert at % 2 == 0
            ents, at_next = read_ifd_tags(data, at, big)
            tags = [e[0] for e in ents]
            want = [256, 257, 258, 259, 262] + ([270] if seen == 0 else []) + [273, 277, 278, 279] + ([317] if predictor == 2 else []) + [339]
            assert tags == want == sorted(tags)
            for tag, ftype, count in ents:
                if tag in (273, 279):
                    assert count == per and ftype == (16 if big else 4)
            at, seen = at_next, seen + 1
        assert seen == len(pages)


def test_default_strips_and_the_4_gib_decision():
    assert tiff.strip_layout(512, 512)[0] == 32 and len(tiff.strip_layout(512, 512)[1]) == 16
    assert tiff.strip_layout(70, 77)[0] == 70 and tiff.strip_layout(5, 40000)[0] == 1
    rps, row0, rows = tiff.strip_layout(70, 77, 16)
    assert row0.tolist() == [0, 16, 32, 48, 64] and rows.tolist() == [16, 16, 16, 16, 6]
    for bad in (0, 71, -1):
        with pytest.raises(ValueError, match='rows_per_strip'):
            tiff.strip_layout(70, 77, bad)
    # 512 x 512 pages: 524288 raw bytes; all stored they take 16 * (32768 + 11) + 1 + an IFD
    page = 16 * tiff.stored_bound(32768) + 1
    assert tiff.stored_bound(32768) == 32779
    small, large = (1 << 32) // (page + 400), (1 << 32) // page + 1
    assert tiff.file_bound(small, 512, 512, None, False) < 1 << 32 <= tiff.file_bound(large, 512, 512, None, False)
    assert tiff.choose_bigtiff(small, 512, 512) is False and tiff.choose_bigtiff(large, 512, 512) is True
    assert tiff.choose_bigtiff(small, 512, 512, bigtiff=True) is True and tiff.choose_bigtiff(small, 512, 512, bigtiff=False) is False
    with pytest.raises(ValueError, match='4 GiB'):
        tiff.choose_bigtiff(large, 512, 512, bigtiff=False)
    # the bound is one: a real IFD is never larger than what file_bound sets aside for it
    for big in (False, True):
        for n in (1, 2, 16):
            ifd, _ = tiff.build_ifd(1000, 16 * n, 80, 16, 2, big, [10 ** 9] * n, [33000] * n, b'x' * 11)
            assert len(ifd) <= tiff._ifd_size(n, big, 12)
