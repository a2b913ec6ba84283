"""Helpers of tests/test_tiff_deflate_cpu.py and tests/test_tiff_deflate_gpu.py: the battery of strips that both the host
program (tests/tiff_deflate_host.cpp, under the sanitizers) and the kernel of csrc/tiff_deflate.hip deflate, a walk over a
stream's block types with the textbook inflater of tests/tiff_inflate_cases.py (imported, not edited), and plain-numpy
restatements of the predictor and of what process_timelapse does to a recording.

Each case is a strip: uint16 [rows, W] and a predictor. The shapes are the smallest at which the encoder can still go
wrong: one and two samples, odd sizes, exactly 32768 bytes, more than 65535 bytes (two stored pieces, positions beyond the
Deflate window), a match at distance exactly 32768, several fillings of the token buffer with blocks of different types,
a code set over all 256 byte values and many match lengths, and Fibonacci frequencies whose unrestricted Huffman code
would be deeper than 15 bits."""
import collections
import functools
import os
import struct
import subprocess

import numpy as np

import tiff_cases as tc
import tiff_inflate_cases as ic

DeflateCase = collections.namedtuple('DeflateCase', 'name a predictor')


def stored_bytes(a, predictor=1):
    """The strip's bytes as stored: little-endian, with predictor 2 every sample minus its left neighbour modulo 2^16."""
    a = np.asarray(a, np.uint16)
    if predictor == 2:
        d = a.astype(np.int64)
        d[:, 1:] -= a[:, :-1].astype(np.int64)
        a = (d & 0xffff).astype(np.uint16)
    return a.astype('<u2').tobytes()


def bound(raw):
    """raw + 5 * max(1, ceil(raw / 65535)) + 6: the all-stored stream."""
    return raw + 5 * max(1, -(-raw // 65535)) + 6


def sparse_frame(shape, seed, density=0.02):
    """2 % of the samples non-zero, values 200..4000."""
    rng = np.random.default_rng(seed)
    v = rng.integers(200, 4001, shape)
    return np.where(rng.random(shape) < density, v, 0).astype(np.uint16)


def blobs_frame(shape, seed, n_blobs=6):
    """Gaussian blobs (sigma 2..5, peak 500..3000) on a sparse frame."""
    rng = np.random.default_rng(seed)
    H, W = shape
    y, x = np.mgrid[:H, :W]
    a = sparse_frame(shape, seed + 1000).astype(np.float64)
    for _ in range(n_blobs):
        cy, cx, s, peak = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(2, 5), rng.uniform(500, 3000)
        a += peak * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
    return np.clip(np.rint(a), 0, 65535).astype(np.uint16)


def camera_frame(shape, seed):
    """Normal noise around 121, sigma 6: a dark camera frame."""
    return np.clip(np.rint(np.random.default_rng(seed).normal(121, 6, shape)), 0, 65535).astype(np.uint16)


def zeros_frame(shape, seed=0):
    return np.zeros(shape, np.uint16)


FRAME_KINDS = {'sparse': sparse_frame, 'blobs': blobs_frame, 'zeros': zeros_frame, 'camera': camera_frame,
               'noise': lambda shape, seed: tc.noise(shape, seed)}


def _from_bytes(data, W):
    data = bytes(data)
    assert len(data) % (2 * W) == 0, (len(data), W)
    return np.frombuffer(data, '<u2').astype(np.uint16).reshape(-1, W)


def fibonacci_strip(seed=7, W=77):
    """Byte value k occurs F(k) times, k = 1..18 (F(1) = F(2) = 1), shuffled; padded with the value 18 to whole rows of W
    samples. An unrestricted Huffman code of these frequencies is 17 deep."""
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    data = np.concatenate([np.full(f, k + 1, np.uint8) for k, f in enumerate(fib)])
    np.random.default_rng(seed).shuffle(data)
    pad = -len(data) % (2 * W)
    return _from_bytes(np.concatenate([data, np.full(pad, 18, np.uint8)]).tobytes(), W)


def all_values_strip(seed=8, W=80):
    """All 256 byte values with skewed frequencies, and between them runs of 3..258 equal bytes: literals over the whole
    alphabet and (nearly) every length symbol in one strip."""
    rng = np.random.default_rng(seed)
    parts = [np.arange(256, dtype=np.uint8)]
    for length in range(3, 259, 5):
        parts.append(rng.integers(0, 256, 40).astype(np.uint8) // (1 + length % 7))
        parts.append(np.full(length + 1, length & 255, np.uint8))
    data = np.concatenate(parts)
    pad = -len(data) % (2 * W)
    return _from_bytes(np.concatenate([data, rng.integers(0, 256, pad).astype(np.uint8)]).tobytes(), W)


@functools.lru_cache(maxsize=None)
def deflate_cases():
    cases = []

    def add(name, a, predictors=(1, 2)):
        for pr in predictors:
            cases.append(DeflateCase(f'{name}_p{pr}', np.ascontiguousarray(a, np.uint16), pr))
    add('one_sample', tc.noise((1, 1), 201))
    add('two_samples', tc.noise((1, 2), 202))
    add('sparse_7x77', tc.sparse((7, 77), 0.1, 203))
    add('sparse_16x80', tc.sparse((16, 80), 0.1, 204))
    add('zeros_32x512', zeros_frame((32, 512)))
    add('period2_16x80', np.tile(np.array([513, 7], np.uint16), 640).reshape(16, 80))
    add('period3_7x77', np.resize(np.array([1000, 2, 40000], np.uint16), 7 * 77).reshape(7, 77))
    add('sparse_32x512', sparse_frame((32, 512), 0))
    add('blobs_32x512', blobs_frame((32, 512), 0))
    add('camera_32x512', camera_frame((32, 512), 0))
    add('noise_16x80', tc.noise((16, 80), 205))
    add('noise_66x512', tc.noise((66, 512), 206), (1,))
    add('sparse_66x512', sparse_frame((66, 512), 207))
    half = tc.sparse((32, 512), 0.3, 208)
    add('repeat_at_32768', np.concatenate([half, half]), (1,))
    add('half_noise_half_zeros_40x512', np.concatenate([tc.noise((20, 512), 209), zeros_frame((20, 512))]))
    add('all_values', all_values_strip(), (1,))
    add('fibonacci', fibonacci_strip(), (1,))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


def write_case_file(path, cases):
    """What tests/tiff_deflate_host.cpp reads (little-endian): count; per case three int32 (predictor, rows, W) and the
    rows * W samples."""
    with open(path, 'wb') as f:
        f.write(struct.pack('<i', len(cases)))
        for c in cases:
            f.write(struct.pack('<3i', c.predictor, c.a.shape[0], c.a.shape[1]))
            f.write(np.ascontiguousarray(c.a, '<u2').tobytes())


def read_result_file(path, n_cases):
    """What it writes: per case int32 status, int64 length, int64 batches, the stream."""
    out = []
    with open(path, 'rb') as f:
        for _ in range(n_cases):
            status, length, batches = struct.unpack('<iqq', f.read(20))
            out.append((status, f.read(length), batches))
        assert f.read() == b''
    return out


def build_host_program(tmp, sanitize):
    """tests/tiff_deflate_host.cpp, a stand-alone program with its own main, compiled for the host only; sanitize: with
    AddressSanitizer and UBSan (the program is run directly, nothing is preloaded)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp), 'tiff_deflate_host')
    san = ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all'] if sanitize else []
    subprocess.check_call(['/opt/rocm/bin/hipcc', '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g'] + san +
                          [f'-I{os.path.join(root, "axtrack_amd", "csrc")}', os.path.join(root, 'tests', 'tiff_deflate_host.cpp'), '-o', exe])
    return exe


def run_host_program(exe, cases, tmp, tag='a'):
    """-> (the process's result, [(status, stream, batches)] per case)."""
    case_file, result_file = os.path.join(str(tmp), f'cases_{tag}.bin'), os.path.join(str(tmp), f'streams_{tag}.bin')
    write_case_file(case_file, cases)
    res = subprocess.run([exe, case_file, result_file], capture_output=True, text=True)
    return res, (read_result_file(result_file, len(cases)) if res.returncode in (0, 1) else None)


def block_types(stream):
    """The BTYPE of every block of a zlib stream, in order, read with the textbook inflater's bit reader and code sets."""
    br = ic._BitReader(stream)
    br.get(16)
    types, final, produced = [], 0, 0
    while not final:
        final, btype = br.get(1), br.get(2)
        types.append(btype)
        assert btype != 3
        if btype == 0:
            br.align()
            n, inv = br.get(16), br.get(16)
            assert n == inv ^ 0xffff
            br.pos += 8 * n
            produced += n
            continue
        if btype == 1:
            ll, dd = ic._code_set(ic.FIXED_LL, ic.LENS), ic._code_set(ic.FIXED_D, ic.DISTS)
        else:
            n_ll, n_d, n_cl = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
            cl_lens = [0] * 19
            for k in range(n_cl):
                cl_lens[ic.CL_ORDER[k]] = br.get(3)
            cl = ic._code_set(cl_lens, ic.CODES)
            lens = []
            while len(lens) < n_ll + n_d:
                sym = ic._symbol(br, cl)
                if sym < 16:
                    lens.append(sym)
                elif sym == 16:
                    lens += [lens[-1]] * (3 + br.get(2))
                elif sym == 17:
                    lens += [0] * (3 + br.get(3))
                else:
                    lens += [0] * (11 + br.get(7))
            assert len(lens) == n_ll + n_d and max(lens) <= 15 and max(cl_lens) <= 7
            ll, dd = ic._code_set(lens[:n_ll], ic.LENS), ic._code_set(lens[n_ll:], ic.DISTS)
        while True:
            sym = ic._symbol(br, ll)
            if sym == 256:
                break
            if sym < 256:
                produced += 1
                continue
            produced += ic.LENGTH_BASE[sym - 257] + br.get(ic.LENGTH_EXTRA[sym - 257])
            sym = ic._symbol(br, dd)
            br.get(ic.DIST_EXTRA[sym])
    return types


# ------------------------------------------------------------------------------------------------ notebook 01, restated
def ref_process(stack, offset=0, mask=None, second_mask=None, to_shape=None, H_slice=None, W_slice=None):
    """uint16 [T,H,W] -> (stack, mask): values below `offset` become 0 and the rest lose it; pixels outside the second mask
    and then outside the mask become 0; zero padding of (to - size) // 2 on both sides of an axis that is smaller than
    to_shape (an odd difference ends one short); then the slices. The mask is padded and sliced alike."""
    s = np.asarray(stack, np.uint16).astype(np.int64)
    s = np.where(s < offset, 0, s - offset)
    T, H, W = s.shape
    m = np.ones((H, W), bool) if mask is None else np.asarray(mask, bool)
    if second_mask is not None:
        s[:, ~np.asarray(second_mask, bool)] = 0
    if mask is not None:
        s[:, ~m] = 0
    if to_shape is not None:
        ph, pw = (to_shape[0] - H) // 2, (to_shape[1] - W) // 2
        s = np.pad(s, ((0, 0), (ph, ph), (pw, pw)))
        m = np.pad(m, ((ph, ph), (pw, pw)))
    hs, ws = (slice(*v) if v is not None else slice(None) for v in (H_slice, W_slice))          # (start, stop) pairs
    return s[:, hs, ws].astype(np.uint16), m[hs, ws]
