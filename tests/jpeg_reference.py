"""A reference for the JPEG encoder of csrc/jpeg_encode.h / csrc/jpeg.hip, written from the specification in DESIGN.md
6.8i and from nothing else: one block after the other, one bit after the other, numpy int64 and plain Python. It knows
nothing of rows coded in parallel, of scans or of launch shapes, and it does not import axtrack_amd.jpeg. Its Huffman
tables are the DHT segments of a file Pillow (libjpeg) writes with optimize=False, and its quantisation tables are
checked against what Pillow reads back from such a file at the same quality.

encode_scan(rgb, quality) -> (the entropy-coded segment, facts about it that tests/jpeg_cases.py asserts)."""
import functools
import io
import math
import struct

import numpy as np
from PIL import Image

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
BASE_LUM = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80,
            62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98,
            112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
               99, 99] + [99] * 32
# C[u][x] = round(8192 k(u) cos((2x + 1) u pi / 16))
DCT = np.array([[int(round(8192 * (math.sqrt(1 / 8) if u == 0 else 0.5) * math.cos((2 * x + 1) * u * math.pi / 16)))
                 for x in range(8)] for u in range(8)], np.int64)


def segments(data):
    """(marker, payload) of every segment of a JPEG file up to and including SOS."""
    assert data[:2] == b'\xff\xd8'
    i, out = 2, []
    while True:
        assert data[i] == 0xFF, i
        marker, n = data[i + 1], struct.unpack('>H', data[i + 2:i + 4])[0]
        out.append((marker, data[i + 4:i + 2 + n]))
        i += 2 + n
        if marker == 0xDA:
            return out, i


def dht_tables(data):
    """{class << 4 | destination: (bits[16], vals)} of a JPEG file."""
    out = {}
    for marker, p in segments(data)[0]:
        j = 0
        while marker == 0xC4 and j < len(p):
            bits = list(p[j + 1:j + 17])
            out[p[j]] = (bits, list(p[j + 17:j + 17 + sum(bits)]))
            j += 17 + sum(bits)
    return out


def _pillow_file(quality):
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(buf, 'JPEG', quality=quality, optimize=False, subsampling=0)
    return buf.getvalue()


@functools.lru_cache(None)
def huffman_specs():
    """Pillow's (libjpeg's) standard tables."""
    t = dht_tables(_pillow_file(75))
    assert sorted(t) == [0x00, 0x01, 0x10, 0x11]
    return t


@functools.lru_cache(None)
def huffman_codes():
    """{table: {symbol: the code as a string of '0' / '1'}}, derived from the DHT the way Annex C says."""
    out = {}
    for ident, (bits, vals) in huffman_specs().items():
        code, k, tab = 0, 0, {}
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                tab[vals[k]] = format(code, f'0{length}b')
                code += 1
                k += 1
            code <<= 1
        out[ident] = tab
    return out


@functools.lru_cache(None)
def quant_tables(quality):
    """(luminance, chrominance), natural order, IJG scaling -- and equal to what Pillow reads back from its own file."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    tabs = tuple(tuple(min(255, max(1, (b * s + 50) // 100)) for b in base) for base in (BASE_LUM, BASE_CHROMA))
    q = Image.open(io.BytesIO(_pillow_file(quality))).quantization
    assert (tuple(q[0]), tuple(q[1])) == tabs, 'Pillow scales the Annex K tables differently'
    return tabs


def header(H, W, quality):
    """SOI .. SOS: JFIF APP0, two DQT, SOF0, four DHT (luminance DC, AC, chrominance DC, AC), DRI, SOS."""
    seg = lambda m, p: struct.pack('>BBH', 0xFF, m, len(p) + 2) + p
    out = b'\xff\xd8' + seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for k, t in enumerate(quant_tables(quality)):
        out += seg(0xDB, bytes([k]) + bytes(t[n] for n in ZIGZAG))
    out += seg(0xC0, struct.pack('>BHHB', 8, H, W, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for ident in (0x00, 0x10, 0x01, 0x11):
        bits, vals = huffman_specs()[ident]
        out += seg(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, struct.pack('>H', (W + 7) // 8))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def ycc(rgb):
    """int64 [H, W, 3]: Y, Cb, Cr of uint8 RGB, level-shifted."""
    R, G, B = (rgb[..., k].astype(np.int64) for k in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    return np.stack([Y, Cb, Cr], -1) - 128


def block_coefficients(p, q):
    """One 8 x 8 block p (int64, [y][x]) -> its 64 quantised coefficients in zigzag order; q natural order."""
    t = (p @ DCT.T + 1024) >> 11                       # rows:    t[y][u] = sum_x C[u][x] p[y][x]
    c = (DCT @ t + 16384) >> 15                        # columns: c[v][u] = sum_y C[v][y] t[y][u]
    assert np.abs(p @ DCT.T).max() < 2 ** 31 and np.abs(DCT @ t).max() < 2 ** 31
    c = c.reshape(64)
    Q = np.array(q, np.int64)
    m = (np.abs(c) + (Q >> 1)) // Q
    return (np.sign(c) * m)[ZIGZAG]


def _value_bits(v, cat):
    return format(v if v >= 0 else v + (1 << cat) - 1, f'0{cat}b') if cat else ''


def encode_scan(rgb, quality):
    """uint8 [H, W, 3] -> (scan segment, facts). facts: per MCU row the bits before padding ('row_bits') and the positions
    of the 0xFF bytes in the row before stuffing ('ff_at'); the markers written; counts of ZRL symbols and of blocks that
    are an EOB only; the largest DC and AC category."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    H, W, _ = rgb.shape
    bh, bw = (H + 7) // 8, (W + 7) // 8
    yy = np.minimum(np.arange(8 * bh), H - 1)
    xx = np.minimum(np.arange(8 * bw), W - 1)
    planes = ycc(rgb[yy][:, xx])                        # the last row and column repeated into the padding
    qt = quant_tables(quality)
    codes = huffman_codes()
    facts = dict(row_bits=[], ff_at=[], markers=[], zrl=0, eob_only=0, dc_cat=0, ac_cat=0, dc_diffs=[])
    out = bytearray()
    for by in range(bh):
        pred = [0, 0, 0]
        bits = []
        for bx in range(bw):
            for c in range(3):
                zz = block_coefficients(planes[8 * by:8 * by + 8, 8 * bx:8 * bx + 8, c], qt[c != 0]).tolist()
                dc_tab, ac_tab = codes[0x00 | (c != 0)], codes[0x10 | (c != 0)]
                diff = zz[0] - pred[c]
                pred[c] = zz[0]
                cat = abs(diff).bit_length()
                assert cat <= 11
                facts['dc_cat'] = max(facts['dc_cat'], cat)
                facts['dc_diffs'].append(diff)
                bits.append(dc_tab[cat] + _value_bits(diff, cat))
                run = 0
                for k in range(1, 64):
                    v = zz[k]
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        bits.append(ac_tab[0xF0])
                        facts['zrl'] += 1
                        run -= 16
                    cat = abs(v).bit_length()
                    assert cat <= 10
                    facts['ac_cat'] = max(facts['ac_cat'], cat)
                    bits.append(ac_tab[run << 4 | cat] + _value_bits(v, cat))
                    run = 0
                if run:
                    bits.append(ac_tab[0x00])
                    facts['eob_only'] += run == 63
        row = ''.join(bits)
        facts['row_bits'].append(len(row))
        row += '1' * (-len(row) % 8)
        raw = int(row, 2).to_bytes(len(row) // 8, 'big')
        facts['ff_at'].append([i for i, b in enumerate(raw) if b == 0xFF])
        out += raw.replace(b'\xff', b'\xff\x00')
        if by < bh - 1:
            out += bytes([0xFF, 0xD0 + by % 8])
            facts['markers'].append(0xD0 + by % 8)
    return bytes(out), facts


def encode(rgb, quality):
    """A whole JPEG file of one frame."""
    return header(rgb.shape[0], rgb.shape[1], quality) + encode_scan(rgb, quality)[0] + b'\xff\xd9'


def psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    mse = float((d * d).mean())
    return float('inf') if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)
