"""Helpers of tests/test_tiff_cpu.py and tests/test_tiff_gpu.py: a small TIFF writer, encoders for PackBits and TIFF's LZW,
a reference decoder that returns the status codes of include/axtrack_hip_tiff.h, and the list of strip cases both the
host program (tests/tiff_decode_host.cpp, under the sanitizers) and the kernels decode.

Everything here is pure Python / numpy and independent of axtrack_amd/tiff.py and csrc/tiff_decode.h: the reference
decoder keeps a table of byte strings, the textbook formulation, not the offset / length table of the code under test."""
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tiff')
OK, SHORT_INPUT, BAD_CODE, OVERRUN, BAD_SEGMENT = 0, 1, 2, 3, 4
NONE, LZW, PACKBITS, ADOBE_DEFLATE, DEFLATE = 1, 5, 32773, 8, 32946
CLEAR, EOI, FIRST = 256, 257, 258


# ================================================================================================== encoders
class _BitWriter:
    def __init__(self):
        self.acc, self.nbits, self.out = 0, 0, bytearray()

    def put(self, code, width):
        self.acc = self.acc << width | code
        self.nbits += width
        while self.nbits >= 8:
            self.nbits -= 8
            self.out.append(self.acc >> self.nbits & 0xff)
        self.acc &= (1 << self.nbits) - 1

    def bytes(self):
        tail = bytes([self.acc << (8 - self.nbits) & 0xff]) if self.nbits else b''
        return bytes(self.out) + tail


def lzw_encode(data, leading_clear=True, eoi=True, clear_at=4094, return_codes=False):
    """TIFF 6.0 LZW: codes most significant bit first, 9 to 12 bits, the width changing one code early, Clear when the
    table reaches `clear_at` entries (the specification's 4094). clear_at=None never clears and stops adding entries at
    4096 (a writer that owes a Clear: decoders refuse what follows)."""
    data = bytes(data)
    bw, codes = _BitWriter(), []
    width, nxt, table = 9, FIRST, {}                    # table: (code of the string so far) << 8 | next byte -> code

    def emit(code):
        bw.put(code, width)
        codes.append((code, width))
    if leading_clear:
        emit(CLEAR)
    w = -1                                              # the code of the string matched so far; -1: none
    for c in data:
        if w < 0:
            w = c
            continue
        key = w << 8 | c
        hit = table.get(key)
        if hit is not None:
            w = hit
            continue
        emit(w)
        if nxt < 4096:
            table[key] = nxt
        nxt += 1
        if clear_at is not None and nxt == clear_at:
            emit(CLEAR)
            width, nxt, table = 9, FIRST, {}
        elif nxt > (1 << width) - 1 and width < 12:
            width += 1
        w = c
    if w >= 0:
        emit(w)
        nxt += 1
        if nxt > (1 << width) - 1 and width < 12:
            width += 1
    if eoi:
        emit(EOI)
    return (bw.bytes(), codes) if return_codes else bw.bytes()


def pack_codes(codes):
    """[(code, width)] -> bytes, MSB first: for hand-made (malformed) LZW streams."""
    bw = _BitWriter()
    for code, width in codes:
        bw.put(code, width)
    return bw.bytes()


def packbits_encode(data, row_bytes=None):
    """PackBits, each row packed on its own as TIFF 6.0 asks (row_bytes None: the whole input is one row)."""
    data = bytes(data)
    row_bytes = row_bytes or max(len(data), 1)
    out = bytearray()
    for r0 in range(0, len(data), row_bytes):
        row = data[r0:r0 + row_bytes]
        i = 0
        while i < len(row):
            run = 1
            while i + run < len(row) and run < 128 and row[i + run] == row[i]:
                run += 1
            if run >= 2:
                out += bytes([(1 - run) & 0xff, row[i]])
                i += run
                continue
            j = i
            while j < len(row) and j - i < 128 and not (j + 1 < len(row) and row[j + 1] == row[j]):
                j += 1
            j = max(j, i + 1)
            out += bytes([j - i - 1]) + row[i:j]
            i = j
    return bytes(out)


# ================================================================================================== reference decoder
def ref_lzw(src, out_bytes):
    """-> (status, bytes). The textbook decoder with a table of strings; statuses as the header defines them."""
    src = bytes(src)
    nbits_total = 8 * len(src)
    value = int.from_bytes(src, 'big') if src else 0
    pos, width, out = 0, 9, bytearray()
    table = {}
    nxt, prev = FIRST, None
    while len(out) < out_bytes:
        if pos + width > nbits_total:
            return SHORT_INPUT, bytes(out)
        code = value >> (nbits_total - pos - width) & ((1 << width) - 1)
        pos += width
        if code == EOI:
            return SHORT_INPUT, bytes(out)
        if code == CLEAR:
            width, table, nxt, prev = 9, {}, FIRST, None
            continue
        if code < 256:
            s = bytes([code])
        elif prev is None:
            return BAD_CODE, bytes(out)
        elif code < nxt:
            s = table[code]
        elif code == nxt:
            s = prev + prev[:1]
        else:
            return BAD_CODE, bytes(out)
        if len(s) > out_bytes - len(out):
            return OVERRUN, bytes(out)
        if prev is not None:
            if nxt >= 4096:
                return BAD_CODE, bytes(out)
            table[nxt] = prev + s[:1]
            nxt += 1
            if nxt + 1 >= 1 << width and width < 12:
                width += 1
        out += s
        prev = s
    return OK, bytes(out)


def ref_packbits(src, out_bytes):
    src = bytes(src)
    pos, out = 0, bytearray()
    while len(out) < out_bytes:
        if pos >= len(src):
            return SHORT_INPUT, bytes(out)
        n = src[pos] - 256 if src[pos] > 127 else src[pos]
        pos += 1
        if n == -128:
            continue
        if n >= 0:
            if n + 1 > len(src) - pos:
                return SHORT_INPUT, bytes(out)
            s = src[pos:pos + n + 1]
            pos += n + 1
        else:
            if pos >= len(src):
                return SHORT_INPUT, bytes(out)
            s = src[pos:pos + 1] * (1 - n)
            pos += 1
        if len(s) > out_bytes - len(out):
            return OVERRUN, bytes(out)
        out += s
    return OK, bytes(out)


def ref_decode_segment(src, rows, W, compression, predictor=1, big_endian=False):
    """One strip -> (status, uint16 [rows, W] or None)."""
    n = rows * W * 2
    if compression == NONE:
        status, raw = (OK, bytes(src[:n])) if len(src) >= n else (SHORT_INPUT, b'')
    elif compression == LZW:
        status, raw = ref_lzw(src, n)
    elif compression == PACKBITS:
        status, raw = ref_packbits(src, n)
    elif compression in (ADOBE_DEFLATE, DEFLATE):
        raw = zlib.decompress(bytes(src))
        status = OK if len(raw) >= n else SHORT_INPUT
        raw = raw[:n]
    else:
        raise ValueError(compression)
    if status != OK:
        return status, None
    a = np.frombuffer(raw, '>u2' if big_endian else '<u2').astype(np.uint16).reshape(rows, W)
    if predictor == 2:
        a = np.cumsum(a.astype(np.uint32), axis=1).astype(np.uint16)      # (a sum of < 2^16 terms below 2^16: exact in u32)
    return status, a


def ref_check_segment(src_offset, src_bytes, dst_offset, rows, W, src_len, out_len):
    if min(src_offset, src_bytes, dst_offset, rows, W, src_len, out_len) < 0:
        return BAD_SEGMENT
    if src_offset + src_bytes > src_len or rows * W > 0x7fffffff or dst_offset + rows * W > out_len:
        return BAD_SEGMENT
    return OK


def ref_read(path, info):
    """The whole file through the reference decoder and a parsed segment table (axtrack_amd.tiff.tiff_info's)."""
    T, H, W = info.shape
    buf = open(path, 'rb').read()
    out = np.zeros((T, H, W), np.uint16)
    for k in range(len(info.src_offset)):
        o, n = int(info.src_offset[k]), int(info.src_bytes[k])
        status, a = ref_decode_segment(buf[o:o + n], int(info.rows[k]), W, info.compression, info.predictor, info.byteorder == '>')
        assert status == OK, (k, status)
        r0 = int(info.row0[k])
        out[int(info.frame[k]), r0:r0 + int(info.rows[k])] = a
    return out


# ================================================================================================== strip encoding
def encode_strip(a, compression=NONE, predictor=1, big_endian=False, **lzw_kw):
    """uint16 [rows, W] -> the strip's bytes."""
    a = np.asarray(a, np.uint16)
    if predictor == 2:
        d = a.copy()
        d[:, 1:] = a[:, 1:] - a[:, :-1]                                  # (modulo 2^16)
        a = d
    raw = a.astype('>u2' if big_endian else '<u2').tobytes()
    if compression == NONE:
        return raw
    if compression == LZW:
        return lzw_encode(raw, **lzw_kw)
    if compression == PACKBITS:
        return packbits_encode(raw, a.shape[1] * 2)
    if compression in (ADOBE_DEFLATE, DEFLATE):
        return zlib.compress(raw, 6)
    raise ValueError(compression)


# ================================================================================================== TIFF writer
def write_tiff(path, stack, byteorder='<', bigtiff=False, rows_per_strip=None, compression=NONE, predictor=1, odd_offsets=False,
               imagej=False, tags_override=None, reduced_copies=False, omit_rows_per_strip=False, **lzw_kw):
    """stack uint16 [T, H, W] -> a TIFF file, strips first and the IFD chain behind them. imagej: ONE IFD whose description
    says images=T, the raw frames back to back behind its first strip (ImageJ's layout for stacks beyond 4 GB).
    odd_offsets: every strip starts at an odd file offset. tags_override: {tag: (type, [values]) or None} replaces or drops
    tags of every IFD. reduced_copies: a NewSubfileType = 1 page (a 1 x 1 thumbnail) behind every page.
    -> list over pages of (strip offsets, strip byte counts)."""
    stack = np.asarray(stack, np.uint16)
    T, H, W = stack.shape
    bo, big_endian = byteorder, byteorder == '>'
    rps = H if rows_per_strip is None else int(rows_per_strip)
    body = bytearray(b'II' if bo == '<' else b'MM')
    body += struct.pack(bo + 'HHHQ', 43, 8, 0, 0) if bigtiff else struct.pack(bo + 'HI', 42, 0)
    layout = []

    def place(data):
        if odd_offsets and len(body) % 2 == 0:
            body.append(0xee)
        off = len(body)
        body.extend(data)
        return off

    if imagej:
        assert compression == NONE and predictor == 1
        off = place(stack.astype('>u2' if big_endian else '<u2').tobytes())
        layout.append(([off], [H * W * 2]))
        pages = [0]
    else:
        pages = range(T)
        for t in pages:
            offs, cnts = [], []
            for r0 in range(0, H, rps):
                data = encode_strip(stack[t, r0:r0 + rps], compression, predictor, big_endian, **lzw_kw)
                offs.append(place(data))
                cnts.append(len(data))
            layout.append((offs, cnts))
    LONG = 16 if bigtiff else 4
    ifds = []
    for i, t in enumerate(pages):
        offs, cnts = layout[i]
        tags = {254: (4, [0]), 256: (4, [W]), 257: (4, [H]), 258: (3, [16]), 259: (3, [compression]), 262: (3, [1]),
                273: (LONG, offs), 277: (3, [1]), 278: (4, [H if imagej else rps]), 279: (LONG, cnts), 339: (3, [1])}
        if predictor != 1:
            tags[317] = (3, [predictor])
        if imagej:
            tags[270] = (2, f'ImageJ=1.53t\nimages={T}\nframes={T}\nloop=false\n'.encode() + b'\0')
        if omit_rows_per_strip:
            del tags[278]
        for k, v in (tags_override or {}).items():
            if v is None:
                tags.pop(k, None)
            else:
                tags[k] = v
        ifds.append(tags)
        if reduced_copies:
            o = place(b'\0\0')
            ifds.append({254: (4, [1]), 256: (4, [1]), 257: (4, [1]), 258: (3, [16]), 259: (3, [1]), 262: (3, [1]), 273: (LONG, [o]),
                         277: (3, [1]), 278: (4, [1]), 279: (LONG, [2])})
    letters = {1: 'B', 3: 'H', 4: 'I', 16: 'Q'}
    sizes = {1: 1, 2: 1, 3: 2, 4: 4, 16: 8}
    inline = 8 if bigtiff else 4
    first, patch_at = None, None
    for tags in ifds:
        entries = []
        for tag in sorted(tags):
            ftype, vals = tags[tag]
            data = bytes(vals) if ftype == 2 else struct.pack(bo + letters[ftype] * len(vals), *vals)
            count = len(vals)
            if len(data) > inline:
                if len(body) % 2:
                    body.append(0)
                where = len(body)
                body.extend(data)
                data = struct.pack(bo + ('Q' if bigtiff else 'I'), where)
            entries.append(struct.pack(bo + 'HH' + ('Q' if bigtiff else 'I'), tag, ftype, count) + data.ljust(inline, b'\0'))
        if len(body) % 2:
            body.append(0)
        here = len(body)
        if first is None:
            first = here
        else:
            body[patch_at:patch_at + inline] = struct.pack(bo + ('Q' if bigtiff else 'I'), here)
        body += struct.pack(bo + ('Q' if bigtiff else 'H'), len(entries)) + b''.join(entries)
        patch_at = len(body)
        body += b'\0' * inline
    hdr = 8 if bigtiff else 4
    body[hdr:hdr + inline] = struct.pack(bo + ('Q' if bigtiff else 'I'), first)
    with open(path, 'wb') as f:
        f.write(body)
    return layout


# ================================================================================================== synthetic frames
def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 65536, shape).astype(np.uint16)


def sparse(shape, density, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 65536, shape).astype(np.uint16)
    return np.where(rng.random(shape) < density, a, 0).astype(np.uint16)


# ================================================================================================== strip cases
class Case:
    def __init__(self, name, src, rows, W, compression, predictor=1, big_endian=False, expect=None, status=OK):
        self.name, self.src, self.rows, self.W = name, bytes(src), rows, W
        self.compression, self.predictor, self.big_endian, self.expect, self.status = compression, predictor, big_endian, expect, status


def _good(name, a, compression, predictor=1, big_endian=False, **kw):
    a = np.asarray(a, np.uint16)
    return Case(name, encode_strip(a, compression, predictor, big_endian, **kw), a.shape[0], a.shape[1], compression, predictor,
                big_endian, a, OK)


def packbits_handmade():
    """Literal runs of 1 and 128 bytes, repeat runs of 2 and 128, a -128 header, a run that ends exactly at the segment end.
    -> (stream, decoded bytes): 1 + 128 + 2 + 128 + 3 = 262 bytes = 131 samples."""
    lit128 = bytes((7 * i + 3) & 0xff for i in range(128))
    stream = bytes([0, 0x41]) + bytes([127]) + lit128 + bytes([0xff, 0x42]) + bytes([0x80]) + bytes([0x81, 0x43]) + bytes([0x80]) \
        + bytes([0xfe, 0x44])
    return stream, b'\x41' + lit128 + b'\x42' * 2 + b'\x43' * 128 + b'\x44' * 3


def decode_cases():
    """The strip cases, good and malformed. Each malformed stream is built from a good one so that exactly one thing is
    wrong with it, and its status is what the reference decoder above returns for it."""
    cases = []
    n64 = noise((64, 80), 11)
    cases.append(_good('lzw_noise_64x80', n64, LZW))
    cases.append(_good('lzw_sparse_256x160', sparse((256, 160), 0.02, 12), LZW))
    cases.append(_good('lzw_zeros_64x80', np.zeros((64, 80), np.uint16), LZW))
    cases.append(_good('lzw_no_leading_clear', sparse((16, 77), 0.1, 13), LZW, leading_clear=False))
    cases.append(_good('lzw_no_eoi', sparse((16, 77), 0.1, 14), LZW, eoi=False))
    cases.append(_good('lzw_big_endian_pred2_w77', sparse((5, 77), 0.3, 15), LZW, 2, True))
    cases.append(_good('lzw_pred2_w300', noise((3, 300), 16), LZW, 2, False))
    stream, raw = packbits_handmade()
    cases.append(Case('packbits_handmade', stream, 1, 131, PACKBITS, expect=np.frombuffer(raw, '<u2').reshape(1, 131)))
    cases.append(_good('packbits_sparse_50x77', sparse((50, 77), 0.1, 17), PACKBITS))
    cases.append(_good('packbits_noise_be_pred2', noise((4, 130), 18), PACKBITS, 2, True))
    cases.append(_good('raw_big_endian_pred2_w77', noise((7, 77), 19), NONE, 2, True))
    cases.append(_good('raw_big_endian_w300', noise((2, 300), 20), NONE, 1, True))
    cases.append(_good('raw_little_endian_pred2', noise((3, 65), 21), NONE, 2, False))
    cases.append(_good('one_sample', np.array([[54321]], np.uint16), LZW))
    cases.append(Case('empty_segment', b'', 0, 80, LZW, expect=np.zeros((0, 80), np.uint16)))

    # ---- malformed
    sp = sparse((16, 80), 0.1, 22)
    good = encode_strip(sp, LZW)
    cases.append(Case('lzw_truncated', good[:len(good) // 2], 16, 80, LZW, status=SHORT_INPUT))
    cases.append(Case('lzw_empty_input', b'', 16, 80, LZW, status=SHORT_INPUT))
    cases.append(Case('lzw_eoi_early', encode_strip(sp[:8], LZW), 16, 80, LZW, status=SHORT_INPUT))
    _, codes = lzw_encode(sp.tobytes(), return_codes=True)
    bad = list(codes)
    bad[40] = (300 + 40, bad[40][1])                    # far above the next free entry (258 + 38 at that point)
    cases.append(Case('lzw_code_above_next', pack_codes(bad), 16, 80, LZW, status=BAD_CODE))
    cases.append(Case('lzw_first_code_not_literal', pack_codes([(CLEAR, 9), (300, 9)] + codes[2:]), 16, 80, LZW, status=BAD_CODE))
    tail0 = sp.copy()
    tail0[14:] = 0                                      # zeros across the end of row 14: the string there is longer than what is left
    cases.append(Case('lzw_too_many_rows', encode_strip(tail0, LZW), 15, 80, LZW, status=OVERRUN))
    cases.append(Case('lzw_table_overflow', encode_strip(n64, LZW, clear_at=None), 64, 80, LZW, status=BAD_CODE))
    pb = encode_strip(sp, PACKBITS)
    cases.append(Case('packbits_truncated', pb[:len(pb) // 2], 16, 80, PACKBITS, status=SHORT_INPUT))
    cases.append(Case('packbits_literal_cut', bytes([5, 1, 2, 3]), 1, 8, PACKBITS, status=SHORT_INPUT))
    cases.append(Case('packbits_repeat_cut', bytes([0xfd]), 1, 8, PACKBITS, status=SHORT_INPUT))
    cases.append(Case('packbits_run_past_the_end', bytes([0, 9, 0xf1, 0x55]), 1, 4, PACKBITS, status=OVERRUN))
    cases.append(Case('raw_short', sp.tobytes()[:-2], 16, 80, NONE, status=SHORT_INPUT))
    for c in cases:                                     # the statuses above are the reference decoder's
        status, a = ref_decode_segment(c.src, c.rows, c.W, c.compression, c.predictor, c.big_endian)
        assert status == c.status, (c.name, status, c.status)
        assert c.status != OK or np.array_equal(a, c.expect), c.name
    return cases


DESCRIPTOR_CASES = [       # (src_offset, src_bytes, dst_offset, rows, W, src_len, out_len)
    (0, 10, 0, 1, 5, 10, 5), (0, 0, 0, 0, 5, 0, 0), (10, 0, 5, 0, 5, 10, 5),
    (0, 11, 0, 1, 5, 10, 5), (1, 10, 0, 1, 5, 10, 5), (11, 0, 0, 0, 5, 10, 5), (-1, 2, 0, 1, 1, 10, 5), (0, -1, 0, 1, 1, 10, 5),
    (0, 10, 1, 1, 5, 10, 5), (0, 10, 0, 2, 5, 10, 5), (0, 10, -1, 1, 5, 10, 5), (0, 10, 0, -1, 5, 10, 5), (0, 10, 6, 0, 5, 10, 5),
    (2 ** 62, 2 ** 62, 0, 1, 1, 2 ** 62 + 5, 5), (0, 0, 2 ** 62, 2 ** 31 - 1, 2 ** 31 - 1, 0, 2 ** 62 + 5),
    (0, 0, 0, 65536, 32768, 0, 2 ** 40), (0, 0, 0, 65535, 32768, 0, 2 ** 40),
]


def write_case_file(path, cases):
    """The binary case file tests/tiff_decode_host.cpp reads (little-endian): count; per case six int32 (compression,
    predictor, big_endian, rows, W, expected status), int64 src_bytes, the bytes, and for status 0 the rows * W expected
    samples; then the descriptor cases: count; per case seven int64 and the expected status as int32."""
    with open(path, 'wb') as f:
        f.write(struct.pack('<i', len(cases)))
        for c in cases:
            f.write(struct.pack('<6iq', c.compression, c.predictor, int(c.big_endian), c.rows, c.W, c.status, len(c.src)))
            f.write(c.src)
            if c.status == OK:
                f.write(np.ascontiguousarray(c.expect, '<u2').tobytes())
        f.write(struct.pack('<i', len(DESCRIPTOR_CASES)))
        for d in DESCRIPTOR_CASES:
            f.write(struct.pack('<7qi', *d, ref_check_segment(*d)))
