"""Helpers of tests/test_tiff_inflate_cpu.py and tests/test_tiff_inflate_gpu.py: an independent reference inflater that
returns the status codes of csrc/axt_tiff_inflate.h, a bit writer for hand-assembled Deflate streams, and the battery of
strip cases that both the host program (tests/tiff_inflate_host.cpp, under the sanitizers) and the kernel inflate.

The reference is the textbook formulation -- one bit at a time, a dictionary {(length, code): symbol} per code set, the
RFC's tables of length and distance bases written out -- and shares nothing with csrc/tiff_inflate.h, which keeps a 64-bit
bit buffer, direct lookup tables and closed forms for the bases. Its yardstick in turn is zlib.decompress
(test_tiff_inflate_cpu.py): status 0 exactly where zlib succeeds with rows * W * 2 bytes."""
import functools
import struct
import zlib

import numpy as np

import tiff_cases as tc

OK, SHORT_INPUT, BAD_CODE, OVERRUN, BAD_SEGMENT, BAD_CHECKSUM = 0, 1, 2, 3, 4, 5
INFLATE = tc.ADOBE_DEFLATE
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
CODES, LENS, DISTS = 0, 1, 2


# ================================================================================================== reference inflater
class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _BitReader:
    def __init__(self, src):
        self.bits = np.unpackbits(np.frombuffer(bytes(src), np.uint8), bitorder='little').tolist()
        self.pos = 0

    def get(self, n):
        if self.pos + n > len(self.bits):
            raise _Stop(SHORT_INPUT)
        v = 0
        for k in range(n):
            v |= self.bits[self.pos + k] << k
        self.pos += n
        return v

    def align(self):
        self.pos = (self.pos + 7) & ~7


def canonical_codes(lengths):
    """RFC 1951 3.2.2: {symbol: (length, code)} for the symbols of non-zero length."""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for sym, n in enumerate(lengths):
        if n:
            out[sym] = (n, nxt[n])
            nxt[n] += 1
    return out


def _code_set(lengths, kind):
    """-> {(length, code): symbol}, refusing what zlib's inflate refuses."""
    used = [n for n in lengths if n]
    space = sum(2 ** (15 - n) for n in used)                # Kraft sum in units of 2^-15
    if space > 2 ** 15:
        raise _Stop(BAD_CODE)                               # over-subscribed
    if not used:
        if kind != DISTS:
            raise _Stop(BAD_CODE)
        return {}
    if space < 2 ** 15 and (kind == CODES or max(used) != 1):
        raise _Stop(BAD_CODE)                               # incomplete, and not the single 1-bit code
    return {v: sym for sym, v in canonical_codes(lengths).items()}


def _symbol(br, codes):
    code = 0
    for n in range(1, 16):
        code = code << 1 | br.get(1)
        if (n, code) in codes:
            return codes[(n, code)]
    raise _Stop(BAD_CODE)


def adler32(data):
    a, b = 1, 0
    for c in data:
        a = (a + c) % 65521
        b = (b + a) % 65521
    return b << 16 | a


def _inflate(src, out_bytes):
    br, out = _BitReader(src), bytearray()
    cmf, flg = br.get(8), br.get(8)                          # (a one-byte input is short either way)
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf * 256 + flg) % 31 or flg & 32:
        raise _Stop(BAD_CODE)
    final = 0
    while not final:
        final, btype = br.get(1), br.get(2)
        if btype == 3:
            raise _Stop(BAD_CODE)
        if btype == 0:
            br.align()
            n, inv = br.get(16), br.get(16)
            if n != inv ^ 0xffff:
                raise _Stop(BAD_CODE)
            at = br.pos // 8
            if n > len(src) - at:
                raise _Stop(SHORT_INPUT)
            if n > out_bytes - len(out):
                raise _Stop(OVERRUN)
            out += src[at:at + n]
            br.pos += 8 * n
            continue
        if btype == 1:
            ll, dd = _code_set(FIXED_LL, LENS), _code_set(FIXED_D, DISTS)
        else:
            n_ll, n_d, n_cl = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
            if n_ll > 286 or n_d > 30:
                raise _Stop(BAD_CODE)
            cl = [0] * 19
            for k in range(n_cl):
                cl[CL_ORDER[k]] = br.get(3)
            cl = _code_set(cl, CODES)
            lens = []
            while len(lens) < n_ll + n_d:
                sym = _symbol(br, cl)
                if sym < 16:
                    lens.append(sym)
                    continue
                if sym == 16:
                    if not lens:
                        raise _Stop(BAD_CODE)
                    value, rep = lens[-1], 3 + br.get(2)
                elif sym == 17:
                    value, rep = 0, 3 + br.get(3)
                else:
                    value, rep = 0, 11 + br.get(7)
                if len(lens) + rep > n_ll + n_d:
                    raise _Stop(BAD_CODE)
                lens += [value] * rep
            if lens[256] == 0:
                raise _Stop(BAD_CODE)
            ll = _code_set(lens[:n_ll], LENS)
            dd = _code_set(lens[n_ll:], DISTS)
        while True:
            sym = _symbol(br, ll)
            if sym == 256:
                break
            if sym < 256:
                if len(out) >= out_bytes:
                    raise _Stop(OVERRUN)
                out.append(sym)
                continue
            if sym > 285:
                raise _Stop(BAD_CODE)
            length = LENGTH_BASE[sym - 257] + br.get(LENGTH_EXTRA[sym - 257])
            sym = _symbol(br, dd)
            if sym > 29:
                raise _Stop(BAD_CODE)
            dist = DIST_BASE[sym] + br.get(DIST_EXTRA[sym])
            if dist > len(out):
                raise _Stop(BAD_CODE)
            if length > out_bytes - len(out):
                raise _Stop(OVERRUN)
            for _ in range(length):
                out.append(out[-dist])
    if len(out) < out_bytes:
        raise _Stop(SHORT_INPUT)
    br.align()
    stored = 0
    for _ in range(4):
        stored = stored << 8 | br.get(8)
    if stored != adler32(out):
        raise _Stop(BAD_CHECKSUM)
    return bytes(out)


def ref_inflate(src, out_bytes):
    """One zlib stream -> (status, the out_bytes bytes or None)."""
    try:
        return OK, _inflate(bytes(src), out_bytes)
    except _Stop as e:
        return e.status, None


def ref_inflate_segment(src, rows, W, predictor=1, big_endian=False):
    status, raw = ref_inflate(src, rows * W * 2)
    if status != OK:
        return status, None
    a = np.frombuffer(raw, '>u2' if big_endian else '<u2').astype(np.uint16).reshape(rows, W)
    if predictor == 2:
        a = np.cumsum(a.astype(np.uint32), axis=1).astype(np.uint16)
    return status, a


# ================================================================================================== stream writers
def deflate(raw, level=-1, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_every=None, flush=zlib.Z_FULL_FLUSH):
    """zlib.compressobj with a level, a strategy, a window size, and optionally a flush every flush_every bytes."""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    out = b''
    if flush_every:
        for p in range(0, len(raw), flush_every):
            out += co.compress(raw[p:p + flush_every]) + co.flush(flush)
    else:
        out = co.compress(raw)
    return out + co.flush()


class BitWriter:
    """Deflate's bit order: fields least significant bit first, Huffman codes most significant bit first."""

    def __init__(self, header=b'\x78\x9c'):
        self.out, self.acc, self.n = bytearray(header), 0, 0

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, length_code):
        n, code = length_code
        return self.bits(int(format(code, f'0{n}b')[::-1], 2), n)

    def align(self):
        return self.bits(0, (8 - self.n) % 8)

    def stored(self, data, final=0, nlen=None):
        self.bits(final, 1).bits(0, 2).align()
        self.out += struct.pack('<HH', len(data), len(data) ^ 0xffff if nlen is None else nlen) + bytes(data)
        return self

    def finish(self, produced=None, adler=None):
        """Align and append the Adler-32 of `produced` (or `adler` as it is)."""
        self.align()
        self.out += struct.pack('>I', zlib.adler32(bytes(produced)) if adler is None else adler)
        return bytes(self.out)


class HuffmanBlock:
    """Symbols of one fixed or dynamic block, written through a BitWriter."""

    def __init__(self, bw, ll_lens, d_lens):
        self.bw, self.ll, self.dd = bw, canonical_codes(ll_lens), canonical_codes(d_lens)

    def literals(self, data):
        for c in bytes(data):
            self.bw.code(self.ll[c])
        return self

    def symbol(self, sym):
        self.bw.code(self.ll[sym])
        return self

    def match(self, length, dist, length_code=None):
        """length_code: the symbol to write the length with (258 is 285, or 284 with extra 31)."""
        k = max(i for i in range(29) if LENGTH_BASE[i] <= length) if length_code is None else length_code - 257
        assert 0 <= length - LENGTH_BASE[k] < 1 << LENGTH_EXTRA[k] or (LENGTH_EXTRA[k] == 0 and length == LENGTH_BASE[k])
        self.bw.code(self.ll[257 + k]).bits(length - LENGTH_BASE[k], LENGTH_EXTRA[k])
        j = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.bw.code(self.dd[j]).bits(dist - DIST_BASE[j], DIST_EXTRA[j])
        return self

    def end(self):
        return self.symbol(256)


def fixed_block(bw, final=0):
    bw.bits(final, 1).bits(1, 2)
    return HuffmanBlock(bw, FIXED_LL, FIXED_D)


def complete_lengths(n):
    """Code lengths of a complete code over n >= 2 symbols: the shorter codes first."""
    k = n.bit_length() - 1
    short = 2 ** (k + 1) - n
    return [k] * short + [k + 1] * (n - short)


CL_PLAIN = [4] * 13 + [5] * 6                                # a complete code-length code over all 19 symbols


def dynamic_block(bw, ll_lens, d_lens, final=0, cl_lens=CL_PLAIN, items=None, hlit=None, hdist=None):
    """The header of a dynamic block. items: the code-length symbols as (symbol, extra value) pairs; None: every length
    written plainly. hlit / hdist: the header fields as they are (None: from the lists)."""
    bw.bits(final, 1).bits(2, 2)
    bw.bits(len(ll_lens) - 257 if hlit is None else hlit, 5).bits(len(d_lens) - 1 if hdist is None else hdist, 5)
    n_cl = max(k + 1 for k in range(19) if cl_lens[CL_ORDER[k]] or k < 4)
    bw.bits(n_cl - 4, 4)
    for k in range(n_cl):
        bw.bits(cl_lens[CL_ORDER[k]], 3)
    cl = canonical_codes(cl_lens)
    if items is None:
        items = [(n, 0) for n in list(ll_lens) + list(d_lens)]
    for sym, extra in items:
        bw.code(cl[sym])
        if sym >= 16:
            bw.bits(extra, {16: 2, 17: 3, 18: 7}[sym])
    return HuffmanBlock(bw, ll_lens, d_lens)


# ================================================================================================== the battery
def raw_of(a, predictor=1, big_endian=False):
    return tc.encode_strip(a, tc.NONE, predictor, big_endian)


def _case(name, src, a, predictor=1, big_endian=False, status=OK):
    a = np.asarray(a, np.uint16)
    return tc.Case(name, src, a.shape[0], a.shape[1], INFLATE, predictor, big_endian, a if status == OK else None, status)


def _handmade_good():
    cases = []
    big = tc.noise((256, 80), 71)                            # 40960 bytes: beyond the 32 KiB window
    raw = raw_of(big)
    # a stored block of 32768 bytes, then distance exactly 32768 with length 258 in one match (as code 285), the same
    # with 284 + extra 31, a match of distance 1 and one with distance < length, all behind the window's first wrap
    out = bytearray(raw[:32768])
    bw = BitWriter().stored(out)
    blk = fixed_block(bw)

    def match(length, dist, **kw):
        blk.match(length, dist, **kw)
        for _ in range(length):
            out.append(out[-dist])
    match(258, 32768)
    match(258, 32768, length_code=284)
    match(258, 1)
    match(200, 7)
    match(3, 32768)
    lit = raw[len(out):len(out) + 300]
    blk.literals(lit)
    out += lit
    match(258, 32767)
    match(258, 32768 - 258)
    match(258, 32768 - 64)
    blk.end()
    rest = 40960 - len(out)
    out += raw[:rest]
    bw.stored(raw[:rest], final=1)
    cases.append(_case('hand_window_32768_and_wrap', bw.finish(out), np.frombuffer(bytes(out), '<u2').reshape(256, 80)))
    # matches that cross the wrap of a 32 KiB ring: the output position passes 32768 inside a distance-1 match and inside
    # one with distance < length
    out = bytearray(raw[:32768 - 100])
    bw = BitWriter().stored(out)
    blk = fixed_block(bw)
    match(258, 1)                                            # 32668 .. 32926
    blk.literals(raw[:5])
    out += raw[:5]
    for _ in range(25):
        match(258, 5)
    match(258, 32768)
    blk.end()
    rest = 40960 - len(out)
    out += raw[100:100 + rest]
    bw.stored(raw[100:100 + rest], final=1)
    cases.append(_case('hand_matches_across_the_wrap', bw.finish(out), np.frombuffer(bytes(out), '<u2').reshape(256, 80)))
    # dynamic blocks zlib never writes
    sp = tc.sparse((7, 77), 0.1, 72)
    raw = raw_of(sp)
    ll = complete_lengths(257)
    blk = dynamic_block(BitWriter(), ll, [0], final=1)       # an all-zero distance set, literals only
    cases.append(_case('hand_all_zero_distance_set', blk.literals(raw).end().bw.finish(raw), sp))
    one = np.full((16, 80), 0x4141, np.uint16)               # one byte value throughout: distance 1 is all it needs
    raw = raw_of(one)
    blk = dynamic_block(BitWriter(), complete_lengths(286), [1], final=1)               # a one-code distance set
    blk.literals(raw[:1])
    n = 1
    while n < len(raw):
        step = min(258, len(raw) - n)
        if step < 3:
            blk.literals(raw[n:n + step])
        else:
            blk.match(step, 1)
        n += step
    cases.append(_case('hand_one_code_distance_set', blk.end().bw.finish(raw), one))
    # an end-of-block-only literal/length set of one 1-bit code: a final block without output behind a stored one
    raw = raw_of(sp)
    bw = BitWriter().stored(raw)
    lens = [0] * 256 + [1]
    dynamic_block(bw, lens, [0], final=1).end()
    cases.append(_case('hand_single_code_end_of_block_set', bw.finish(raw), sp))
    # stored blocks of LEN 0 and LEN 65535
    wide = tc.noise((410, 80), 75)                           # 65600 bytes
    raw = raw_of(wide)
    bw = BitWriter().stored(b'').stored(raw[:65535]).stored(b'').stored(raw[65535:], final=1)
    cases.append(_case('hand_stored_0_and_65535', bw.finish(raw), wide))
    # a final block that is empty, after the output is complete: fixed, and stored
    raw = raw_of(sp)
    bw = BitWriter()
    fixed_block(bw).literals(raw).end()
    fixed_block(bw, final=1).end()
    cases.append(_case('hand_empty_final_fixed_block', bw.finish(raw), sp))
    cases.append(_case('hand_empty_final_stored_block', BitWriter().stored(raw).stored(b'', final=1).finish(raw), sp))
    return cases


def _malformed():
    sp = tc.sparse((16, 80), 0.1, 81)
    raw = raw_of(sp)
    half = len(raw) // 2
    good = zlib.compress(raw, 6)
    cases = []

    def bad(name, src, status):
        cases.append(_case(name, src, sp, status=status))

    def header(cmf, flg_base):
        flg = flg_base + (31 - (cmf * 256 + flg_base) % 31) % 31
        return bytes([cmf, flg]) + good[2:]
    bad('bad_header_cm', header(0x77, 0x80), BAD_CODE)
    bad('bad_header_cinfo', header(0x88, 0x80), BAD_CODE)
    bad('bad_header_check_bits', bytes([good[0], good[1] ^ 1]) + good[2:], BAD_CODE)
    bad('bad_header_fdict', header(0x78, 0xa0), BAD_CODE)

    def fixed_then(f):
        """half the bytes as literals of a fixed block, then what f writes"""
        bw = BitWriter()
        blk = fixed_block(bw).literals(raw[:half])
        return f(bw, blk)

    def rest_fixed(bw):
        fixed_block(bw, final=1).literals(raw[half:]).end()
        return bw.finish(raw)
    bad('btype_3', fixed_then(lambda bw, blk: rest_fixed(blk.end().bw.bits(0, 1).bits(3, 2))), BAD_CODE)
    bw = BitWriter().stored(raw[:half]).stored(raw[half:], final=1, nlen=(len(raw) - half) ^ 0xfffe)
    bad('stored_len_nlen_mismatch', bw.finish(raw), BAD_CODE)
    bad('symbol_286', fixed_then(lambda bw, blk: rest_fixed(bw.code((8, 0b11000110)))), BAD_CODE)
    bad('distance_symbol_30', fixed_then(lambda bw, blk: rest_fixed(blk.symbol(257).bw.code((5, 30)))), BAD_CODE)
    bw = BitWriter()
    fixed_block(bw, final=1).literals(raw[:3]).match(3, 4).literals(raw[6:]).end()
    bad('distance_before_the_start', bw.finish(raw), BAD_CODE)
    ll257 = complete_lengths(257)

    def dyn(name, status, *a, body=True, **kw):
        bw = BitWriter().stored(raw[:half])
        blk = dynamic_block(bw, *a, final=1, **kw)
        if body:
            blk.literals(raw[half:]).end()
        bad(name, bw.finish(raw), status)
    dyn('hlit_287', BAD_CODE, ll257, [0], hlit=30, body=False)
    dyn('hdist_31', BAD_CODE, ll257, [0], hdist=30, body=False)
    plain = [(n, 0) for n in ll257 + [0]]
    dyn('repeat_16_first', BAD_CODE, ll257, [0], items=[(16, 0)] + plain[3:], body=False)
    dyn('repeat_past_the_end', BAD_CODE, ll257, [0], items=plain[:-2] + [(16, 3)], body=False)
    dyn('repeat_18_past_the_end', BAD_CODE, ll257, [0], items=plain[:-1] + [(18, 0)], body=False)
    no_eob = complete_lengths(256) + [0]
    dyn('no_end_of_block_code', BAD_CODE, no_eob, [0], body=False)
    dyn('oversubscribed_lengths', BAD_CODE, [8] * 257, [0], body=False)
    dyn('incomplete_lengths', BAD_CODE, [9] * 257, [0], body=False)
    dyn('incomplete_distances', BAD_CODE, ll257, [2], body=False)
    dyn('oversubscribed_distances', BAD_CODE, ll257, [1, 1, 1], body=False)
    dyn('incomplete_code_length_code', BAD_CODE, ll257, [0], cl_lens=[4] * 12 + [5] * 7, body=False)
    dyn('oversubscribed_code_length_code', BAD_CODE, ll257, [0], cl_lens=[4] * 14 + [5] * 5, body=False)
    # a length symbol under an all-zero distance set, and the unused code of a one-code distance set
    bw = BitWriter().stored(raw[:half])
    blk = dynamic_block(bw, complete_lengths(286), [0], final=1)
    blk.symbol(257)
    bw.bits(0, 16)
    bad('length_under_all_zero_distance_set', bw.finish(raw), BAD_CODE)
    bw = BitWriter().stored(raw[:half])
    blk = dynamic_block(bw, complete_lengths(286), [1], final=1)
    blk.symbol(257)
    bw.bits(0xffff, 16)
    bad('unused_code_of_one_code_distance_set', bw.finish(raw), BAD_CODE)
    for name, stream in (('default', good), ('stored', deflate(raw, 0)), ('fixed', deflate(raw, 6, zlib.Z_FIXED))):
        for q in (1, 2, 3):
            bad(f'cut_{name}_{q}_of_4', stream[:len(stream) * q // 4], SHORT_INPUT)
    bad('cut_inside_the_checksum', good[:-2], SHORT_INPUT)
    bad('empty_input', b'', SHORT_INPUT)
    bad('header_only', good[:2], SHORT_INPUT)
    bad('stream_of_fewer_rows', zlib.compress(raw[:half], 6), SHORT_INPUT)
    bw = BitWriter()
    fixed_block(bw, final=1).literals(raw[:-2]).match(3, 1).end()
    bad('match_overruns_by_one_byte', bw.finish(raw[:-2] + raw[-3:-2] * 3), OVERRUN)
    bad('stream_of_more_rows', zlib.compress(raw + b'\0\0', 6), OVERRUN)
    bw = BitWriter()
    fixed_block(bw).literals(raw).end()
    fixed_block(bw, final=1).literals(b'x').end()
    bad('literal_after_completion', bw.finish(raw + b'x'), OVERRUN)
    bad('stored_block_after_completion', BitWriter().stored(raw).stored(b'yz', final=1).finish(raw + b'yz'), OVERRUN)
    wrong = bytearray(good)
    wrong[-1] ^= 1
    bad('wrong_adler', bytes(wrong), BAD_CHECKSUM)
    flipped = bytearray(deflate(raw, 0))
    flipped[7 + half] ^= 0x10                                # a data byte of a stored block: only the checksum can tell
    bad('stored_data_bit_flipped', bytes(flipped), BAD_CHECKSUM)
    cases.append(_case('trailing_bytes_after_the_checksum', good + b'\x00\xff garbage', sp))
    return cases


@functools.lru_cache(maxsize=None)
def inflate_cases():
    """The battery, good and malformed. The status of every case is what the reference inflater returns for it, and a
    good case's samples are what it inflates to."""
    cases = []
    sp7, sp16, n16 = tc.sparse((7, 77), 0.1, 61), tc.sparse((16, 80), 0.1, 62), tc.noise((16, 80), 63)
    big_sp, big_n = tc.sparse((256, 80), 0.05, 64), tc.noise((256, 80), 65)
    streams = {'stored': dict(level=0), 'fixed': dict(level=6, strategy=zlib.Z_FIXED), 'huffman_only': dict(strategy=zlib.Z_HUFFMAN_ONLY),
               'rle': dict(strategy=zlib.Z_RLE), 'default': dict(), 'level9': dict(level=9), 'wbits9': dict(wbits=9),
               'full_flush': dict(flush_every=8192, flush=zlib.Z_FULL_FLUSH), 'sync_flush': dict(flush_every=8192, flush=zlib.Z_SYNC_FLUSH)}
    for sname, kw in streams.items():
        for aname, a in (('sparse_7x77', sp7), ('noise_16x80', n16)):
            cases.append(_case(f'{sname}_{aname}', deflate(raw_of(a), **kw), a))
    for sname in ('default', 'rle', 'fixed', 'full_flush', 'sync_flush', 'stored'):
        cases.append(_case(f'{sname}_sparse_256x80', deflate(raw_of(big_sp), **streams[sname]), big_sp))
    for sname in ('default', 'huffman_only', 'sync_flush'):
        cases.append(_case(f'{sname}_noise_256x80', deflate(raw_of(big_n), **streams[sname]), big_n))
    zeros = np.zeros((256, 80), np.uint16)
    cases.append(_case('default_zeros_256x80', deflate(raw_of(zeros)), zeros))
    cases.append(_case('default_big_endian_pred2_7x77', deflate(raw_of(sp7, 2, True)), sp7, 2, True))
    cases.append(_case('default_pred2_16x80', deflate(raw_of(sp16, 2, False)), sp16, 2, False))
    cases.append(_case('fixed_big_endian_16x80', deflate(raw_of(n16, 1, True), 6, zlib.Z_FIXED), n16, 1, True))
    cases.append(_case('default_pred2_w300', deflate(raw_of(tc.noise((3, 300), 66), 2)), tc.noise((3, 300), 66), 2))
    for n in (1, 2, 3):
        a = tc.noise((1, n), 66 + n)
        for sname in ('stored', 'fixed', 'default'):
            cases.append(_case(f'{sname}_{n}_samples', deflate(raw_of(a), **streams[sname]), a))
    cases.append(_case('empty_output', zlib.compress(b''), np.zeros((0, 80), np.uint16)))
    cases += _handmade_good()
    cases += _malformed()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        status, a = ref_inflate_segment(c.src, c.rows, c.W, c.predictor, c.big_endian)
        assert status == c.status, (c.name, status, c.status)
        assert c.status != OK or np.array_equal(a, c.expect), c.name
    return tuple(cases)


def first_block_type(stream):
    """BTYPE of the first block of a zlib stream."""
    return stream[2] >> 1 & 3


def write_case_file(path, cases):
    """The binary case file tests/tiff_inflate_host.cpp reads (little-endian): count; per case five int32 (predictor,
    big_endian, rows, W, expected status), int64 src_bytes, the bytes, and for status 0 the rows * W expected samples."""
    with open(path, 'wb') as f:
        f.write(struct.pack('<i', len(cases)))
        for c in cases:
            f.write(struct.pack('<5iq', c.predictor, int(c.big_endian), c.rows, c.W, c.status, len(c.src)))
            f.write(c.src)
            if c.status == OK:
                f.write(np.ascontiguousarray(c.expect, '<u2').tobytes())
