// tiff_inflate.h -- the Deflate strip decoder core of csrc/tiff_inflate.hip, in the manner of
// tiff_decode.h: plain C++ that compiles for the host and for gfx950 alike; the kernel and the stand-alone host program of
// tests/test_tiff_inflate_cpu.py (built with the sanitizers) run these very functions. A strip is a zlib stream (RFC 1950)
// around Deflate blocks (RFC 1951). Everything that can go out of range is decided HERE, before a byte is copied:
//
//   axt_tiff_inflate_next    one step: the 2-byte header, a block header (stored: with LEN / NLEN; dynamic: with the code
//                            lengths and the tables built from them), one literal / length+distance / end-of-block
//                            symbol, or the Adler-32 trailer                                    -> status 1, 2, 3
//   axt_tiff_adler_*         the Adler-32 of the produced bytes, strided over `nlanes` workers  -> status 5
//
// A step hands back ONE copy operation of tiff_decode.h (a literal is a FILL of one byte, a match a FROM_OUTPUT with
// period = distance, a stored block a FROM_INPUT), its ranges already checked against [0, src_bytes) and [0, out_bytes).
// The parse is wave-uniform: on the device the 64 lanes take the same steps and share the copies and the building of the
// lookup tables (lane, nlanes); on the host nlanes = 1.
//
// Unlike the other codecs of tiff_decode.h, inflate does not stop where the output is complete: it goes on to the end of
// the stream (only end-of-block codes and blocks without output may follow; anything that would produce output is status
// 3), aligns, and reads the big-endian Adler-32, the format's only integrity check. Bytes behind the checksum are ignored.
//
// Bits: a 64-bit buffer, least significant bit first, refilled from bytes below src_bytes only. A read of n bits is
// checked against the bits the buffer holds; after a refill fewer than 56 means the input is exhausted, so this IS the
// check against 8 * src_bytes.
//
// Huffman codes: canonical, per set a count per length, the symbols sorted by (length, symbol), and a direct table over
// the first `fast` bits (entry = symbol << 4 | length, 0 = longer than `fast` or no code). A code longer than `fast` bits is
// found by the textbook walk over the counts, one bit a turn; so is the absence of a code in an incomplete set.
#pragma once
#include "tiff_decode.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define AXT_TIFF_LANES_SYNC() __syncthreads()        // the block is one wave: orders its lanes' LDS writes and reads
#else
#define AXT_TIFF_LANES_SYNC() ((void)0)
#endif

enum { AXT_TIFF_BAD_CHECKSUM = 5 };                  // the stream's Adler-32 is not that of the produced bytes
enum { AXT_TIFF_COMP_ADOBE_DEFLATE = 8, AXT_TIFF_COMP_DEFLATE = 32946 };

enum {
    AXT_INF_MAXBITS = 15, AXT_INF_N_LL = 288, AXT_INF_N_D = 32, AXT_INF_N_CL = 19,
    AXT_INF_FAST_LL = 10, AXT_INF_FAST_D = 8, AXT_INF_FAST_CL = 7,
    AXT_INF_WINDOW = 32768, AXT_INF_ADLER_MOD = 65521
};
enum { AXT_INF_KIND_CODES = 0, AXT_INF_KIND_LENS = 1, AXT_INF_KIND_DISTS = 2 };
enum { AXT_INF_PHASE_HEADER = 0, AXT_INF_PHASE_BLOCK = 1, AXT_INF_PHASE_SYMBOL = 2, AXT_INF_PHASE_TRAILER = 3 };

// one canonical code set: what axt_tiff_inflate_build writes and axt_tiff_inflate_symbol reads
struct axt_tiff_inflate_tables {
    uint16_t fast_ll[1 << AXT_INF_FAST_LL], fast_d[1 << AXT_INF_FAST_D], fast_cl[1 << AXT_INF_FAST_CL];
    uint16_t lens[AXT_INF_N_LL + AXT_INF_N_D];       // code lengths: literal/length set first, the distance set behind it
    uint16_t code[AXT_INF_N_LL + AXT_INF_N_D];       // the symbols' codes, while a set is built
    uint16_t sorted_ll[AXT_INF_N_LL], sorted_d[AXT_INF_N_D], sorted_cl[AXT_INF_N_CL + 1];
    uint16_t cnt_ll[16], cnt_d[16], cnt_cl[16];
    uint16_t lens_cl[AXT_INF_N_CL + 1];
};

struct axt_tiff_inflate_state {
    uint64_t hold;        // the next nbits bits of the input, least significant first; zero above them once the input is exhausted
    int nbits;
    int64_t next;         // the next input byte to go into hold
    uint32_t out_pos;     // bytes of output produced
    int phase, final;     // final: the block being read carries BFINAL
    uint32_t adler;       // the trailer's Adler-32, once status is OK and done is set
    int status, done;
};

AXT_TIFF_HD void axt_tiff_inflate_init(axt_tiff_inflate_state &s)
{
    s.hold = 0, s.nbits = 0, s.next = 0;
    s.out_pos = 0;
    s.phase = AXT_INF_PHASE_HEADER, s.final = 0;
    s.adler = 0;
    s.status = AXT_TIFF_OK, s.done = 0;
}

AXT_TIFF_HD void axt_tiff_inflate_finish(axt_tiff_inflate_state &s, int status)
{
    s.status = status;
    s.done = 1;
}

// The step bound. Every step of axt_tiff_inflate_next consumes at least one input bit or ends the segment: the header
// step takes 16 bits, a block header at least 3, a symbol at least the one bit of the shortest code, the trailer 32 --
// and a step that cannot have its bits ends the segment with status 1. The input has 8 * src_bytes bits, so after that
// many steps none is left and the next step ends; the loops inside a step (the code lengths of a dynamic block: at most
// 316; the walk over the code lengths: 15) are bounded by constants. This is what keeps a malformed strip from hanging a wave.
AXT_TIFF_HD int64_t axt_tiff_inflate_max_steps(int64_t src_bytes)
{
    return 8 * src_bytes + 2;
}

// hold filled to more than 56 bits, or to the end of the input. No byte at or above src_bytes is read.
AXT_TIFF_HD void axt_tiff_inflate_refill(const uint8_t *src, int64_t src_bytes, axt_tiff_inflate_state &s)
{
    if (s.next + 8 <= src_bytes) {
        uint64_t w = 0;
        for (int k = 0; k < 8; ++k) w |= (uint64_t)src[s.next + k] << (8 * k);
        s.hold |= w << s.nbits;                      // (bits above the new nbits are input bits that come again: idempotent)
        const int take = (63 - s.nbits) >> 3;
        s.next += take;
        s.nbits += 8 * take;
    } else {
        while (s.nbits <= 56 && s.next < src_bytes) {
            s.hold |= (uint64_t)src[s.next++] << s.nbits;
            s.nbits += 8;
        }
    }
}

AXT_TIFF_HD void axt_tiff_inflate_drop(axt_tiff_inflate_state &s, int n)
{
    s.hold >>= n;
    s.nbits -= n;
}

// n <= 32 bits, or false where the input does not have them
AXT_TIFF_HD bool axt_tiff_inflate_bits(axt_tiff_inflate_state &s, int n, uint32_t &v)
{
    if (n > s.nbits) return false;
    v = (uint32_t)(s.hold & ((1ull << n) - 1));
    axt_tiff_inflate_drop(s, n);
    return true;
}

AXT_TIFF_HD uint32_t axt_tiff_inflate_reverse(uint32_t code, int len)
{
    uint32_t r = 0;
    for (int k = 0; k < len; ++k) r |= (code >> k & 1u) << (len - 1 - k);
    return r;
}

// The tables of one code set from its n code lengths (each 0..15). Shared by the workers: the count of length L and the
// codes of the symbols of length L are worker L's, the fill of the direct table is strided over the symbols. Returns 0,
// or status 2 for a set zlib's inflate refuses: over-subscribed, or incomplete -- except a literal/length or distance
// set of one single 1-bit code, and a distance set without any code (legal as long as no length symbol is met).
AXT_TIFF_HD int axt_tiff_inflate_build(const uint16_t *lens, int n, int kind, uint16_t *cnt, uint16_t *sorted, uint16_t *code,
                                       uint16_t *fast, int fast_bits, uint32_t lane, uint32_t nlanes)
{
    AXT_TIFF_LANES_SYNC();                                                // the lengths are written, the old tables read
    for (uint32_t L = lane; L <= AXT_INF_MAXBITS; L += nlanes) {
        int c = 0;
        for (int sy = 0; sy < n; ++sy) c += lens[sy] == L;
        cnt[L] = (uint16_t)c;
    }
    for (uint32_t k = lane; k < (1u << fast_bits); k += nlanes) fast[k] = 0;
    AXT_TIFF_LANES_SYNC();
    int left = 1, max = 0;
    for (int L = 1; L <= AXT_INF_MAXBITS; ++L) {
        left = (left << 1) - (int)cnt[L];
        if (left < 0) return AXT_TIFF_BAD_CODE;                           // over-subscribed
        if (cnt[L]) max = L;
    }
    if (max == 0) return kind == AXT_INF_KIND_DISTS ? AXT_TIFF_OK : AXT_TIFF_BAD_CODE;
    if (left > 0 && (kind == AXT_INF_KIND_CODES || max != 1)) return AXT_TIFF_BAD_CODE;      // incomplete
    for (uint32_t L = 1 + lane; L <= AXT_INF_MAXBITS; L += nlanes) {
        uint32_t first = 0, at = 0;                                       // the first code of length L, its place in `sorted`
        for (uint32_t l = 1; l < L; ++l) first = (first + cnt[l]) << 1, at += cnt[l];
        for (int sy = 0; sy < n; ++sy)
            if (lens[sy] == L) {
                sorted[at++] = (uint16_t)sy;
                code[sy] = (uint16_t)first++;
            }
    }
    AXT_TIFF_LANES_SYNC();
    for (uint32_t sy = lane; sy < (uint32_t)n; sy += nlanes) {
        const int L = lens[sy];
        if (L >= 1 && L <= fast_bits)
            for (uint32_t k = axt_tiff_inflate_reverse(code[sy], L); k < (1u << fast_bits); k += 1u << L)
                fast[k] = (uint16_t)(sy << 4 | L);
    }
    AXT_TIFF_LANES_SYNC();
    return AXT_TIFF_OK;
}

// The symbol whose code stands at the front of hold: 0 with sym and len set (nothing dropped yet), status 1 where the
// input ends inside the code, status 2 where 15 bits match no code of an incomplete set.
AXT_TIFF_HD int axt_tiff_inflate_symbol(const axt_tiff_inflate_state &s, const uint16_t *cnt, const uint16_t *sorted,
                                        const uint16_t *fast, int fast_bits, int &sym, int &len)
{
    const uint32_t e = fast[s.hold & ((1u << fast_bits) - 1)];
    if (e) {
        sym = (int)(e >> 4), len = (int)(e & 15);
        return len <= s.nbits ? AXT_TIFF_OK : AXT_TIFF_SHORT_INPUT;
    }
    int code = 0, first = 0, index = 0;
    for (int L = 1; L <= AXT_INF_MAXBITS; ++L) {
        if (L > s.nbits) return AXT_TIFF_SHORT_INPUT;
        code |= (int)(s.hold >> (L - 1) & 1);
        const int count = cnt[L];
        if (code - count < first) {
            sym = sorted[index + (code - first)], len = L;
            return AXT_TIFF_OK;
        }
        index += count, first += count;
        first <<= 1, code <<= 1;
    }
    return AXT_TIFF_BAD_CODE;
}

// the order in which a dynamic block lists the lengths of the code-length code: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15,
// five bits each from the least significant end
AXT_TIFF_HD int axt_tiff_inflate_cl_order(int k)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40
        | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((k < 12 ? lo >> (5 * k) : hi >> (5 * (k - 12))) & 31);
}

// The header of a dynamic block behind BTYPE: HLIT, HDIST, HCLEN, the code-length code, the lengths with the repeats 16 /
// 17 / 18, and the two sets' tables. n_ll: where the distance lengths start in t.lens.
AXT_TIFF_HD int axt_tiff_inflate_dynamic(const uint8_t *src, int64_t src_bytes, axt_tiff_inflate_state &s, axt_tiff_inflate_tables &t,
                                         uint32_t lane, uint32_t nlanes)
{
    uint32_t v;
    axt_tiff_inflate_refill(src, src_bytes, s);
    if (!axt_tiff_inflate_bits(s, 14, v)) return AXT_TIFF_SHORT_INPUT;
    const int n_ll = (int)(v & 31) + 257, n_d = (int)(v >> 5 & 31) + 1, n_cl = (int)(v >> 10 & 15) + 4;
    if (n_ll > 286 || n_d > 30) return AXT_TIFF_BAD_CODE;
    for (int k = 0; k < AXT_INF_N_CL; ++k) t.lens_cl[k] = 0;
    for (int k = 0; k < n_cl; ++k) {
        axt_tiff_inflate_refill(src, src_bytes, s);
        if (!axt_tiff_inflate_bits(s, 3, v)) return AXT_TIFF_SHORT_INPUT;
        t.lens_cl[axt_tiff_inflate_cl_order(k)] = (uint16_t)v;
    }
    int rc = axt_tiff_inflate_build(t.lens_cl, AXT_INF_N_CL, AXT_INF_KIND_CODES, t.cnt_cl, t.sorted_cl, t.code, t.fast_cl,
                                    AXT_INF_FAST_CL, lane, nlanes);
    if (rc != AXT_TIFF_OK) return rc;
    int have = 0;
    while (have < n_ll + n_d) {
        int sym, len;
        axt_tiff_inflate_refill(src, src_bytes, s);
        rc = axt_tiff_inflate_symbol(s, t.cnt_cl, t.sorted_cl, t.fast_cl, AXT_INF_FAST_CL, sym, len);
        if (rc != AXT_TIFF_OK) return rc;
        axt_tiff_inflate_drop(s, len);
        if (sym < 16) {
            t.lens[have++] = (uint16_t)sym;
            continue;
        }
        int value = 0, extra, base;
        if (sym == 16) {
            if (have == 0) return AXT_TIFF_BAD_CODE;                      // nothing to repeat
            value = t.lens[have - 1], extra = 2, base = 3;
        } else if (sym == 17) {
            extra = 3, base = 3;
        } else {
            extra = 7, base = 11;
        }
        if (!axt_tiff_inflate_bits(s, extra, v)) return AXT_TIFF_SHORT_INPUT;
        const int rep = base + (int)v;
        if (rep > n_ll + n_d - have) return AXT_TIFF_BAD_CODE;            // the repeat runs past HLIT + HDIST
        for (int k = 0; k < rep; ++k) t.lens[have++] = (uint16_t)value;
    }
    if (t.lens[256] == 0) return AXT_TIFF_BAD_CODE;                       // no end-of-block code
    rc = axt_tiff_inflate_build(t.lens, n_ll, AXT_INF_KIND_LENS, t.cnt_ll, t.sorted_ll, t.code, t.fast_ll, AXT_INF_FAST_LL, lane, nlanes);
    if (rc != AXT_TIFF_OK) return rc;
    return axt_tiff_inflate_build(t.lens + n_ll, n_d, AXT_INF_KIND_DISTS, t.cnt_d, t.sorted_d, t.code + n_ll, t.fast_d, AXT_INF_FAST_D,
                                  lane, nlanes);
}

// the fixed code of RFC 1951 3.2.6, symbols 286 / 287 and distances 30 / 31 included (met in the data they are status 2)
AXT_TIFF_HD int axt_tiff_inflate_fixed(axt_tiff_inflate_tables &t, uint32_t lane, uint32_t nlanes)
{
    AXT_TIFF_LANES_SYNC();
    for (uint32_t sy = lane; sy < AXT_INF_N_LL + AXT_INF_N_D; sy += nlanes)
        t.lens[sy] = (uint16_t)(sy < 144 ? 8 : sy < 256 ? 9 : sy < 280 ? 7 : sy < 288 ? 8 : 5);
    int rc = axt_tiff_inflate_build(t.lens, AXT_INF_N_LL, AXT_INF_KIND_LENS, t.cnt_ll, t.sorted_ll, t.code, t.fast_ll, AXT_INF_FAST_LL,
                                    lane, nlanes);
    if (rc != AXT_TIFF_OK) return rc;
    return axt_tiff_inflate_build(t.lens + AXT_INF_N_LL, AXT_INF_N_D, AXT_INF_KIND_DISTS, t.cnt_d, t.sorted_d, t.code + AXT_INF_N_LL,
                                  t.fast_d, AXT_INF_FAST_D, lane, nlanes);
}

// One step. op: the copy the step stands for (kind NONE where it has none), checked.
AXT_TIFF_HD void axt_tiff_inflate_next(const uint8_t *src, int64_t src_bytes, uint32_t out_bytes, axt_tiff_inflate_state &s,
                                       axt_tiff_inflate_tables &t, axt_tiff_op &op, uint32_t lane, uint32_t nlanes)
{
    op.kind = AXT_TIFF_OP_NONE;
    op.dst = s.out_pos, op.len = 0, op.src = 0, op.period = 1;
    uint32_t v;
    if (s.nbits < 48) axt_tiff_inflate_refill(src, src_bytes, s);         // (a symbol step reads at most 15 + 5 + 15 + 13 bits)
    if (s.phase == AXT_INF_PHASE_HEADER) {
        if (!axt_tiff_inflate_bits(s, 16, v)) return axt_tiff_inflate_finish(s, AXT_TIFF_SHORT_INPUT);
        const uint32_t cmf = v & 255, flg = v >> 8;
        if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (cmf * 256 + flg) % 31 != 0 || (flg & 32))
            return axt_tiff_inflate_finish(s, AXT_TIFF_BAD_CODE);
        s.phase = AXT_INF_PHASE_BLOCK;
        return;
    }
    if (s.phase == AXT_INF_PHASE_BLOCK) {
        if (!axt_tiff_inflate_bits(s, 3, v)) return axt_tiff_inflate_finish(s, AXT_TIFF_SHORT_INPUT);
        s.final = (int)(v & 1);
        const int btype = (int)(v >> 1);
        if (btype == 3) return axt_tiff_inflate_finish(s, AXT_TIFF_BAD_CODE);
        if (btype == 0) {
            axt_tiff_inflate_drop(s, s.nbits & 7);
            axt_tiff_inflate_refill(src, src_bytes, s);
            if (!axt_tiff_inflate_bits(s, 32, v)) return axt_tiff_inflate_finish(s, AXT_TIFF_SHORT_INPUT);
            const uint32_t len = v & 0xffff;
            if (len != (~v >> 16 & 0xffff)) return axt_tiff_inflate_finish(s, AXT_TIFF_BAD_CODE);
            const int64_t at = s.next - (s.nbits >> 3);                   // (hold has whole bytes only: aligned above)
            if ((int64_t)len > src_bytes - at) return axt_tiff_inflate_finish(s, AXT_TIFF_SHORT_INPUT);
            if (len > out_bytes - s.out_pos) return axt_tiff_inflate_finish(s, AXT_TIFF_OVERRUN);
            if (len) op.kind = AXT_TIFF_OP_FROM_INPUT, op.src = at, op.len = len;
            s.hold = 0, s.nbits = 0, s.next = at + len;
            s.out_pos += len;
            s.phase = s.final ? AXT_INF_PHASE_TRAILER : AXT_INF_PHASE_BLOCK;
            return;
        }
        const int rc = btype == 1 ? axt_tiff_inflate_fixed(t, lane, nlanes) : axt_tiff_inflate_dynamic(src, src_bytes, s, t, lane, nlanes);
        if (rc != AXT_TIFF_OK) return axt_tiff_inflate_finish(s, rc);
        s.phase = AXT_INF_PHASE_SYMBOL;
        return;
    }
    if (s.phase == AXT_INF_PHASE_SYMBOL) {
        int sym, len;
        int rc = axt_tiff_inflate_symbol(s, t.cnt_ll, t.sorted_ll, t.fast_ll, AXT_INF_FAST_LL, sym, len);
        if (rc != AXT_TIFF_OK) return axt_tiff_inflate_finish(s, rc);
        axt_tiff_inflate_drop(s, len);
        if (sym == 256) {
            s.phase = s.final ? AXT_INF_PHASE_TRAILER : AXT_INF_PHASE_BLOCK;
            return;
        }
        if (sym < 256) {
            if (s.out_pos >= out_bytes) return axt_tiff_inflate_finish(s, AXT_TIFF_OVERRUN);
            op.kind = AXT_TIFF_OP_FILL, op.src = sym, op.len = 1;
            s.out_pos += 1;
            return;
        }
        if (sym > 285) return axt_tiff_inflate_finish(s, AXT_TIFF_BAD_CODE);
        // length 3..258: codes 257..264 stand for 3..10, then four codes per extra-bit count 1..5, and 285 for 258
        uint32_t length = 258;
        if (sym < 265) {
            length = (uint32_t)(sym - 257) + 3;
        } else if (sym < 285) {
            const int e = (sym - 261) >> 2;
            if (!axt_tiff_inflate_bits(s, e, v)) return axt_tiff_inflate_finish(s, AXT_TIFF_SHORT_INPUT);
            length = 3 + ((4u + (uint32_t)((sym - 261) & 3)) << e) + v;
        }
        rc = axt_tiff_inflate_symbol(s, t.cnt_d, t.sorted_d, t.fast_d, AXT_INF_FAST_D, sym, len);
        if (rc != AXT_TIFF_OK) return axt_tiff_inflate_finish(s, rc);
        axt_tiff_inflate_drop(s, len);
        if (sym > 29) return axt_tiff_inflate_finish(s, AXT_TIFF_BAD_CODE);
        // distance 1..32768: codes 0..3 stand for 1..4, then two codes per extra-bit count 1..13
        uint32_t dist = (uint32_t)sym + 1;
        if (sym >= 4) {
            const int e = (sym >> 1) - 1;
            if (!axt_tiff_inflate_bits(s, e, v)) return axt_tiff_inflate_finish(s, AXT_TIFF_SHORT_INPUT);
            dist = 1 + ((2u + (uint32_t)(sym & 1)) << e) + v;
        }
        if (dist > s.out_pos) return axt_tiff_inflate_finish(s, AXT_TIFF_BAD_CODE);           // before the strip's first byte
        if (length > out_bytes - s.out_pos) return axt_tiff_inflate_finish(s, AXT_TIFF_OVERRUN);
        op.kind = AXT_TIFF_OP_FROM_OUTPUT, op.src = (int64_t)(s.out_pos - dist), op.len = length, op.period = dist;
        s.out_pos += length;
        return;
    }
    // the trailer: the Adler-32 of the produced bytes, most significant byte first, at the next byte boundary
    if (s.out_pos < out_bytes) return axt_tiff_inflate_finish(s, AXT_TIFF_SHORT_INPUT);       // the stream ends before the rows do
    axt_tiff_inflate_drop(s, s.nbits & 7);
    axt_tiff_inflate_refill(src, src_bytes, s);
    if (!axt_tiff_inflate_bits(s, 32, v)) return axt_tiff_inflate_finish(s, AXT_TIFF_SHORT_INPUT);
    s.adler = (v & 0xff) << 24 | (v & 0xff00) << 8 | (v >> 8 & 0xff00) | v >> 24;
    axt_tiff_inflate_finish(s, AXT_TIFF_OK);
}

// Adler-32 over n bytes, worker `lane` of `nlanes` taking every nlanes-th: a = sum of p[i], b = sum of (n - i) * p[i], both
// modulo 65521; the workers' sums add up (modulo 65521) to the arguments of axt_tiff_adler_value.
AXT_TIFF_HD void axt_tiff_adler_partial(const uint8_t *p, uint32_t n, uint32_t lane, uint32_t nlanes, uint32_t &a, uint32_t &b)
{
    uint64_t sa = 0, sb = 0;
    uint32_t turn = 0;
    for (uint32_t i = lane; i < n; i += nlanes) {
        sa += p[i];
        sb += (uint64_t)(n - i) * p[i];                                   // (< 2^40 a term)
        if ((++turn & 4095) == 0) sb %= AXT_INF_ADLER_MOD;
        if (n - i <= nlanes) break;                                       // (i + nlanes must not wrap)
    }
    a = (uint32_t)(sa % AXT_INF_ADLER_MOD), b = (uint32_t)(sb % AXT_INF_ADLER_MOD);
}

// s1 = 1 + sum p[i], s2 = sum over i of s1 after byte i = n + sum (n - i) p[i]
AXT_TIFF_HD uint32_t axt_tiff_adler_value(uint64_t a, uint64_t b, uint32_t n)
{
    const uint32_t s1 = (uint32_t)((1 + a) % AXT_INF_ADLER_MOD), s2 = (uint32_t)((n % AXT_INF_ADLER_MOD + b) % AXT_INF_ADLER_MOD);
    return s2 << 16 | s1;
}

// Whole segment on one worker: what the host program runs, and the statement of what the kernel computes. The bytes are
// inflated in place into `out`, checked against the trailer, then swapped and accumulated row by row (the uncompressed
// route of axt_tiff_decode_segment_serial, in place). steps: where not null, receives the number of steps taken.
inline int axt_tiff_inflate_segment_serial(const uint8_t *src, int64_t src_bytes, int rows, int W, int predictor, int big_endian,
                                           uint16_t *out, axt_tiff_inflate_tables &t, int64_t *steps = nullptr)
{
    const uint32_t out_bytes = (uint32_t)rows * (uint32_t)W * 2u;
    uint8_t *bytes = reinterpret_cast<uint8_t *>(out);
    axt_tiff_inflate_state s;
    axt_tiff_inflate_init(s);
    axt_tiff_op op;
    const int64_t bound = axt_tiff_inflate_max_steps(src_bytes);
    int64_t it = 0;
    for (; it < bound && !s.done; ++it) {
        axt_tiff_inflate_next(src, src_bytes, out_bytes, s, t, op, 0, 1);
        axt_tiff_apply(op, src, bytes, 0, 1);
    }
    if (steps) *steps = it;
    if (!s.done) axt_tiff_inflate_finish(s, AXT_TIFF_SHORT_INPUT);
    if (s.status != AXT_TIFF_OK) return s.status;
    uint32_t a, b;
    axt_tiff_adler_partial(bytes, out_bytes, 0, 1, a, b);
    if (axt_tiff_adler_value(a, b, out_bytes) != s.adler) return AXT_TIFF_BAD_CHECKSUM;
    return axt_tiff_decode_segment_serial(bytes, out_bytes, rows, W, AXT_TIFF_COMP_NONE, predictor, big_endian, out, nullptr, nullptr);
}
