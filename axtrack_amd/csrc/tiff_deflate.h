// tiff_deflate.h -- the Deflate strip ENCODER core of csrc/tiff_deflate.hip ("TIFF output"), in the manner
// of tiff_inflate.h: plain C++ that compiles for the host and for gfx950 alike; the kernel and the stand-alone host
// program of tests/test_tiff_deflate_cpu.py (built with the sanitizers) run these very functions, the kernel with 64
// workers (lane, nlanes = 64), the host with one (0, 1). The stream is the same byte for byte: every step below is a
// function of the strip's bytes alone, and what the workers share goes through the work area between two barriers.
//
// A strip is rows * W uint16 samples, stored little-endian with the predictor applied on load (axt_tiff_deflate_byte:
// the difference to the left neighbour is read from the input, modulo 2^16). It becomes one zlib stream (RFC 1950 / 1951):
//
//   header     0x78 0x01: CM 8, CINFO 7, no preset dictionary, FLEVEL 0, check bits
//   parse      positions are taken in batches of 64 from `base` on. Position p = base + i with p + 3 <= n has two
//              candidates: (a) the position the hash table held for its three bytes BEFORE the batch (the table keeps the
//              highest position seen per hash; dropped where it lies more than 32768 behind), (b) p - 2, the previous
//              sample. Each is measured byte by byte up to min(258, n - p); the longer wins, (b) on a tie. A match
//              counts with length >= 4, or length 3 and distance <= 4096. Then every position of the batch with three
//              bytes is put into the table (maximum of position + 1), and the greedy cover is walked from i = 0: a
//              counting match at i becomes a token and i advances by its length, anything else is a literal. The next
//              batch begins where the cover ended (inside a match that runs past the batch nothing is hashed).
//   blocks     tokens are buffered (AXT_DEF_TOKENS). A block ends when another batch might not fit, or with the strip.
//              Its exact size in bits is computed as stored, fixed and dynamic; the smallest is written, stored before
//              fixed before dynamic on a tie. Stored blocks that follow one another are written as ONE run of pieces of
//              at most 65535 bytes (the run's header is charged to its first block, a further piece to the block that
//              crosses into it). Should the stream still end up longer than the all-stored stream,
//              axt_tiff_deflate_bound, it is written again all stored: the bound holds for every input.
//   codes      length-limited by construction and Kraft-sum repair: a used symbol's length is maxbits - floor(log2(1 +
//              f * (2^maxbits - used) / total)) -- one unit of the 2^maxbits Kraft budget is set aside per used symbol,
//              so no length exceeds maxbits and the sum never exceeds the budget --, then the symbols are taken by
//              falling frequency (symbol number on ties) and each is shortened while its doubled share still fits the
//              slack. The slack ends at zero: the set is complete. One used symbol gets the single 1-bit code (the
//              code-length code a second 1-bit code: zlib refuses it incomplete), none an all-zero set.
//   bits       every worker encodes one token of 64, an exclusive scan of the bit lengths places them, and the codes are
//              ORed into a staging area that is flushed to the slot in whole bytes with plain stores.
//   trailer    Adler-32 of the stored bytes, position-weighted and strided over the workers.
//
// Bounds: a batch advances `base` by at least min(64, n - base), so a strip takes at most n / 64 + 1 batches
// (axt_tiff_deflate_max_batches), n = 2 * rows * W; a block holds at least one batch; every loop inside a batch or a block
// is bounded by a constant (64 positions, 258 bytes of a match, AXT_DEF_TOKENS tokens, 320 symbols); the copies of stored
// pieces and the checksum pass n bytes once. No byte outside [0, n) of the input is read, none outside [0, cap) of the
// slot written: a stream that does not fit is counted, not written, and ends as status 3.
#pragma once
#include "tiff_inflate.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define AXT_DEF_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define AXT_DEF_ATOMIC_OR(p, v) atomicOr((p), (v))
#define AXT_DEF_ATOMIC_MAX(p, v) atomicMax((p), (v))
#else
#define AXT_DEF_ATOMIC_ADD(p, v) (*(p) += (v))
#define AXT_DEF_ATOMIC_OR(p, v) (*(p) |= (v))
#define AXT_DEF_ATOMIC_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#endif

enum {
    AXT_DEF_BATCH = 64, AXT_DEF_HASH_BITS = 12, AXT_DEF_TOKENS = 4096, AXT_DEF_STAGE_WORDS = 512,
    AXT_DEF_MIN_MATCH = 3, AXT_DEF_MAX_MATCH = 258, AXT_DEF_MAX_DIST = 32768, AXT_DEF_FAR = 4096,
    AXT_DEF_N_LL = 286, AXT_DEF_N_D = 30, AXT_DEF_N_CL = 19, AXT_DEF_D0 = 288,      // distance symbols start at D0 in the tables
    AXT_DEF_SYMS = 320, AXT_DEF_STORED_MAX = 65535,
    AXT_DEF_TOKEN_BITS = 48                                                         // 15 + 5 + 15 + 13
};
enum { AXT_DEF_STORED = 0, AXT_DEF_FIXED = 1, AXT_DEF_DYNAMIC = 2 };

// what the workers share; on the device it lives in LDS
struct axt_tiff_deflate_work {
    uint32_t head[1 << AXT_DEF_HASH_BITS];           // per hash: highest position seen + 1, 0 = none
    uint32_t tok[AXT_DEF_TOKENS];                    // literal: the byte; match: 1 << 23 | (length - 3) << 15 | (distance - 1)
    uint32_t stage[AXT_DEF_STAGE_WORDS];             // the bits not yet flushed, least significant first
    uint32_t freq[AXT_DEF_SYMS], freq_cl[AXT_DEF_N_CL + 1];
    uint32_t red[AXT_DEF_BATCH];
    uint16_t len[AXT_DEF_SYMS], code[AXT_DEF_SYMS];  // code: bit-reversed, ready to be ORed in
    uint16_t len_cl[AXT_DEF_N_CL + 1], code_cl[AXT_DEF_N_CL + 1];
    uint16_t order[AXT_DEF_SYMS];                    // the used symbols of the set being built, by falling frequency
    uint16_t items[AXT_DEF_SYMS];                    // the code-length symbols of a dynamic header: symbol | extra value << 5
    uint16_t mlen[AXT_DEF_BATCH], mdist[AXT_DEF_BATCH];      // a batch's matches: length (0 = literal), distance - 1
    uint8_t mlit[AXT_DEF_BATCH];
};

struct axt_tiff_deflate_state {
    uint8_t *out;
    int64_t cap, out_pos;     // out_pos: bytes flushed, or that would have been
    uint32_t bitpos;          // bits standing in work.stage
    int overflow;             // something did not fit below cap and was left unwritten
};

// raw + 5 * max(1, ceil(raw / 65535)) + 6: the all-stored stream
AXT_TIFF_HD int64_t axt_tiff_deflate_bound_bytes(int64_t raw)
{
    int64_t pieces = (raw + AXT_DEF_STORED_MAX - 1) / AXT_DEF_STORED_MAX;
    if (pieces < 1) pieces = 1;
    return raw + 5 * pieces + 6;
}

AXT_TIFF_HD int64_t axt_tiff_deflate_max_batches(int64_t n)
{
    return n / AXT_DEF_BATCH + 1;
}

// byte p of the strip as stored
AXT_TIFF_HD uint32_t axt_tiff_deflate_byte(const uint16_t *in, uint32_t W, int predictor, uint32_t p)
{
    const uint32_t s = p >> 1;
    uint32_t v = in[s];
    if (predictor == 2 && s % W != 0) v = (v - in[s - 1]) & 0xffffu;
    return p & 1 ? v >> 8 : v & 255u;
}

// the sum of every worker's v
AXT_TIFF_HD uint32_t axt_def_sum(uint32_t v, uint32_t *red, uint32_t lane, uint32_t nlanes)
{
    AXT_TIFF_LANES_SYNC();
    red[lane] = v;
    AXT_TIFF_LANES_SYNC();
    uint32_t s = 0;
    for (uint32_t k = 0; k < nlanes; ++k) s += red[k];
    return s;
}

// the sum of the workers' v below this one, and of all
AXT_TIFF_HD uint32_t axt_def_scan(uint32_t v, uint32_t *red, uint32_t lane, uint32_t nlanes, uint32_t &total)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)red, (void)nlanes;
    uint32_t s = v;
    for (int d = 1; d < AXT_DEF_BATCH; d <<= 1) {
        const uint32_t up = __shfl_up(s, d, AXT_DEF_BATCH);
        if ((int)lane >= d) s += up;
    }
    total = __shfl(s, AXT_DEF_BATCH - 1, AXT_DEF_BATCH);
    return s - v;
#else
    (void)red, (void)lane, (void)nlanes;
    total = v;
    return 0;
#endif
}

// ------------------------------------------------------------------------------------------------ bits
// nbits <= 48 bits of v at bit `at` of the staging area
AXT_TIFF_HD void axt_def_or(uint32_t *stage, uint32_t at, uint64_t v, uint32_t nbits)
{
    if (nbits == 0) return;
    const uint32_t w = at >> 5, sh = at & 31;
    const uint32_t w0 = (uint32_t)(v << sh);
    const uint64_t rest = sh ? v >> (32 - sh) : v >> 32;
    if (w0) AXT_DEF_ATOMIC_OR(&stage[w], w0);
    if ((uint32_t)rest) AXT_DEF_ATOMIC_OR(&stage[w + 1], (uint32_t)rest);
    if (rest >> 32) AXT_DEF_ATOMIC_OR(&stage[w + 2], (uint32_t)(rest >> 32));
}

// The whole bytes of the staging area go to the slot (with `all`: the last partial byte too, zero-padded); the bits
// behind them move to the front.
AXT_TIFF_HD void axt_def_flush(axt_tiff_deflate_work &wk, axt_tiff_deflate_state &st, int all, uint32_t lane, uint32_t nlanes)
{
    AXT_TIFF_LANES_SYNC();
    const uint32_t nbytes = all ? (st.bitpos + 7) >> 3 : st.bitpos >> 3;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(wk.stage);
    const uint32_t tail = (st.bitpos & 7) && !all ? bytes[nbytes] : 0;
    if (st.out_pos + (int64_t)nbytes <= st.cap) {
        for (uint32_t i = lane; i < nbytes; i += nlanes) st.out[st.out_pos + i] = bytes[i];
    } else {
        st.overflow = 1;
    }
    AXT_TIFF_LANES_SYNC();
    for (uint32_t w = lane; w <= nbytes / 4 + 1 && w < AXT_DEF_STAGE_WORDS; w += nlanes) wk.stage[w] = w == 0 ? tail : 0;
    AXT_TIFF_LANES_SYNC();
    st.out_pos += nbytes;
    st.bitpos = all ? 0 : st.bitpos & 7;
}

// nbits <= 32 bits of v behind the bits standing; every worker calls it, one writes
AXT_TIFF_HD void axt_def_put(axt_tiff_deflate_work &wk, axt_tiff_deflate_state &st, uint32_t v, uint32_t nbits, uint32_t lane,
                             uint32_t nlanes)
{
    if (st.bitpos + 64 > 32 * (AXT_DEF_STAGE_WORDS - 3)) axt_def_flush(wk, st, 0, lane, nlanes);
    if (lane == 0) axt_def_or(wk.stage, st.bitpos, v, nbits);
    st.bitpos += nbits;
}

// bytes [from, to) of the strip as stored pieces of one run; `final`: the last piece carries BFINAL
AXT_TIFF_HD void axt_def_stored(const uint16_t *in, uint32_t W, int predictor, uint32_t from, uint32_t to, int final,
                                axt_tiff_deflate_work &wk, axt_tiff_deflate_state &st, uint32_t lane, uint32_t nlanes)
{
    do {
        const uint32_t len = to - from < AXT_DEF_STORED_MAX ? to - from : AXT_DEF_STORED_MAX;
        axt_def_put(wk, st, final && from + len == to ? 1u : 0u, 3, lane, nlanes);
        st.bitpos = (st.bitpos + 7) & ~7u;
        axt_def_put(wk, st, len | (~len & 0xffffu) << 16, 32, lane, nlanes);
        axt_def_flush(wk, st, 1, lane, nlanes);
        if (st.out_pos + (int64_t)len <= st.cap) {
            for (uint32_t i = lane; i < len; i += nlanes) st.out[st.out_pos + i] = (uint8_t)axt_tiff_deflate_byte(in, W, predictor, from + i);
        } else {
            st.overflow = 1;
        }
        st.out_pos += len;
        from += len;
    } while (from < to);
}

// pieces a stored run of x bytes takes
AXT_TIFF_HD uint32_t axt_def_pieces(uint32_t x)
{
    return x == 0 ? 1u : (x + AXT_DEF_STORED_MAX - 1) / AXT_DEF_STORED_MAX;
}

// ------------------------------------------------------------------------------------------------ symbols
// length 3..258 -> symbol 257..285, extra bits and their value
AXT_TIFF_HD void axt_def_length_symbol(uint32_t length, uint32_t &sym, uint32_t &ebits, uint32_t &evalue)
{
    const uint32_t l = length - 3;
    if (length == 258) {
        sym = 285, ebits = 0, evalue = 0;
    } else if (l < 8) {
        sym = 257 + l, ebits = 0, evalue = 0;
    } else {
        ebits = (uint32_t)(31 - __builtin_clz(l)) - 2;
        sym = 261 + 4 * ebits + (l >> ebits & 3);
        evalue = l & ((1u << ebits) - 1);
    }
}

// distance 1..32768 -> symbol 0..29
AXT_TIFF_HD void axt_def_dist_symbol(uint32_t dist, uint32_t &sym, uint32_t &ebits, uint32_t &evalue)
{
    const uint32_t d = dist - 1;
    if (d < 4) {
        sym = d, ebits = 0, evalue = 0;
    } else {
        ebits = (uint32_t)(31 - __builtin_clz(d)) - 1;
        sym = 2 * ebits + 2 + (d >> ebits & 1);
        evalue = d & ((1u << ebits) - 1);
    }
}

AXT_TIFF_HD uint32_t axt_def_length_extra(uint32_t sym)      // symbol 257..285
{
    return sym < 265 || sym == 285 ? 0u : (sym - 261) >> 2;
}

AXT_TIFF_HD uint32_t axt_def_dist_extra(uint32_t sym)        // symbol 0..29
{
    return sym < 4 ? 0u : (sym >> 1) - 1;
}

AXT_TIFF_HD uint32_t axt_def_fixed_len(uint32_t sym)
{
    return sym < 144 ? 8u : sym < 256 ? 9u : sym < 280 ? 7u : 8u;
}

AXT_TIFF_HD uint32_t axt_def_fixed_code(uint32_t sym)
{
    return sym < 144 ? 0x30 + sym : sym < 256 ? 0x190 + (sym - 144) : sym < 280 ? sym - 256 : 0xc0 + (sym - 280);
}

// The code lengths of n symbols from their frequencies f, none above maxbits, the set complete (header comment,
// "codes"). len, order: n entries each. second: a lone used symbol gets a partner, so that the set is complete.
AXT_TIFF_HD void axt_def_lengths(const uint32_t *f, uint32_t n, uint32_t maxbits, int second, uint16_t *len, uint16_t *order,
                                 uint32_t lane, uint32_t nlanes)
{
    AXT_TIFF_LANES_SYNC();                                                // the frequencies are complete
    uint32_t used = 0, only = 0;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (f[i]) ++used, total += f[i], only = i;
    if (used <= 1) {
        for (uint32_t i = lane; i < n; i += nlanes)
            len[i] = (uint16_t)((used == 1 && (i == only || (second && i == (only == 0 ? 1u : 0u)))) ? 1 : 0);
        AXT_TIFF_LANES_SYNC();
        return;
    }
    const uint64_t budget = (1u << maxbits) - used;
    for (uint32_t i = lane; i < n; i += nlanes) {
        const uint32_t fi = f[i];
        if (!fi) {
            len[i] = 0;
            continue;
        }
        const uint64_t share = 1 + fi * budget / total;                   // (< 2^maxbits: used >= 2)
        len[i] = (uint16_t)(maxbits - (uint32_t)(63 - __builtin_clzll(share)));
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) rank += f[j] > fi || (f[j] == fi && j < i);
        order[rank] = (uint16_t)i;
    }
    AXT_TIFF_LANES_SYNC();
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (len[i]) kraft += 1u << (maxbits - len[i]);
    uint32_t slack = (1u << maxbits) - kraft;
    for (uint32_t r = 0; r < used && slack; ++r) {                        // the same walk on every worker; one writes
        const uint32_t i = order[r];
        uint32_t l = len[i];
        while (l > 1 && (1u << (maxbits - l)) <= slack) slack -= 1u << (maxbits - l), --l;
        if (lane == 0) len[i] = (uint16_t)l;
    }
    AXT_TIFF_LANES_SYNC();
}

// canonical codes (RFC 1951 3.2.2) of n lengths, bit-reversed: a symbol's code is the codes of all shorter symbols
// scaled to its length, plus the symbols of its own length before it
AXT_TIFF_HD void axt_def_codes(const uint16_t *len, uint32_t n, uint16_t *code, uint32_t lane, uint32_t nlanes)
{
    for (uint32_t i = lane; i < n; i += nlanes) {
        const uint32_t l = len[i];
        uint32_t c = 0;
        for (uint32_t j = 0; j < n && l; ++j) {
            const uint32_t lj = len[j];
            if (lj && lj < l) c += 1u << (l - lj);
            else if (lj == l && j < i) ++c;
        }
        code[i] = (uint16_t)axt_tiff_inflate_reverse(c, (int)l);
    }
    AXT_TIFF_LANES_SYNC();
}

// a token's bits, least significant first, from the tables in wk
AXT_TIFF_HD uint64_t axt_def_token_bits(const axt_tiff_deflate_work &wk, uint32_t t, uint32_t &nbits)
{
    if (!(t >> 23)) {
        nbits = wk.len[t];
        return wk.code[t];
    }
    uint32_t ls, le, lv, ds, de, dv;
    axt_def_length_symbol((t >> 15 & 255) + 3, ls, le, lv);
    axt_def_dist_symbol((t & 32767) + 1, ds, de, dv);
    uint64_t v = wk.code[ls];
    uint32_t at = wk.len[ls];
    v |= (uint64_t)lv << at, at += le;
    v |= (uint64_t)wk.code[AXT_DEF_D0 + ds] << at, at += wk.len[AXT_DEF_D0 + ds];
    v |= (uint64_t)dv << at, at += de;
    nbits = at;
    return v;
}

// ------------------------------------------------------------------------------------------------ the parse
AXT_TIFF_HD uint32_t axt_def_hash(uint32_t b0, uint32_t b1, uint32_t b2)
{
    return ((b0 | b1 << 8 | b2 << 16) * 0x9e3779b1u) >> (32 - AXT_DEF_HASH_BITS);
}

// bytes that agree from positions c < p on, at most `max`
AXT_TIFF_HD uint32_t axt_def_match_length(const uint16_t *in, uint32_t W, int predictor, uint32_t c, uint32_t p, uint32_t max)
{
    uint32_t k = 0;
    while (k < max && axt_tiff_deflate_byte(in, W, predictor, c + k) == axt_tiff_deflate_byte(in, W, predictor, p + k)) ++k;
    return k;
}

// One batch from `base` on: its tokens behind wk.tok[ntok]; returns the new base.
AXT_TIFF_HD uint32_t axt_def_batch(const uint16_t *in, uint32_t W, int predictor, uint32_t n, uint32_t base, axt_tiff_deflate_work &wk,
                                   uint32_t &ntok, uint32_t lane, uint32_t nlanes)
{
    const uint32_t cnt = n - base < AXT_DEF_BATCH ? n - base : AXT_DEF_BATCH;
    AXT_TIFF_LANES_SYNC();                                                // the last batch's walk has read mlen / mdist / mlit
    for (uint32_t i = lane; i < cnt; i += nlanes) {
        const uint32_t p = base + i, b0 = axt_tiff_deflate_byte(in, W, predictor, p);
        uint32_t best = 0, dist = 0;
        if (n - p >= AXT_DEF_MIN_MATCH) {
            const uint32_t max = n - p < AXT_DEF_MAX_MATCH ? n - p : AXT_DEF_MAX_MATCH;
            const uint32_t h = axt_def_hash(b0, axt_tiff_deflate_byte(in, W, predictor, p + 1), axt_tiff_deflate_byte(in, W, predictor, p + 2));
            const uint32_t e = wk.head[h];
            if (e && p - (e - 1) <= AXT_DEF_MAX_DIST) {                   // (e - 1 < base <= p)
                best = axt_def_match_length(in, W, predictor, e - 1, p, max);
                dist = p - (e - 1);
            }
            if (p >= 2) {
                const uint32_t l2 = axt_def_match_length(in, W, predictor, p - 2, p, max);
                if (l2 >= best) best = l2, dist = 2;
            }
            if (best < AXT_DEF_MIN_MATCH || (best == AXT_DEF_MIN_MATCH && dist > AXT_DEF_FAR)) best = 0;
        }
        wk.mlen[i] = (uint16_t)best;
        wk.mdist[i] = (uint16_t)(best ? dist - 1 : 0);
        wk.mlit[i] = (uint8_t)b0;
    }
    AXT_TIFF_LANES_SYNC();                                                // every probe has read the table as it was
    for (uint32_t i = lane; i < cnt; i += nlanes) {
        const uint32_t p = base + i;
        if (n - p >= AXT_DEF_MIN_MATCH) {
            const uint32_t h = axt_def_hash(wk.mlit[i], axt_tiff_deflate_byte(in, W, predictor, p + 1), axt_tiff_deflate_byte(in, W, predictor, p + 2));
            AXT_DEF_ATOMIC_MAX(&wk.head[h], p + 1);
        }
    }
    uint32_t i = 0;
    while (i < cnt) {                                                     // the greedy cover: the same walk on every worker
        const uint32_t l = wk.mlen[i];
        if (lane == 0) wk.tok[ntok] = l ? 1u << 23 | (l - 3) << 15 | wk.mdist[i] : wk.mlit[i];
        ++ntok;
        i += l ? l : 1;
    }
    return base + i;
}

// ------------------------------------------------------------------------------------------------ blocks
// The block of wk.tok[0, ntok) that stands for bytes [b0, b1). pending: start of the stored run not yet written, or
// 0xffffffff; a stored block only extends it.
AXT_TIFF_HD void axt_def_block(const uint16_t *in, uint32_t W, int predictor, uint32_t b0, uint32_t b1, uint32_t ntok, int final,
                               uint32_t &pending, axt_tiff_deflate_work &wk, axt_tiff_deflate_state &st, uint32_t lane, uint32_t nlanes)
{
    // frequencies
    AXT_TIFF_LANES_SYNC();
    for (uint32_t i = lane; i < AXT_DEF_SYMS; i += nlanes) wk.freq[i] = i == 256 ? 1u : 0u;
    AXT_TIFF_LANES_SYNC();
    for (uint32_t k = lane; k < ntok; k += nlanes) {
        const uint32_t t = wk.tok[k];
        if (t >> 23) {
            uint32_t s, e, v;
            axt_def_length_symbol((t >> 15 & 255) + 3, s, e, v);
            AXT_DEF_ATOMIC_ADD(&wk.freq[s], 1u);
            axt_def_dist_symbol((t & 32767) + 1, s, e, v);
            AXT_DEF_ATOMIC_ADD(&wk.freq[AXT_DEF_D0 + s], 1u);
        } else {
            AXT_DEF_ATOMIC_ADD(&wk.freq[t], 1u);
        }
    }
    axt_def_lengths(wk.freq, AXT_DEF_N_LL, 15, 0, wk.len, wk.order, lane, nlanes);
    axt_def_lengths(wk.freq + AXT_DEF_D0, AXT_DEF_N_D, 15, 0, wk.len + AXT_DEF_D0, wk.order, lane, nlanes);
    // the three sizes, in bits
    uint32_t dyn = 0, fix = 0;
    for (uint32_t i = lane; i < AXT_DEF_N_LL; i += nlanes) {
        const uint32_t f = wk.freq[i], x = i > 256 ? axt_def_length_extra(i) : 0;
        dyn += f * (wk.len[i] + x), fix += f * (axt_def_fixed_len(i) + x);
    }
    for (uint32_t i = lane; i < AXT_DEF_N_D; i += nlanes) {
        const uint32_t f = wk.freq[AXT_DEF_D0 + i], x = axt_def_dist_extra(i);
        dyn += f * (wk.len[AXT_DEF_D0 + i] + x), fix += f * (5 + x);
    }
    dyn = axt_def_sum(dyn, wk.red, lane, nlanes);
    fix = axt_def_sum(fix, wk.red, lane, nlanes);
    // the dynamic header: HLIT, HDIST, the lengths run-length coded (the same walk on every worker; one writes)
    uint32_t n_ll = AXT_DEF_N_LL, n_d = AXT_DEF_N_D;
    while (n_ll > 257 && wk.len[n_ll - 1] == 0) --n_ll;
    while (n_d > 1 && wk.len[AXT_DEF_D0 + n_d - 1] == 0) --n_d;
    AXT_TIFF_LANES_SYNC();
    for (uint32_t i = lane; i <= AXT_DEF_N_CL; i += nlanes) wk.freq_cl[i] = 0;
    AXT_TIFF_LANES_SYNC();
    uint32_t n_items = 0;
    const uint32_t n_seq = n_ll + n_d;
#define AXT_DEF_SEQ(k) ((uint32_t)wk.len[(k) < n_ll ? (k) : AXT_DEF_D0 + (k) - n_ll])
#define AXT_DEF_ITEM(sym, extra) do { if (lane == 0) wk.items[n_items] = (uint16_t)((sym) | (extra) << 5), wk.freq_cl[sym] += 1; ++n_items; } while (0)
    for (uint32_t k = 0; k < n_seq;) {
        const uint32_t v = AXT_DEF_SEQ(k);
        uint32_t run = 1;
        while (k + run < n_seq && AXT_DEF_SEQ(k + run) == v) ++run;
        k += run;
        if (v == 0) {
            while (run >= 11) {
                const uint32_t r = run < 138 ? run : 138;
                AXT_DEF_ITEM(18u, r - 11);
                run -= r;
            }
            if (run >= 3) {
                AXT_DEF_ITEM(17u, run - 3);
                run = 0;
            }
        } else {
            AXT_DEF_ITEM(v, 0u);
            --run;
            while (run >= 3) {
                const uint32_t r = run < 6 ? run : 6;
                AXT_DEF_ITEM(16u, r - 3);
                run -= r;
            }
        }
        for (; run; --run) AXT_DEF_ITEM(v, 0u);
    }
#undef AXT_DEF_SEQ
#undef AXT_DEF_ITEM
    axt_def_lengths(wk.freq_cl, AXT_DEF_N_CL, 7, 1, wk.len_cl, wk.order, lane, nlanes);
    uint32_t n_cl = AXT_DEF_N_CL;
    while (n_cl > 4 && wk.len_cl[axt_tiff_inflate_cl_order((int)n_cl - 1)] == 0) --n_cl;
    uint32_t hdr = 0;
    for (uint32_t k = lane; k < n_items; k += nlanes) {
        const uint32_t s = wk.items[k] & 31;
        hdr += wk.len_cl[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u);
    }
    hdr = axt_def_sum(hdr, wk.red, lane, nlanes) + 14 + 3 * n_cl;
    const uint64_t bits_dyn = 3ull + hdr + dyn, bits_fix = 3ull + fix;
    uint64_t bits_sto;
    if (pending != 0xffffffffu) {
        bits_sto = 8ull * (b1 - b0) + 40ull * (axt_def_pieces(b1 - pending) - axt_def_pieces(b0 - pending));
    } else {
        const uint32_t at = st.bitpos + 3;
        bits_sto = 3ull + ((8 - (at & 7)) & 7) + 32 + 8ull * (b1 - b0) + 40ull * (axt_def_pieces(b1 - b0) - 1);
    }
    const int type = bits_sto <= bits_fix && bits_sto <= bits_dyn ? AXT_DEF_STORED : bits_fix <= bits_dyn ? AXT_DEF_FIXED : AXT_DEF_DYNAMIC;
    if (type == AXT_DEF_STORED) {
        if (pending == 0xffffffffu) pending = b0;
        if (final) axt_def_stored(in, W, predictor, pending, b1, 1, wk, st, lane, nlanes);
        return;
    }
    if (pending != 0xffffffffu) {
        axt_def_stored(in, W, predictor, pending, b0, 0, wk, st, lane, nlanes);
        pending = 0xffffffffu;
    }
    axt_def_put(wk, st, (uint32_t)final | (uint32_t)type << 1, 3, lane, nlanes);
    if (type == AXT_DEF_FIXED) {
        AXT_TIFF_LANES_SYNC();
        for (uint32_t i = lane; i < AXT_DEF_N_LL; i += nlanes) {
            wk.len[i] = (uint16_t)axt_def_fixed_len(i);
            wk.code[i] = (uint16_t)axt_tiff_inflate_reverse(axt_def_fixed_code(i), (int)axt_def_fixed_len(i));
        }
        for (uint32_t i = lane; i < AXT_DEF_N_D; i += nlanes) {
            wk.len[AXT_DEF_D0 + i] = 5;
            wk.code[AXT_DEF_D0 + i] = (uint16_t)axt_tiff_inflate_reverse(i, 5);
        }
        AXT_TIFF_LANES_SYNC();
    } else {
        axt_def_codes(wk.len, AXT_DEF_N_LL, wk.code, lane, nlanes);
        axt_def_codes(wk.len + AXT_DEF_D0, AXT_DEF_N_D, wk.code + AXT_DEF_D0, lane, nlanes);
        axt_def_codes(wk.len_cl, AXT_DEF_N_CL, wk.code_cl, lane, nlanes);
        axt_def_put(wk, st, (n_ll - 257) | (n_d - 1) << 5 | (n_cl - 4) << 10, 14, lane, nlanes);
        for (uint32_t k = 0; k < n_cl; ++k) axt_def_put(wk, st, wk.len_cl[axt_tiff_inflate_cl_order((int)k)], 3, lane, nlanes);
        for (uint32_t k = 0; k < n_items; ++k) {
            const uint32_t s = wk.items[k] & 31, x = wk.items[k] >> 5, l = wk.len_cl[s];
            axt_def_put(wk, st, wk.code_cl[s] | x << l, l + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u), lane, nlanes);
        }
    }
    // the tokens: one a worker, placed by the scan of their lengths
    for (uint32_t k0 = 0; k0 < ntok; k0 += nlanes) {
        if (st.bitpos + AXT_DEF_TOKEN_BITS * AXT_DEF_BATCH + 64 > 32 * (AXT_DEF_STAGE_WORDS - 3)) axt_def_flush(wk, st, 0, lane, nlanes);
        uint32_t nbits = 0, total;
        uint64_t v = 0;
        if (k0 + lane < ntok) v = axt_def_token_bits(wk, wk.tok[k0 + lane], nbits);
        const uint32_t at = axt_def_scan(nbits, wk.red, lane, nlanes, total);
        axt_def_or(wk.stage, st.bitpos + at, v, nbits);
        st.bitpos += total;
    }
    axt_def_put(wk, st, wk.code[256], wk.len[256], lane, nlanes);
}

// ------------------------------------------------------------------------------------------------ one strip
// rows * W samples at `in` -> one zlib stream in out[0, cap). Returns the status (0, or 3 where the stream does not fit
// cap); *bytes: the stream's length (0 with status 3). batches: where not null, the batches the parse took.
AXT_TIFF_HD int axt_tiff_deflate_segment(const uint16_t *in, int rows, int W, int predictor, uint8_t *out, int64_t cap,
                                         axt_tiff_deflate_work &wk, uint32_t lane, uint32_t nlanes, int64_t *bytes, int64_t *batches = nullptr)
{
    const uint32_t n = (uint32_t)rows * (uint32_t)W * 2u;
    const int64_t bound = axt_tiff_deflate_bound_bytes(n);
    axt_tiff_deflate_state st;
    int64_t taken = 0;
    for (int all_stored = 0; all_stored < 2; ++all_stored) {
        st.out = out, st.cap = cap, st.out_pos = 0, st.bitpos = 0, st.overflow = 0;
        AXT_TIFF_LANES_SYNC();
        for (uint32_t i = lane; i < AXT_DEF_STAGE_WORDS; i += nlanes) wk.stage[i] = 0;
        for (uint32_t i = lane; i < (1u << AXT_DEF_HASH_BITS); i += nlanes) wk.head[i] = 0;
        AXT_TIFF_LANES_SYNC();
        axt_def_put(wk, st, 0x0178, 16, lane, nlanes);
        if (all_stored) {
            axt_def_stored(in, (uint32_t)W, predictor, 0, n, 1, wk, st, lane, nlanes);
        } else {
            uint32_t base = 0, pending = 0xffffffffu;
            const int64_t max_batches = axt_tiff_deflate_max_batches(n);
            do {
                const uint32_t b0 = base;
                uint32_t ntok = 0;
                while (base < n && ntok + AXT_DEF_BATCH <= AXT_DEF_TOKENS && taken < max_batches) {
                    base = axt_def_batch(in, (uint32_t)W, predictor, n, base, wk, ntok, lane, nlanes);
                    ++taken;
                }
                if (taken >= max_batches) base = n;                       // (cannot happen: the bound of the header comment)
                axt_def_block(in, (uint32_t)W, predictor, b0, base, ntok, base >= n, pending, wk, st, lane, nlanes);
            } while (base < n);
        }
        axt_def_flush(wk, st, 1, lane, nlanes);
        if (st.out_pos + 4 <= bound) break;
    }
    if (batches) *batches = taken;
    // the trailer
    uint64_t sa = 0, sb = 0;
    uint32_t turn = 0;
    for (uint32_t i = lane; i < n; i += nlanes) {
        const uint32_t b = axt_tiff_deflate_byte(in, (uint32_t)W, predictor, i);
        sa += b, sb += (uint64_t)(n - i) * b;
        if ((++turn & 4095) == 0) sb %= AXT_INF_ADLER_MOD;
        if (n - i <= nlanes) break;
    }
    const uint32_t a = axt_def_sum((uint32_t)(sa % AXT_INF_ADLER_MOD), wk.red, lane, nlanes);
    const uint32_t b = axt_def_sum((uint32_t)(sb % AXT_INF_ADLER_MOD), wk.red, lane, nlanes);
    const uint32_t adler = axt_tiff_adler_value(a, b, n);
    if (st.overflow || st.out_pos + 4 > cap) {
        *bytes = 0;
        return AXT_TIFF_OVERRUN;
    }
    if (lane < 4) out[st.out_pos + lane] = (uint8_t)(adler >> (24 - 8 * lane));
    if (nlanes < 4)
        for (uint32_t k = 1; k < 4; ++k) out[st.out_pos + k] = (uint8_t)(adler >> (24 - 8 * k));
    *bytes = st.out_pos + 4;
    return AXT_TIFF_OK;
}
