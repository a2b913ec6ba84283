// tiff_decode.h -- the strip decoder core of csrc/tiff.hip as plain C++ that compiles for the host and
// for gfx950 alike: the kernels and the stand-alone host program of tests/test_tiff_cpu.py (built with the sanitizers)
// run these very functions. Everything that can go out of range is decided HERE, before a byte is copied:
//
//   axt_tiff_check_segment   descriptor against src_len / out_len                                      -> status 4
//   axt_tiff_lzw_next        one LZW code: MSB-first bit reader, 9..12 bit schedule, Clear / EOI, table  -> status 1, 2, 3
//   axt_tiff_packbits_next   one PackBits run header                                                    -> status 1, 3
//   axt_tiff_apply           the copy an accepted code or run stands for, strided over `nlanes` workers
//
// A step consumes at least one code / one header byte or ends the segment, and hands back ONE copy operation whose
// source and destination ranges it has already checked against [0, src_bytes) and [0, out_bytes). The caller bounds the
// number of steps by axt_tiff_max_steps; on the device the 64 lanes of a wave take the same steps (the parse is
// wave-uniform) and share each copy, on the host nlanes = 1.
//
// The LZW table holds no strings. Every code's string is written to the output when the code is read, so the entry
// added after a code -- the previous string plus the first byte of the current one -- IS the output range
// [p_prev, p_prev + L_prev + 1): the current string lands right behind the previous one. An entry is that range's
// (offset, length); the "code == next free entry" case (KwKwK) is out[p_prev + i % L_prev] for i < L_prev + 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AXT_TIFF_HD __host__ __device__ inline
#else
#define AXT_TIFF_HD inline
#endif

enum {
    AXT_TIFF_OK = 0,
    AXT_TIFF_SHORT_INPUT = 1,        // input exhausted (or EOI) before rows * W samples were produced
    AXT_TIFF_BAD_CODE = 2,           // LZW code above the next free entry, non-literal first code, table overflow
    AXT_TIFF_OVERRUN = 3,            // the next string or run would pass the end of the segment's output
    AXT_TIFF_BAD_SEGMENT = 4         // descriptor out of range
};

enum { AXT_TIFF_COMP_NONE = 1, AXT_TIFF_COMP_LZW = 5, AXT_TIFF_COMP_PACKBITS = 32773 };

enum { AXT_TIFF_LZW_CLEAR = 256, AXT_TIFF_LZW_EOI = 257, AXT_TIFF_LZW_FIRST = 258, AXT_TIFF_LZW_ENTRIES = 4096 };

// one copy, all offsets in bytes and already checked: dst, len inside the segment's output; src inside the segment's
// input (FROM_INPUT) or inside the output written so far (FROM_OUTPUT, read with period `period`)
enum { AXT_TIFF_OP_NONE = 0, AXT_TIFF_OP_FROM_INPUT = 1, AXT_TIFF_OP_FROM_OUTPUT = 2, AXT_TIFF_OP_FILL = 3 };
struct axt_tiff_op {
    int kind;
    uint32_t dst, len;
    int64_t src;          // FROM_INPUT: offset in the segment's input; FROM_OUTPUT: offset in its output; FILL: the byte
    uint32_t period;      // FROM_OUTPUT: out[dst + i] = out[src + i % period]
};

struct axt_tiff_state {
    int64_t pos;          // LZW: bit position in the input; PackBits: byte position
    uint32_t out_pos;     // bytes of output produced
    uint32_t prev_off, prev_len;      // LZW: where the previous code's string stands in the output; prev_len 0 = none yet
    int width, next;      // LZW: current code width, next free table entry
    int status, done;
};

AXT_TIFF_HD void axt_tiff_state_init(axt_tiff_state &s)
{
    s.pos = 0;
    s.out_pos = 0;
    s.prev_off = 0, s.prev_len = 0;
    s.width = 9, s.next = AXT_TIFF_LZW_FIRST;
    s.status = AXT_TIFF_OK, s.done = 0;
}

AXT_TIFF_HD void axt_tiff_finish(axt_tiff_state &s, int status)
{
    s.status = status;
    s.done = 1;
}

// 0 when the segment lies inside both buffers and its output fits the decoder's 32-bit byte offsets, else status 4
AXT_TIFF_HD int axt_tiff_check_segment(int64_t src_offset, int64_t src_bytes, int64_t dst_offset, int32_t rows, int W,
                                       int64_t src_len, int64_t out_len)
{
    if (src_offset < 0 || src_bytes < 0 || dst_offset < 0 || rows < 0 || W < 0 || src_len < 0 || out_len < 0)
        return AXT_TIFF_BAD_SEGMENT;
    if (src_offset > src_len || src_bytes > src_len - src_offset) return AXT_TIFF_BAD_SEGMENT;
    const int64_t samples = (int64_t)rows * W;
    if (samples > 0x7fffffffLL) return AXT_TIFF_BAD_SEGMENT;              // 2 * samples fits uint32_t
    if (dst_offset > out_len || samples > out_len - dst_offset) return AXT_TIFF_BAD_SEGMENT;
    return AXT_TIFF_OK;
}

// the number of steps that consumes any input of src_bytes: a code has at least 9 bits, a run header one byte
AXT_TIFF_HD int64_t axt_tiff_max_steps(int compression, int64_t src_bytes)
{
    return compression == AXT_TIFF_COMP_LZW ? 8 * src_bytes / 9 + 1 : src_bytes;
}

// `width` bits at bit position `pos`, most significant bit first. The caller has checked pos + width <= 8 * src_bytes,
// so the two or three bytes read here, pos / 8 .. (pos + width - 1) / 8, are inside the input.
AXT_TIFF_HD int axt_tiff_read_code(const uint8_t *src, int64_t pos, int width)
{
    const int64_t b0 = pos >> 3, b1 = (pos + width - 1) >> 3;
    uint32_t acc = 0;
    for (int64_t b = b0; b <= b1; ++b) acc = acc << 8 | src[b];
    const int tail = (int)(((b1 + 1) << 3) - (pos + width));             // bits right of the code in the last byte
    return (int)(acc >> tail) & ((1 << width) - 1);
}

// One LZW code. tbl_off / tbl_len: AXT_TIFF_LZW_ENTRIES entries each; only [258, next) is ever read.
AXT_TIFF_HD void axt_tiff_lzw_next(const uint8_t *src, int64_t src_bytes, uint32_t out_bytes, axt_tiff_state &s,
                                   uint32_t *tbl_off, uint16_t *tbl_len, axt_tiff_op &op)
{
    op.kind = AXT_TIFF_OP_NONE;
    op.dst = s.out_pos, op.len = 0, op.src = 0, op.period = 1;
    if (s.out_pos >= out_bytes) return axt_tiff_finish(s, AXT_TIFF_OK);   // complete: stops here, EOI or not
    if (s.pos + s.width > 8 * src_bytes) return axt_tiff_finish(s, AXT_TIFF_SHORT_INPUT);
    const int code = axt_tiff_read_code(src, s.pos, s.width);
    s.pos += s.width;
    if (code == AXT_TIFF_LZW_EOI) return axt_tiff_finish(s, AXT_TIFF_SHORT_INPUT);
    if (code == AXT_TIFF_LZW_CLEAR) {
        s.width = 9, s.next = AXT_TIFF_LZW_FIRST, s.prev_len = 0;
        return;
    }
    uint32_t len;
    if (code < 256) {
        op.kind = AXT_TIFF_OP_FILL, op.src = code, len = 1;
    } else if (s.prev_len == 0) {
        return axt_tiff_finish(s, AXT_TIFF_BAD_CODE);                     // the first code after Clear must be a literal
    } else if (code < s.next) {
        op.kind = AXT_TIFF_OP_FROM_OUTPUT, op.src = tbl_off[code], len = tbl_len[code], op.period = len;
    } else if (code == s.next) {
        op.kind = AXT_TIFF_OP_FROM_OUTPUT, op.src = s.prev_off, len = s.prev_len + 1, op.period = s.prev_len;
    } else {
        return axt_tiff_finish(s, AXT_TIFF_BAD_CODE);
    }
    if (len > out_bytes - s.out_pos) {
        op.kind = AXT_TIFF_OP_NONE;
        return axt_tiff_finish(s, AXT_TIFF_OVERRUN);
    }
    if (s.prev_len != 0) {                                                // previous string + this string's first byte
        if (s.next >= AXT_TIFF_LZW_ENTRIES) {
            op.kind = AXT_TIFF_OP_NONE;
            return axt_tiff_finish(s, AXT_TIFF_BAD_CODE);                 // the writer owed a Clear
        }
        tbl_off[s.next] = s.prev_off;
        tbl_len[s.next] = (uint16_t)(s.prev_len + 1);                     // (< 4096: one byte more per entry since Clear)
        ++s.next;
        if (s.next + 1 >= (1 << s.width) && s.width < 12) ++s.width;      // early change
    }
    op.len = len;
    s.prev_off = s.out_pos, s.prev_len = len;
    s.out_pos += len;
    if (s.out_pos == out_bytes) axt_tiff_finish(s, AXT_TIFF_OK);
}

// One PackBits header: n in 0..127 copies n + 1 literal bytes, n in -127..-1 repeats the next byte 1 - n times, -128 nothing.
AXT_TIFF_HD void axt_tiff_packbits_next(const uint8_t *src, int64_t src_bytes, uint32_t out_bytes, axt_tiff_state &s,
                                        axt_tiff_op &op)
{
    op.kind = AXT_TIFF_OP_NONE;
    op.dst = s.out_pos, op.len = 0, op.src = 0, op.period = 1;
    if (s.out_pos >= out_bytes) return axt_tiff_finish(s, AXT_TIFF_OK);
    if (s.pos >= src_bytes) return axt_tiff_finish(s, AXT_TIFF_SHORT_INPUT);
    const int n = (int)(int8_t)src[s.pos];
    s.pos += 1;
    if (n == -128) return;
    uint32_t len;
    if (n >= 0) {
        len = (uint32_t)n + 1;
        if ((int64_t)len > src_bytes - s.pos) return axt_tiff_finish(s, AXT_TIFF_SHORT_INPUT);
        op.kind = AXT_TIFF_OP_FROM_INPUT, op.src = s.pos;
        s.pos += len;
    } else {
        len = (uint32_t)(1 - n);
        if (s.pos >= src_bytes) return axt_tiff_finish(s, AXT_TIFF_SHORT_INPUT);
        op.kind = AXT_TIFF_OP_FILL, op.src = src[s.pos];
        s.pos += 1;
    }
    if (len > out_bytes - s.out_pos) {
        op.kind = AXT_TIFF_OP_NONE;
        return axt_tiff_finish(s, AXT_TIFF_OVERRUN);
    }
    op.len = len;
    s.out_pos += len;
    if (s.out_pos == out_bytes) axt_tiff_finish(s, AXT_TIFF_OK);
}

// The copy of one accepted step, worker `lane` of `nlanes` taking every nlanes-th byte. src: the segment's input,
// out: the segment's output as bytes.
AXT_TIFF_HD void axt_tiff_apply(const axt_tiff_op &op, const uint8_t *src, uint8_t *out, uint32_t lane, uint32_t nlanes)
{
    if (op.kind == AXT_TIFF_OP_FILL) {
        for (uint32_t i = lane; i < op.len; i += nlanes) out[op.dst + i] = (uint8_t)op.src;
    } else if (op.kind == AXT_TIFF_OP_FROM_INPUT) {
        for (uint32_t i = lane; i < op.len; i += nlanes) out[op.dst + i] = src[op.src + i];
    } else if (op.kind == AXT_TIFF_OP_FROM_OUTPUT) {
        if (op.period >= op.len) {
            for (uint32_t i = lane; i < op.len; i += nlanes) out[op.dst + i] = out[op.src + i];
        } else {
            for (uint32_t i = lane; i < op.len; i += nlanes) out[op.dst + i] = out[op.src + i % op.period];
        }
    }
}

// a 16-bit sample from two bytes at any address, in the file's byte order
AXT_TIFF_HD uint16_t axt_tiff_sample(const uint8_t *p, int big_endian)
{
    return big_endian ? (uint16_t)(p[0] << 8 | p[1]) : (uint16_t)(p[1] << 8 | p[0]);
}

// Whole segment on one worker: what the host program runs, and the statement of what the kernel computes. bytes:
// the segment's output viewed as bytes (decoded in place, then swapped and accumulated row by row into `out`).
inline int axt_tiff_decode_segment_serial(const uint8_t *src, int64_t src_bytes, int rows, int W, int compression, int predictor,
                                          int big_endian, uint16_t *out, uint32_t *tbl_off, uint16_t *tbl_len)
{
    const uint32_t out_bytes = (uint32_t)rows * (uint32_t)W * 2u;
    uint8_t *bytes = reinterpret_cast<uint8_t *>(out);
    const uint8_t *rows_from = bytes;
    if (compression == AXT_TIFF_COMP_NONE) {
        if (src_bytes < (int64_t)out_bytes) return AXT_TIFF_SHORT_INPUT;
        rows_from = src;
    } else {
        axt_tiff_state s;
        axt_tiff_state_init(s);
        axt_tiff_op op;
        const int64_t steps = axt_tiff_max_steps(compression, src_bytes);
        for (int64_t it = 0; it < steps && !s.done; ++it) {
            if (compression == AXT_TIFF_COMP_LZW) axt_tiff_lzw_next(src, src_bytes, out_bytes, s, tbl_off, tbl_len, op);
            else axt_tiff_packbits_next(src, src_bytes, out_bytes, s, op);
            axt_tiff_apply(op, src, bytes, 0, 1);
        }
        if (!s.done) axt_tiff_finish(s, s.out_pos >= out_bytes ? AXT_TIFF_OK : AXT_TIFF_SHORT_INPUT);
        if (s.status != AXT_TIFF_OK) return s.status;
    }
    for (int r = 0; r < rows; ++r) {
        uint16_t acc = 0;
        for (int x = 0; x < W; ++x) {
            const uint16_t v = axt_tiff_sample(rows_from + ((size_t)r * W + x) * 2, big_endian);
            acc = predictor == 2 ? (uint16_t)(acc + v) : v;
            out[(size_t)r * W + x] = acc;
        }
    }
    return AXT_TIFF_OK;
}
