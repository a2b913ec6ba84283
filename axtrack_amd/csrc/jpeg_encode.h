// jpeg_encode.h -- the arithmetic of the baseline JPEG encoder of csrc/jpeg.hip as plain C++ that
// compiles for the host and for gfx950 alike: the kernels and the stand-alone host program of tests/test_jpeg_cpu.py
// (built with the sanitizers) run these very functions. Baseline sequential (SOF0), 8 bit, Y Cb Cr at 4:4:4, one MCU =
// one 8 x 8 block of each component, the Annex K quantisation and Huffman tables, a restart interval of one MCU row.
// Everything is integer; every `>>` is an arithmetic shift of an int (floor).
//
//   axt_jpeg_quant_tables    the two tables at a quality, IJG scaling
//   axt_jpeg_load_block      colour conversion of one component's 8 x 8 block, edges replicated, level shift
//   axt_jpeg_fdct_quant      forward DCT, quantisation, zigzag
//   axt_jpeg_code_dc / _ac   the Huffman codes of a block, handed to a sink (a bit counter, a bit writer)
//   axt_jpeg_encode_frame_serial   (host) one frame's scan segment, block after block: what the kernels must reproduce
//
// Ranges (the reason every intermediate is an int and the tables' categories suffice): a level-shifted sample p lies in
// [-128, 127]. A row of the DCT matrix C sums to at most 23168 in absolute value (row 0: 8 x 2896), the rows u > 0 to at
// most 21404. Row pass: |sum C p| <= 128 x 23168 = 2 965 504, so |t| <= 1448 (u = 0) and <= 1338 (u > 0). Column pass:
// |sum C t| <= 23168 x 1448 = 33 547 264 < 2^31, so |DC| <= 1024 and, a coefficient with u > 0 or v > 0 being bounded by
// max(1448 x 21404, 23168 x 1338) / 32768, |AC| <= 947. Quantisation divides by Q >= 1: a DC difference lies within
// +-2047 (category <= 11) and an AC value within +-1023 (category <= 10), the largest the Annex K tables code.
// A block therefore takes at most 9 + 11 (DC, luminance) or 11 + 11 (DC, chrominance) + 63 x (16 + 10) bits: at most
// AXT_JPEG_MAX_MCU_BITS = 20 + 22 + 22 + 3 x 1638 = 4978 bits per MCU before byte stuffing.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AXT_JPEG_HD __host__ __device__ inline
#else
#define AXT_JPEG_HD inline
#endif

enum { AXT_JPEG_MAX_MCU_BITS = 4978, AXT_JPEG_MAX_DIM = 65535 };

// position in the 8 x 8 block (natural order, 8 v + u) of the k-th coefficient in zigzag order
static constexpr uint8_t axt_jpeg_zigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// C[u][x] = round(8192 k(u) cos((2x + 1) u pi / 16)), k(0) = sqrt(1/8), k(u > 0) = 1/2
static constexpr int16_t axt_jpeg_dct[64] = {
    2896,  2896,  2896,  2896,  2896,  2896,  2896,  2896,
    4017,  3406,  2276,   799,  -799, -2276, -3406, -4017,
    3784,  1567, -1567, -3784, -3784, -1567,  1567,  3784,
    3406,  -799, -4017, -2276,  2276,  4017,   799, -3406,
    2896, -2896, -2896,  2896,  2896, -2896, -2896,  2896,
    2276, -4017,   799,  3406, -3406,  -799,  4017, -2276,
    1567, -3784,  3784, -1567, -1567,  3784, -3784,  1567,
     799, -2276,  3406, -4017,  4017, -3406,  2276,  -799};

// Annex K.1 / K.2, natural order
static constexpr uint8_t axt_jpeg_base_quant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3 - K.6 as a DHT segment states them: the number of codes of each length 1..16, then the symbols in code order
struct axt_jpeg_huff_spec { uint8_t bits[16]; uint8_t vals[162]; };
static constexpr axt_jpeg_huff_spec axt_jpeg_spec_dc[2] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}}};
static constexpr axt_jpeg_huff_spec axt_jpeg_spec_ac[2] = {
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
     {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
      36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73,
      74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133,
      134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180,
      181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226,
      227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250}},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119},
     {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
      21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
      73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131,
      132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178,
      179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
      226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}}};

// symbol -> (length << 16 | code), 0 for a symbol the table does not hold; derived at compile time (Annex C)
struct axt_jpeg_huff_codes { uint32_t e[256]; };
constexpr axt_jpeg_huff_codes axt_jpeg_derive(const axt_jpeg_huff_spec &s)
{
    axt_jpeg_huff_codes t{};
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) t.e[s.vals[k++]] = (uint32_t)len << 16 | code++;
        code <<= 1;
    }
    return t;
}
static constexpr axt_jpeg_huff_codes axt_jpeg_codes_dc[2] = {axt_jpeg_derive(axt_jpeg_spec_dc[0]), axt_jpeg_derive(axt_jpeg_spec_dc[1])};
static constexpr axt_jpeg_huff_codes axt_jpeg_codes_ac[2] = {axt_jpeg_derive(axt_jpeg_spec_ac[0]), axt_jpeg_derive(axt_jpeg_spec_ac[1])};

// ------------------------------------------------------------------------------------------------ quantisation tables
struct axt_jpeg_qtables { uint8_t q[2][64]; };          // natural order; [0] luminance, [1] chrominance

AXT_JPEG_HD axt_jpeg_qtables axt_jpeg_quant_tables(int quality)
{
    axt_jpeg_qtables t;
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) {
            const int v = (axt_jpeg_base_quant[c][i] * s + 50) / 100;
            t.q[c][i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
    return t;
}

// ------------------------------------------------------------------------------------------------ colour, DCT, quantisation
// component c (0 Y, 1 Cb, 2 Cr) of the block whose top-left pixel is (y0, x0) of the H x W RGB frame `rgb`, level-shifted;
// pixels beyond the last column / row repeat it
AXT_JPEG_HD void axt_jpeg_load_block(const uint8_t *rgb, int H, int W, int y0, int x0, int c, int p[64])
{
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        const int yy = y0 + y < H ? y0 + y : H - 1;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int xx = x0 + x < W ? x0 + x : W - 1;
            const uint8_t *px = rgb + ((int64_t)yy * W + xx) * 3;
            const int R = px[0], G = px[1], B = px[2];
            int v;
            if (c == 0) v = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
            else if (c == 1) v = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
            else v = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
            p[8 * y + x] = v - 128;
        }
    }
}

// p (natural order, 8 y + x) -> quantised coefficients in zigzag order; q in natural order
AXT_JPEG_HD void axt_jpeg_fdct_quant(const int p[64], const uint8_t q[64], int16_t zz[64])
{
    int t[64], coef[64];
#pragma unroll
    for (int y = 0; y < 8; ++y)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int s = 0;
#pragma unroll
            for (int x = 0; x < 8; ++x) s += axt_jpeg_dct[8 * u + x] * p[8 * y + x];
            t[8 * y + u] = (s + 1024) >> 11;
        }
#pragma unroll
    for (int v = 0; v < 8; ++v)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int s = 0;
#pragma unroll
            for (int y = 0; y < 8; ++y) s += axt_jpeg_dct[8 * v + y] * t[8 * y + u];
            coef[8 * v + u] = (s + 16384) >> 15;
        }
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int n = axt_jpeg_zigzag[k];
        const int c = coef[n], Q = q[n];
        const int m = ((c < 0 ? -c : c) + (Q >> 1)) / Q;
        zz[k] = (int16_t)(c < 0 ? -m : m);
    }
}

// ------------------------------------------------------------------------------------------------ entropy coding
// A sink has put(uint32_t bits, int n): the n <= 16 low bits of `bits`, most significant first.
AXT_JPEG_HD int axt_jpeg_category(int v)
{
    unsigned a = (unsigned)(v < 0 ? -v : v);
    int n = 0;
    while (a) { ++n; a >>= 1; }
    return n;
}

template <class Sink> AXT_JPEG_HD void axt_jpeg_put_value(int v, int cat, Sink &s)
{
    if (cat) s.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u), cat);
}

// the DC difference `diff` (this block's quantised DC minus its left neighbour's; the first block of an MCU row: minus 0)
template <class Sink> AXT_JPEG_HD void axt_jpeg_code_dc(int diff, int chroma, Sink &s)
{
    const int cat = axt_jpeg_category(diff);
    const uint32_t e = axt_jpeg_codes_dc[chroma].e[cat];
    s.put(e & 0xffffu, (int)(e >> 16));
    axt_jpeg_put_value(diff, cat, s);
}

// coefficients 1..63 of a block in zigzag order: (run, size) codes, ZRL for every 16 zeros of a longer run, EOB if the
// block ends in zeros
template <class Sink> AXT_JPEG_HD void axt_jpeg_code_ac(const int16_t zz[64], int chroma, Sink &s)
{
    const uint32_t *tab = axt_jpeg_codes_ac[chroma].e;
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) s.put(tab[0xf0] & 0xffffu, (int)(tab[0xf0] >> 16));
        const int cat = axt_jpeg_category(v);
        const uint32_t e = tab[run << 4 | cat];
        s.put(e & 0xffffu, (int)(e >> 16));
        axt_jpeg_put_value(v, cat, s);
        run = 0;
    }
    if (run) s.put(tab[0] & 0xffffu, (int)(tab[0] >> 16));
}

struct axt_jpeg_bit_counter {
    int bits = 0;
    AXT_JPEG_HD void put(uint32_t, int n) { bits += n; }
};

// ------------------------------------------------------------------------------------------------ sizes
AXT_JPEG_HD int64_t axt_jpeg_row_raw_bound(int W)        // bytes of one MCU row before stuffing, pad bits included
{
    return ((int64_t)((W + 7) / 8) * AXT_JPEG_MAX_MCU_BITS + 7) / 8;
}
AXT_JPEG_HD int64_t axt_jpeg_scan_bound_hw(int H, int W)  // every byte stuffed, a marker behind every row but the last
{
    const int64_t rows = (H + 7) / 8;
    return rows * 2 * axt_jpeg_row_raw_bound(W) + 2 * (rows - 1);
}

// ------------------------------------------------------------------------------------------------ the serial encoder (host)
#if !defined(__HIP_DEVICE_COMPILE__)
// bits into bytes, 0xFF followed by 0x00; never writes at or beyond `cap`, and goes on counting when the room is used up
struct axt_jpeg_byte_writer {
    uint8_t *out;
    int64_t cap, n = 0;
    uint32_t acc = 0;
    int nacc = 0;
    axt_jpeg_byte_writer(uint8_t *o, int64_t c) : out(o), cap(c) {}
    void byte(uint8_t b)
    {
        if (n < cap) out[n] = b;
        ++n;
    }
    void put(uint32_t bits, int nb)
    {
        acc = acc << nb | bits;
        nacc += nb;
        while (nacc >= 8) {
            const uint8_t b = (uint8_t)(acc >> (nacc - 8));
            nacc -= 8;
            byte(b);
            if (b == 0xff) byte(0);
        }
        acc &= (1u << nacc) - 1u;
    }
};

// One frame's entropy-coded segment (what stands between the SOS header and EOI). Returns the bytes it takes; they are
// complete in `out` if that is <= cap.
inline int64_t axt_jpeg_encode_frame_serial(const uint8_t *rgb, int H, int W, int quality, uint8_t *out, int64_t cap)
{
    const axt_jpeg_qtables qt = axt_jpeg_quant_tables(quality);
    const int bw = (W + 7) / 8, bh = (H + 7) / 8;
    axt_jpeg_byte_writer w(out, cap);
    for (int by = 0; by < bh; ++by) {
        int pred[3] = {0, 0, 0};
        for (int bx = 0; bx < bw; ++bx)
            for (int c = 0; c < 3; ++c) {
                int p[64];
                int16_t zz[64];
                axt_jpeg_load_block(rgb, H, W, 8 * by, 8 * bx, c, p);
                axt_jpeg_fdct_quant(p, qt.q[c != 0], zz);
                axt_jpeg_code_dc(zz[0] - pred[c], c != 0, w);
                pred[c] = zz[0];
                axt_jpeg_code_ac(zz, c != 0, w);
            }
        if (w.nacc) w.put((1u << (8 - w.nacc)) - 1u, 8 - w.nacc);          // pad the row's last byte with 1-bits
        if (by < bh - 1) {
            w.byte(0xff);
            w.byte((uint8_t)(0xd0 + (by & 7)));
        }
    }
    return w.n;
}
#endif
