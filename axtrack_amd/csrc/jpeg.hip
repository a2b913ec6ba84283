// jpeg.hip -- rendered RGB frames into baseline JPEG scan segments on gfx950. The arithmetic is
// jpeg_encode.h, shared with the host; this file is the parallel schedule. The restart interval is one MCU row, so every
// (frame, MCU row) is coded on its own, and inside a row a block needs only its left neighbour's quantised DC.
//
//   jpeg_transform_k   one thread per (MCU, component): colour, DCT, quantisation, zigzag -> int16 coefficients and the bit
//                      length of the block's AC codes. (The DC code's length needs the neighbour's DC, which another
//                      thread is still computing: it is added where the lengths are scanned.)
//   jpeg_emit_k        one workgroup per MCU row. Pass 1 sums the row's bits and zeroes exactly the words they will
//                      occupy in the row's raw buffer; pass 2 scans the lengths, kJpegThreads MCUs per step with a
//                      running carry, and every thread ORs its MCU's codes into place (atomicOr on 32-bit words, stored
//                      big-endian: bits of different MCUs never overlap, so the result does not depend on the order).
//                      Thread 0 pads the last byte with 1-bits.
//   jpeg_count_k       one workgroup per row: the row's 0xFF bytes -> its stuffed length.
//   jpeg_offsets_k     one workgroup per frame: scan of the row lengths (plus 2 per marker) -> every row's offset in the
//                      frame's slot, the frame's byte count, status 1 if that exceeds scan_capacity.
//   jpeg_pack_k        one workgroup per row of a frame that fits: kJpegStuffChunk raw bytes per step, 4 per thread; a
//                      scan of the 0xFF counts, carried from step to step, places every byte (and the 0x00 behind a
//                      0xFF) straight into the slot; then the RSTm marker.
//
// The stuffed row is never staged: the second worst-case buffer that would take is the reason the stuffing pass writes
// into the slot, behind the per-frame scan, and not before it. Nothing that scales with W lives in LDS (a row of the
// reference's recordings has 721 MCUs, a block's worst case is 208 bytes); LDS holds the scans' wave totals only.
//
// Scratch (axt_jpeg_scratch_bytes; B = blocks = n_frames x bh x bw, R = n_frames x bh), each part 256-byte aligned:
//   coef      int16 [B][3][64]      aclen  uint16 [B][3]      raw  R x rowcap bytes, rowcap = axt_jpeg_row_raw_bound(W) up to 4
//   rowbits   int32 [R]             rowlen int32 [R]          rowoff int64 [R]
// Kernel boundaries order the passes; inside jpeg_emit_k the zeroing stores are released (fence + barrier) before the
// first atomic.
#include "axt_common.h"
#include "jpeg_encode.h"

namespace {

constexpr int kJpegThreads = 256;              // threads per workgroup, every kernel
constexpr int kJpegMcusPerThread = 1;          // jpeg_emit_k: MCUs per thread and step
constexpr int kJpegStuffBytesPerThread = 4;    // jpeg_count_k / jpeg_pack_k: raw bytes per thread and step
constexpr int kJpegStuffChunk = kJpegThreads * kJpegStuffBytesPerThread;
constexpr int kJpegMaxGrid = 1 << 16;          // workgroups per launch; the kernels stride beyond

struct JpegScratch {
    int16_t *coef;
    uint16_t *aclen;
    uint8_t *raw;
    int32_t *rowbits, *rowlen;
    int64_t *rowoff;
    int64_t rowcap, bytes;
};

int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }

JpegScratch jpeg_scratch_layout(void *base, int64_t n_frames, int H, int W)
{
    const int64_t bw = (W + 7) / 8, bh = (H + 7) / 8, R = n_frames * bh, B = R * bw;
    JpegScratch s;
    uint8_t *p = static_cast<uint8_t *>(base);
    int64_t o = 0;
    s.rowcap = (axt_jpeg_row_raw_bound(W) + 3) & ~(int64_t)3;
    s.coef = reinterpret_cast<int16_t *>(p + o), o += up256(B * 3 * 64 * 2);
    s.aclen = reinterpret_cast<uint16_t *>(p + o), o += up256(B * 3 * 2);
    s.raw = p + o, o += up256(R * s.rowcap);
    s.rowbits = reinterpret_cast<int32_t *>(p + o), o += up256(R * 4);
    s.rowlen = reinterpret_cast<int32_t *>(p + o), o += up256(R * 4);
    s.rowoff = reinterpret_cast<int64_t *>(p + o), o += up256(R * 8);
    s.bytes = o;
    return s;
}

// exclusive scan of v over the workgroup (kJpegThreads = 4 waves); total = the sum, in every thread. Every thread of the
// workgroup must call it. `part` is 4 entries of LDS, free again when the call returns.
template <typename T> __device__ __forceinline__ T jpeg_block_scan(T v, T &total, T *part)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    T before = 0, sum = 0;
    for (int w = 0; w < kJpegThreads / 64; ++w) {
        const T t = part[w];
        if (w < wave) before += t;
        sum += t;
    }
    __syncthreads();
    total = sum;
    return before + inc - v;
}

__global__ __launch_bounds__(kJpegThreads) void jpeg_transform_k(const uint8_t *__restrict__ rgb, int H, int W, int64_t frame_stride,
                                                                int bh, int bw, int64_t n_items, axt_jpeg_qtables qt,
                                                                int16_t *__restrict__ coef, uint16_t *__restrict__ aclen)
{
    for (int64_t g = (int64_t)blockIdx.x * kJpegThreads + threadIdx.x; g < n_items; g += (int64_t)gridDim.x * kJpegThreads) {
        const int c = (int)(g % 3);
        const int64_t b = g / 3;
        const int bx = (int)(b % bw);
        const int64_t r = b / bw;
        const int by = (int)(r % bh);
        const int64_t f = r / bh;
        int p[64];
        alignas(16) int16_t zz[64];
        axt_jpeg_load_block(rgb + f * frame_stride, H, W, 8 * by, 8 * bx, c, p);
        axt_jpeg_fdct_quant(p, qt.q[c != 0], zz);
        uint4 *dst = reinterpret_cast<uint4 *>(coef + g * 64);
        const uint4 *src = reinterpret_cast<const uint4 *>(zz);
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = src[k];
        axt_jpeg_bit_counter n;
        axt_jpeg_code_ac(coef + g * 64, c != 0, n);                      // (its own stores: the walk indexes memory, not registers)
        aclen[g] = (uint16_t)n.bits;
    }
}

// bits of MCU m (index in the whole batch; m0 = its row's first MCU) with the DC codes
__device__ __forceinline__ int jpeg_mcu_bits(const int16_t *__restrict__ coef, const uint16_t *__restrict__ aclen, int64_t m, int64_t m0)
{
    int bits = 0;
    for (int c = 0; c < 3; ++c) {
        const int dc = coef[(m * 3 + c) * 64], left = m > m0 ? coef[((m - 1) * 3 + c) * 64] : 0;
        axt_jpeg_bit_counter n;
        axt_jpeg_code_dc(dc - left, c != 0, n);
        bits += n.bits + aclen[m * 3 + c];
    }
    return bits;
}

// MSB-first bits into big-endian 32-bit words of a zeroed buffer, from bit `pos` on
struct JpegWordSink {
    uint32_t *words;
    uint64_t acc = 0;
    int nacc;
    __device__ JpegWordSink(uint32_t *w, int64_t pos) : words(w + (pos >> 5)), nacc((int)(pos & 31)) {}
    __device__ __forceinline__ void put(uint32_t bits, int n)
    {
        acc = acc << n | bits;
        nacc += n;
        if (nacc >= 32) {
            nacc -= 32;
            atomicOr(words++, __builtin_bswap32((uint32_t)(acc >> nacc)));
            acc &= (1ull << nacc) - 1ull;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (nacc) atomicOr(words, __builtin_bswap32((uint32_t)(acc << (32 - nacc))));
        nacc = 0, acc = 0;
    }
};

__global__ __launch_bounds__(kJpegThreads) void jpeg_emit_k(const int16_t *__restrict__ coef, const uint16_t *__restrict__ aclen, int bw,
                                                           int64_t n_rows, uint8_t *raw, int64_t rowcap, int32_t *__restrict__ rowbits)
{
    __shared__ int part[kJpegThreads / 64];
    const int tid = threadIdx.x;
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int64_t m0 = r * bw;
        uint32_t *words = reinterpret_cast<uint32_t *>(raw + r * rowcap);
        int mine = 0;
        for (int x = tid; x < bw; x += kJpegThreads) mine += jpeg_mcu_bits(coef, aclen, m0 + x, m0);
        int total;
        jpeg_block_scan(mine, total, part);
        const int n_words = (total + 31) >> 5;                            // <= rowcap / 4: total <= bw x AXT_JPEG_MAX_MCU_BITS
        for (int i = tid; i < n_words; i += kJpegThreads) words[i] = 0u;
        __threadfence();
        __syncthreads();
        int carry = 0;
        for (int x0 = 0; x0 < bw; x0 += kJpegThreads * kJpegMcusPerThread) {   // (uniform trip count: the scan has barriers)
            const int x = x0 + tid;
            const int bits = x < bw ? jpeg_mcu_bits(coef, aclen, m0 + x, m0) : 0;
            int step;
            const int at = carry + jpeg_block_scan(bits, step, part);
            carry += step;
            if (x < bw) {
                JpegWordSink s(words, at);
                for (int c = 0; c < 3; ++c) {
                    const int16_t *zz = coef + ((m0 + x) * 3 + c) * 64;
                    axt_jpeg_code_dc(zz[0] - (x ? zz[-3 * 64] : 0), c != 0, s);
                    axt_jpeg_code_ac(zz, c != 0, s);
                }
                s.flush();
            }
        }
        if (tid == 0) {
            const int pad = -total & 7;
            if (pad) {
                JpegWordSink s(words, total);
                s.put((1u << pad) - 1u, pad);
                s.flush();
            }
            rowbits[r] = total;
        }
    }
}

// the 4 raw bytes [i, i + 4) of a row as a word (byte i lowest), bytes at or beyond nb as 0; the 0xFF bytes among them
__device__ __forceinline__ uint32_t jpeg_raw_word(const uint8_t *row, int i, int nb)
{
    if (i >= nb) return 0u;
    uint32_t w = *reinterpret_cast<const uint32_t *>(row + i);         // (rowcap is a multiple of 4: the word is the row's)
    const int keep = nb - i;
    if (keep < 4) w &= (1u << (8 * keep)) - 1u;
    return w;
}
__device__ __forceinline__ int jpeg_ff_count(uint32_t w)
{
    return ((w & 0xffu) == 0xffu) + ((w >> 8 & 0xffu) == 0xffu) + ((w >> 16 & 0xffu) == 0xffu) + ((w >> 24) == 0xffu);
}

__global__ __launch_bounds__(kJpegThreads) void jpeg_count_k(const uint8_t *__restrict__ raw, int64_t rowcap, const int32_t *__restrict__ rowbits,
                                                            int64_t n_rows, int32_t *__restrict__ rowlen)
{
    __shared__ int part[kJpegThreads / 64];
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const uint8_t *row = raw + r * rowcap;
        const int nb = (rowbits[r] + 7) >> 3;
        int mine = 0;
        for (int i = threadIdx.x * kJpegStuffBytesPerThread; i < nb; i += kJpegStuffChunk) mine += jpeg_ff_count(jpeg_raw_word(row, i, nb));
        int total;
        jpeg_block_scan(mine, total, part);
        if (threadIdx.x == 0) rowlen[r] = nb + total;
    }
}

__global__ __launch_bounds__(kJpegThreads) void jpeg_offsets_k(const int32_t *__restrict__ rowlen, int bh, int n_frames, int64_t scan_capacity,
                                                              int64_t *__restrict__ rowoff, int64_t *__restrict__ scan_bytes,
                                                              int32_t *__restrict__ status)
{
    __shared__ long long part[kJpegThreads / 64];
    for (int f = blockIdx.x; f < n_frames; f += gridDim.x) {
        long long carry = 0;
        for (int y0 = 0; y0 < bh; y0 += kJpegThreads) {
            const int y = y0 + threadIdx.x;
            const long long len = y < bh ? (long long)rowlen[(int64_t)f * bh + y] + (y < bh - 1 ? 2 : 0) : 0;
            long long step;
            const long long at = carry + jpeg_block_scan(len, step, part);
            carry += step;
            if (y < bh) rowoff[(int64_t)f * bh + y] = at;
        }
        if (threadIdx.x == 0) {
            scan_bytes[f] = carry;
            status[f] = carry > scan_capacity;
        }
    }
}

__global__ __launch_bounds__(kJpegThreads) void jpeg_pack_k(const uint8_t *__restrict__ raw, int64_t rowcap, const int32_t *__restrict__ rowbits,
                                                           const int32_t *__restrict__ rowlen, const int64_t *__restrict__ rowoff,
                                                           const int32_t *__restrict__ status, int bh, int64_t n_rows,
                                                           uint8_t *__restrict__ scan, int64_t scan_capacity)
{
    __shared__ int part[kJpegThreads / 64];
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int64_t f = r / bh;
        const int by = (int)(r % bh);
        if (status[f]) continue;                                          // (uniform: the whole workgroup skips the row)
        const uint8_t *row = raw + r * rowcap;
        uint8_t *dst = scan + f * scan_capacity + rowoff[r];              // rowoff + rowlen (+ 2) <= scan_bytes <= scan_capacity
        const int nb = (rowbits[r] + 7) >> 3;
        int carry = 0;                                                    // 0xFF bytes before this step
        for (int i0 = 0; i0 < nb; i0 += kJpegStuffChunk) {
            const int i = i0 + threadIdx.x * kJpegStuffBytesPerThread;
            const uint32_t w = jpeg_raw_word(row, i, nb);
            int step;
            int o = i + carry + jpeg_block_scan(jpeg_ff_count(w), step, part);
            carry += step;
            for (int k = 0; k < kJpegStuffBytesPerThread && i + k < nb; ++k) {
                const uint8_t b = (uint8_t)(w >> (8 * k));
                dst[o++] = b;
                if (b == 0xffu) dst[o++] = 0u;
            }
        }
        if (threadIdx.x == 0 && by < bh - 1) {
            dst[rowlen[r]] = 0xffu;
            dst[rowlen[r] + 1] = (uint8_t)(0xd0 + (by & 7));
        }
    }
}

int jpeg_grid(int64_t n) { return (int)(n < kJpegMaxGrid ? n : kJpegMaxGrid); }

}  // namespace

extern "C" int64_t axt_jpeg_scan_bound(int H, int W)
{
    if (H < 1 || W < 1 || H > AXT_JPEG_MAX_DIM || W > AXT_JPEG_MAX_DIM) {
        axt_set_error("axt_jpeg_scan_bound: H %d or W %d outside 1..65535", H, W);
        return AXT_EINVAL;
    }
    return axt_jpeg_scan_bound_hw(H, W);
}

extern "C" int64_t axt_jpeg_scratch_bytes(int n_frames, int H, int W)
{
    if (n_frames < 0 || H < 1 || W < 1 || H > AXT_JPEG_MAX_DIM || W > AXT_JPEG_MAX_DIM) {
        axt_set_error("axt_jpeg_scratch_bytes: n_frames %d negative, or H %d or W %d outside 1..65535", n_frames, H, W);
        return AXT_EINVAL;
    }
    return jpeg_scratch_layout(nullptr, n_frames, H, W).bytes;
}

extern "C" int axt_jpeg_encode_rgb8(const uint8_t *d_rgb, int n_frames, int H, int W, int64_t frame_stride, int quality,
                                    uint8_t *d_scan, int64_t scan_capacity, int64_t *d_scan_bytes, int32_t *d_status,
                                    void *d_scratch, int64_t scratch_bytes, void *stream)
{
    AXT_REQUIRE(d_rgb && d_scan && d_scan_bytes && d_status && d_scratch, "axt_jpeg_encode_rgb8: null argument");
    AXT_REQUIRE(((uintptr_t)d_scratch & 15) == 0, "axt_jpeg_encode_rgb8: d_scratch is not 16-byte aligned");
    AXT_REQUIRE(n_frames >= 0 && frame_stride >= 0 && scan_capacity >= 0 && scratch_bytes >= 0,
                "axt_jpeg_encode_rgb8: negative size (n_frames %d, frame_stride %lld, scan_capacity %lld, scratch_bytes %lld)", n_frames,
                (long long)frame_stride, (long long)scan_capacity, (long long)scratch_bytes);
    AXT_REQUIRE(H >= 1 && H <= AXT_JPEG_MAX_DIM && W >= 1 && W <= AXT_JPEG_MAX_DIM, "axt_jpeg_encode_rgb8: H %d or W %d outside 1..65535", H,
                W);
    AXT_REQUIRE(quality >= 1 && quality <= 100, "axt_jpeg_encode_rgb8: quality %d outside 1..100", quality);
    AXT_REQUIRE(frame_stride >= (int64_t)3 * H * W, "axt_jpeg_encode_rgb8: frame_stride %lld below 3 x %d x %d", (long long)frame_stride, H,
                W);
    const int bw = (W + 7) / 8, bh = (H + 7) / 8;
    const int64_t n_rows = (int64_t)n_frames * bh, n_blocks = n_rows * bw;
    AXT_REQUIRE(n_blocks < ((int64_t)1 << 31), "axt_jpeg_encode_rgb8: %lld blocks of 8 x 8 pixels, the limit is 2^31 - 1",
                (long long)n_blocks);
    const JpegScratch s = jpeg_scratch_layout(d_scratch, n_frames, H, W);
    AXT_REQUIRE(scratch_bytes >= s.bytes, "axt_jpeg_encode_rgb8: scratch of %lld bytes, axt_jpeg_scratch_bytes asks for %lld",
                (long long)scratch_bytes, (long long)s.bytes);
    if (n_frames == 0) return AXT_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_items = n_blocks * 3;
    hipLaunchKernelGGL(jpeg_transform_k, dim3(jpeg_grid((n_items + kJpegThreads - 1) / kJpegThreads)), dim3(kJpegThreads), 0, st, d_rgb, H, W,
                       frame_stride, bh, bw, n_items, axt_jpeg_quant_tables(quality), s.coef, s.aclen);
    AXT_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_emit_k, dim3(jpeg_grid(n_rows)), dim3(kJpegThreads), 0, st, s.coef, s.aclen, bw, n_rows, s.raw, s.rowcap,
                       s.rowbits);
    AXT_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_count_k, dim3(jpeg_grid(n_rows)), dim3(kJpegThreads), 0, st, s.raw, s.rowcap, s.rowbits, n_rows, s.rowlen);
    AXT_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_offsets_k, dim3(jpeg_grid(n_frames)), dim3(kJpegThreads), 0, st, s.rowlen, bh, n_frames, scan_capacity, s.rowoff,
                       d_scan_bytes, d_status);
    AXT_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_pack_k, dim3(jpeg_grid(n_rows)), dim3(kJpegThreads), 0, st, s.raw, s.rowcap, s.rowbits, s.rowlen, s.rowoff,
                       d_status, bh, n_rows, d_scan, scan_capacity);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}
