// tiff_inflate.hip -- Deflate TIFF strips into the raw uint16 timelapse on gfx950: one wavefront per
// segment, the launch shape and the row pass of tiff.hip (tiff_rows.h).
//
// The inflater itself is tiff_inflate.h, shared with the host: a step reads the stream header, a block header, one
// symbol or the trailer, checks every range, and hands back one copy operation. The 64 lanes of a wave take the SAME
// steps -- the parse reads only wave-uniform addresses (the segment's input, the tables in LDS), so every lane holds the
// same state and nothing is broadcast -- and share what is parallel: building a block's lookup tables from its code
// lengths, the copies, the Adler-32, and the row pass.
//
//   LDS        the tables of tiff_inflate.h (about 5 KiB) and a ring of the last 32 KiB of the segment's output, the
//              Deflate window. Every produced byte goes into the ring; a match (FROM_OUTPUT) is served from the ring, so
//              a back-reference costs a workgroup barrier on LDS (the block is one wave) and never a store-to-load
//              round trip through global memory.
//   output     the ring is flushed to global memory 16 KiB at a time, as 2-byte stores that run along the lanes and that
//              nothing waits for. A stored block goes through the ring in pieces of 8 KiB. The flush also sums the
//              Adler-32: every output byte passes it exactly once, with its position.
//   ring       byte p of the output stands at ring[p % 32768]. A match of distance 32768 reads and writes the same
//              slots (a no-op in the ring); one of a distance just below it overwrites source bytes only after the pass
//              of 64 lanes that read them. Nothing not yet flushed is overwritten: at most 16 KiB + 8 KiB stand unflushed.
//   rows       after the last flush, one fence, then the checksum is compared and the rows are swapped / accumulated
//              in place where the file asks for it.
//   grid       min(n_segs, 2048) blocks of 64 threads, striding over the segments
//
// Every loop is bounded: axt_tiff_inflate_max_steps(src_bytes) steps, each of which consumes input or ends.
// Bad data ends a segment with a status code; nothing traps, prints or retries.
#include "axt_common.h"
#include "axt_tiff_inflate.h"
#include "tiff_inflate.h"
#include "tiff_rows.h"

namespace {

constexpr uint32_t kRing = AXT_INF_WINDOW, kRingMask = kRing - 1;
constexpr uint32_t kFlushAt = 16384;                        // unflushed bytes that trigger a flush
constexpr uint32_t kStoredPiece = 8192;                     // a stored block enters the ring in pieces of this size

struct InflateSums {
    uint64_t a, b;                                          // this lane's share of the Adler-32 sums
};

// Output bytes [from, to), both even, from the ring to global memory; the lanes' Adler sums take them in.
__device__ __forceinline__ void inflate_flush(const uint8_t *ring, uint16_t *out, uint32_t from, uint32_t to, uint32_t out_bytes,
                                              InflateSums &sums, int lane)
{
    __syncthreads();                                                      // the ring's writers are other lanes
    for (uint32_t i = from / 2 + lane; i < to / 2; i += kTiffWave) {
        const uint32_t v = *reinterpret_cast<const uint16_t *>(ring + ((2 * i) & kRingMask));
        out[i] = (uint16_t)v;
        const uint32_t lo = v & 255, hi = v >> 8;                         // bytes 2 i and 2 i + 1
        sums.a += lo + hi;
        sums.b += (uint64_t)(out_bytes - 2 * i) * lo + (uint64_t)(out_bytes - 2 * i - 1) * hi;
    }
    sums.b %= AXT_INF_ADLER_MOD;                                          // (at most 192 turns of < 2^41 since the last)
}

__global__ __launch_bounds__(kTiffWave) void tiff_inflate_k(const uint8_t *__restrict__ d_src, int64_t src_len,
                                                          const axt_tiff_segment *__restrict__ segs, int n_segs, int W,
                                                          int predictor, int big_endian, uint16_t *d_out, int64_t out_len,
                                                          int32_t *__restrict__ d_status)
{
    __shared__ axt_tiff_inflate_tables tables;
    __shared__ __attribute__((aligned(16))) uint8_t ring[kRing];
    const int lane = threadIdx.x;
    for (int sg = blockIdx.x; sg < n_segs; sg += gridDim.x) {
        const axt_tiff_segment seg = segs[sg];
        int status = axt_tiff_check_segment(seg.src_offset, seg.src_bytes, seg.dst_offset, seg.rows, W, src_len, out_len);
        if (status == AXT_TIFF_OK) {
            const uint8_t *src = d_src + seg.src_offset;
            uint16_t *out = d_out + seg.dst_offset;
            const uint32_t out_bytes = (uint32_t)seg.rows * (uint32_t)W * 2u;
            axt_tiff_inflate_state s;
            axt_tiff_inflate_init(s);
            axt_tiff_op op;
            InflateSums sums = {0, 0};
            uint32_t flushed = 0;                                         // even; output below it is in global memory
            const int64_t steps = axt_tiff_inflate_max_steps(seg.src_bytes);
            for (int64_t it = 0; it < steps && !s.done; ++it) {
                axt_tiff_inflate_next(src, seg.src_bytes, out_bytes, s, tables, op, (uint32_t)lane, (uint32_t)kTiffWave);
                if (op.kind == AXT_TIFF_OP_NONE) continue;
                // (op.dst + op.len <= out_bytes: the step has checked it)
                for (uint32_t p = 0; p < op.len; p += kStoredPiece) {     // one turn, except for a stored block
                    const uint32_t dst = op.dst + p, n = op.len - p < kStoredPiece ? op.len - p : kStoredPiece;
                    if (dst + n - flushed > kFlushAt) {
                        inflate_flush(ring, out, flushed, dst & ~1u, out_bytes, sums, lane);
                        flushed = dst & ~1u;
                    }
                    if (op.kind == AXT_TIFF_OP_FILL) {
                        if (lane == 0) ring[dst & kRingMask] = (uint8_t)op.src;
                    } else if (op.kind == AXT_TIFF_OP_FROM_INPUT) {
                        for (uint32_t i = lane; i < n; i += kTiffWave) ring[(dst + i) & kRingMask] = src[op.src + p + i];
                    } else {
                        __syncthreads();                                  // the match's source: other lanes' ring writes
                        const uint32_t from = (uint32_t)op.src;
                        if (op.period >= n) {
                            for (uint32_t i = lane; i < n; i += kTiffWave) ring[(dst + i) & kRingMask] = ring[(from + i) & kRingMask];
                        } else {
                            for (uint32_t i = lane; i < n; i += kTiffWave)
                                ring[(dst + i) & kRingMask] = ring[(from + i % op.period) & kRingMask];
                        }
                    }
                }
            }
            if (!s.done) axt_tiff_inflate_finish(s, AXT_TIFF_SHORT_INPUT);
            status = s.status;
            if (status == AXT_TIFF_OK) {                                  // (out_pos == out_bytes: the trailer step requires it)
                inflate_flush(ring, out, flushed, out_bytes, out_bytes, sums, lane);
                uint32_t a = (uint32_t)(sums.a % AXT_INF_ADLER_MOD), b = (uint32_t)(sums.b % AXT_INF_ADLER_MOD);
                for (int d = 1; d < kTiffWave; d <<= 1) {                 // (64 terms below 65521 each: no wrap)
                    a += __shfl_xor(a, d, kTiffWave);
                    b += __shfl_xor(b, d, kTiffWave);
                }
                if (axt_tiff_adler_value(a, b, out_bytes) != s.adler) {
                    status = AXT_TIFF_BAD_CHECKSUM;
                } else if (big_endian || predictor == 2) {
                    __syncthreads();                                      // the flushed bytes of other lanes
                    tiff_finish_rows(reinterpret_cast<const uint8_t *>(out), out, seg.rows, W, predictor, big_endian, lane);
                }
            }
        }
        if (lane == 0) d_status[sg] = status;
        __syncthreads();                                                  // the next segment's ring and tables stay behind this one's reads
    }
}

}  // namespace

extern "C" int axt_tiff_inflate_u16(const uint8_t *d_src, int64_t src_len, const axt_tiff_segment *d_segs, int n_segs, int W,
                                    int predictor, int big_endian, uint16_t *d_out, int64_t out_len, int32_t *d_status,
                                    void *stream)
{
    AXT_REQUIRE(d_src && d_segs && d_out && d_status, "axt_tiff_inflate_u16: null argument");
    AXT_REQUIRE(src_len >= 0 && n_segs >= 0 && W >= 0 && out_len >= 0,
                "axt_tiff_inflate_u16: negative size (src_len %lld, n_segs %d, W %d, out_len %lld)", (long long)src_len, n_segs, W,
                (long long)out_len);
    AXT_REQUIRE(predictor == 1 || predictor == 2, "axt_tiff_inflate_u16: predictor %d is not 1 or 2", predictor);
    if (n_segs == 0) return AXT_OK;
    const int blocks = n_segs < kTiffMaxBlocks ? n_segs : kTiffMaxBlocks;
    hipLaunchKernelGGL(tiff_inflate_k, dim3(blocks), dim3(kTiffWave), 0, (hipStream_t)stream, d_src, src_len, d_segs, n_segs, W,
                       predictor, big_endian != 0, d_out, out_len, d_status);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}
