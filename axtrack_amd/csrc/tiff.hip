// tiff.hip -- TIFF strips into the raw uint16 timelapse on gfx950: LZW, PackBits and uncompressed
// segments, byte swap and horizontal predictor, one wavefront per segment.
//
// The decoder itself is tiff_decode.h, shared with the host: a step reads one LZW code or one PackBits header, checks
// every range, and hands back one copy operation. Here the 64 lanes of a wave take the SAME steps -- the parse reads only
// wave-uniform addresses (the segment's input, the LZW table in LDS), so every lane holds the same state and nothing has
// to be broadcast -- and share each copy, lane i taking bytes i, i + 64, ... On sparse frames the strings run to
// hundreds of bytes, and that is where the parallelism is.
//
//   LDS        the LZW table, 4096 x (u32 offset, u16 length) = 24 KiB per block; every lane writes the same value to
//              the same entry and reads back its own write, so the table needs no barrier
//   output     an LZW string is copied from output that OTHER lanes of the wave wrote: before a copy whose source
//              reaches past `fenced`, the wave passes __syncthreads() (the block is one wave: a workgroup-scope release /
//              acquire) and `fenced` moves up to the output position. Literal codes and PackBits runs never need it.
//   rows       after the last step, one more fence, then every row of the segment is swapped to host order and, with
//              predictor 2, accumulated modulo 2^16 in place: a wave-wide inclusive scan per 64 samples, the running
//              sum carried from chunk to chunk. Uncompressed segments skip the decode and read the rows from the
//              input, byte by byte (strip offsets are odd in real files).
//   grid       min(n_segs, 2048) blocks of 64 threads, striding over the segments
//
// Every loop is bounded: axt_tiff_max_steps(compression, src_bytes) steps, each of which consumes input or ends.
// Bad data ends a segment with a status code; nothing traps, prints or retries.
#include "axt_common.h"
#include "tiff_decode.h"
#include "tiff_rows.h"

namespace {

__global__ __launch_bounds__(kTiffWave) void tiff_decode_k(const uint8_t *__restrict__ d_src, int64_t src_len,
                                                         const axt_tiff_segment *__restrict__ segs, int n_segs, int W,
                                                         int compression, int predictor, int big_endian, uint16_t *d_out,
                                                         int64_t out_len, int32_t *__restrict__ d_status)
{
    __shared__ uint32_t tbl_off[AXT_TIFF_LZW_ENTRIES];
    __shared__ uint16_t tbl_len[AXT_TIFF_LZW_ENTRIES];
    const int lane = threadIdx.x;
    for (int sg = blockIdx.x; sg < n_segs; sg += gridDim.x) {
        const axt_tiff_segment seg = segs[sg];
        int status = axt_tiff_check_segment(seg.src_offset, seg.src_bytes, seg.dst_offset, seg.rows, W, src_len, out_len);
        if (status == AXT_TIFF_OK) {
            const uint8_t *src = d_src + seg.src_offset;
            uint16_t *out = d_out + seg.dst_offset;
            uint8_t *bytes = reinterpret_cast<uint8_t *>(out);
            const uint32_t out_bytes = (uint32_t)seg.rows * (uint32_t)W * 2u;
            if (compression == AXT_TIFF_COMP_NONE) {
                if (seg.src_bytes < (int64_t)out_bytes) status = AXT_TIFF_SHORT_INPUT;
                else tiff_finish_rows(src, out, seg.rows, W, predictor, big_endian, lane);
            } else {
                axt_tiff_state s;
                axt_tiff_state_init(s);
                axt_tiff_op op;
                uint32_t fenced = 0;                                      // output below this is visible to every lane
                const int64_t steps = axt_tiff_max_steps(compression, seg.src_bytes);
                for (int64_t it = 0; it < steps && !s.done; ++it) {
                    if (compression == AXT_TIFF_COMP_LZW) axt_tiff_lzw_next(src, seg.src_bytes, out_bytes, s, tbl_off, tbl_len, op);
                    else axt_tiff_packbits_next(src, seg.src_bytes, out_bytes, s, op);
                    if (op.kind == AXT_TIFF_OP_FROM_OUTPUT) {
                        const uint32_t span = op.period < op.len ? op.period : op.len;
                        if ((uint32_t)op.src + span > fenced) {
                            __syncthreads();
                            fenced = op.dst;
                        }
                    }
                    axt_tiff_apply(op, src, bytes, (uint32_t)lane, (uint32_t)kTiffWave);
                }
                if (!s.done) axt_tiff_finish(s, s.out_pos >= out_bytes ? AXT_TIFF_OK : AXT_TIFF_SHORT_INPUT);
                status = s.status;
                if (status == AXT_TIFF_OK && (big_endian || predictor == 2)) {
                    __syncthreads();
                    tiff_finish_rows(bytes, out, seg.rows, W, predictor, big_endian, lane);
                }
            }
        }
        if (lane == 0) d_status[sg] = status;
        __syncthreads();                                                  // the next segment's table writes stay behind this one's reads
    }
}

}  // namespace

extern "C" int axt_tiff_decode_u16(const uint8_t *d_src, int64_t src_len, const axt_tiff_segment *d_segs, int n_segs, int W,
                                   int compression, int predictor, int big_endian, uint16_t *d_out, int64_t out_len,
                                   int32_t *d_status, void *stream)
{
    AXT_REQUIRE(d_src && d_segs && d_out && d_status, "axt_tiff_decode_u16: null argument");
    AXT_REQUIRE(src_len >= 0 && n_segs >= 0 && W >= 0 && out_len >= 0,
                "axt_tiff_decode_u16: negative size (src_len %lld, n_segs %d, W %d, out_len %lld)", (long long)src_len, n_segs, W,
                (long long)out_len);
    AXT_REQUIRE(compression == AXT_TIFF_COMP_NONE || compression == AXT_TIFF_COMP_LZW || compression == AXT_TIFF_COMP_PACKBITS,
                "axt_tiff_decode_u16: compression %d is not 1, 5 or 32773", compression);
    AXT_REQUIRE(predictor == 1 || predictor == 2, "axt_tiff_decode_u16: predictor %d is not 1 or 2", predictor);
    if (n_segs == 0) return AXT_OK;
    const int blocks = n_segs < kTiffMaxBlocks ? n_segs : kTiffMaxBlocks;
    hipLaunchKernelGGL(tiff_decode_k, dim3(blocks), dim3(kTiffWave), 0, (hipStream_t)stream, d_src, src_len, d_segs, n_segs, W,
                       compression, predictor, big_endian != 0, d_out, out_len, d_status);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}
