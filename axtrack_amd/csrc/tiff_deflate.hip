// tiff_deflate.hip -- the raw uint16 timelapse into Deflate TIFF strips on gfx950 ("TIFF output"): the
// mirror of tiff_inflate.hip, with its launch shape (tiff_rows.h): one wavefront per segment, min(n_segs, 2048) blocks of
// 64 threads striding over the segments.
//
// The encoder itself is tiff_deflate.h, shared with the host: the 64 lanes are its 64 workers. What is parallel there is
// parallel here -- the probes and match lengths of a batch of 64 positions, the frequency counts, the code lengths and
// canonical codes of a block's three code sets, the bit lengths and the emission of 64 tokens at a time, the copies of
// stored pieces and the Adler-32 --; the greedy cover of a batch, the repair walk over a code set and the run-length coding
// of a dynamic header are walked by all lanes alike from LDS, one lane writing.
//
//   LDS        axt_tiff_deflate_work: the hash table (16 KiB), the token buffer (16 KiB), the bit staging area (2 KiB),
//              frequencies, lengths, codes and the batch's candidates: 38.6 KiB a block
//   input      the strip's bytes are read from global memory where they are needed, predictor applied on load; the
//              window needs no ring: a position in the hash table is a position in the strip, and the strip stays put
//   output     whole bytes of the staging area, and the bytes of stored pieces, go to the slot as plain byte stores that
//              run along the lanes; nothing is read back
//
// axt_tiff_compact_streams: an exclusive scan of the streams' lengths by one block, then one block per stream copies it
// to its place.
#include "axt_common.h"
#include "axt_tiff_deflate.h"
#include "tiff_deflate.h"
#include "tiff_rows.h"

namespace {

constexpr int kCompactThreads = 256;

__global__ __launch_bounds__(kTiffWave) void tiff_deflate_k(const uint16_t *__restrict__ d_in, int64_t in_len,
                                                          const axt_tiff_segment *__restrict__ segs, int n_segs, int W,
                                                          int predictor, uint8_t *d_slots, int64_t slots_len,
                                                          int64_t *__restrict__ d_bytes, int32_t *__restrict__ d_status)
{
    __shared__ axt_tiff_deflate_work work;
    const int lane = threadIdx.x;
    for (int sg = blockIdx.x; sg < n_segs; sg += gridDim.x) {
        const axt_tiff_segment seg = segs[sg];
        // the descriptor's roles are reversed: src_* is the slot, dst_offset / rows the samples
        int status = axt_tiff_check_segment(seg.src_offset, seg.src_bytes, seg.dst_offset, seg.rows, W, slots_len, in_len);
        int64_t bytes = 0;
        if (status == AXT_TIFF_OK)
            status = axt_tiff_deflate_segment(d_in + seg.dst_offset, seg.rows, W, predictor, d_slots + seg.src_offset, seg.src_bytes, work,
                                              (uint32_t)lane, (uint32_t)kTiffWave, &bytes);
        if (lane == 0) {
            d_status[sg] = status;
            d_bytes[sg] = status == AXT_TIFF_OK ? bytes : 0;
        }
        __syncthreads();                                                  // the next segment's work area stays behind this one's reads
    }
}

// a stream's length as the gather takes it: 0 where it is not inside its slot
__device__ __forceinline__ int64_t compact_length(const axt_tiff_segment &seg, int64_t bytes)
{
    return bytes > 0 && seg.src_offset >= 0 && bytes <= seg.src_bytes ? bytes : 0;
}

// d_offsets[k] = the sum of the lengths before k, d_offsets[n_segs] = the sum of all. One block.
__global__ __launch_bounds__(kCompactThreads) void tiff_compact_scan_k(const axt_tiff_segment *__restrict__ segs,
                                                                     const int64_t *__restrict__ d_bytes, int n_segs,
                                                                     int64_t *__restrict__ d_offsets)
{
    __shared__ int64_t part[kCompactThreads];
    const int t = threadIdx.x;
    int64_t carry = 0;
    for (int k0 = 0; k0 < n_segs; k0 += kCompactThreads) {
        const int k = k0 + t;
        const int64_t v = k < n_segs ? compact_length(segs[k], d_bytes[k]) : 0;
        part[t] = v;
        __syncthreads();
        for (int d = 1; d < kCompactThreads; d <<= 1) {
            const int64_t up = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += up;
            __syncthreads();
        }
        if (k < n_segs) d_offsets[k] = carry + part[t] - v;
        carry += part[kCompactThreads - 1];
        __syncthreads();
    }
    if (t == 0) d_offsets[n_segs] = carry;
}

__global__ __launch_bounds__(kCompactThreads) void tiff_compact_gather_k(const uint8_t *__restrict__ d_slots,
                                                                       const axt_tiff_segment *__restrict__ segs,
                                                                       const int64_t *__restrict__ d_bytes, int n_segs,
                                                                       uint8_t *__restrict__ d_packed, int64_t packed_len,
                                                                       const int64_t *__restrict__ d_offsets)
{
    for (int sg = blockIdx.x; sg < n_segs; sg += gridDim.x) {
        const axt_tiff_segment seg = segs[sg];
        const int64_t n = compact_length(seg, d_bytes[sg]), at = d_offsets[sg];
        if (n > packed_len - at) continue;                                // does not fit: left out (the caller sees the total)
        const uint8_t *from = d_slots + seg.src_offset;
        for (int64_t i = threadIdx.x; i < n; i += kCompactThreads) d_packed[at + i] = from[i];
    }
}

}  // namespace

extern "C" int64_t axt_tiff_deflate_bound(int64_t raw_bytes)
{
    return axt_tiff_deflate_bound_bytes(raw_bytes < 0 ? 0 : raw_bytes);
}

extern "C" int axt_tiff_deflate_u16(const uint16_t *d_in, int64_t in_len, const axt_tiff_segment *d_segs, int n_segs, int W,
                                    int predictor, uint8_t *d_slots, int64_t slots_len, int64_t *d_bytes, int32_t *d_status,
                                    void *stream)
{
    AXT_REQUIRE(d_in && d_segs && d_slots && d_bytes && d_status, "axt_tiff_deflate_u16: null argument");
    AXT_REQUIRE(in_len >= 0 && n_segs >= 0 && W >= 0 && slots_len >= 0,
                "axt_tiff_deflate_u16: negative size (in_len %lld, n_segs %d, W %d, slots_len %lld)", (long long)in_len, n_segs, W,
                (long long)slots_len);
    AXT_REQUIRE(predictor == 1 || predictor == 2, "axt_tiff_deflate_u16: predictor %d is not 1 or 2", predictor);
    if (n_segs == 0) return AXT_OK;
    const int blocks = n_segs < kTiffMaxBlocks ? n_segs : kTiffMaxBlocks;
    hipLaunchKernelGGL(tiff_deflate_k, dim3(blocks), dim3(kTiffWave), 0, (hipStream_t)stream, d_in, in_len, d_segs, n_segs, W,
                       predictor, d_slots, slots_len, d_bytes, d_status);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

extern "C" int axt_tiff_compact_streams(const uint8_t *d_slots, const axt_tiff_segment *d_segs, const int64_t *d_bytes, int n_segs,
                                        uint8_t *d_packed, int64_t packed_len, int64_t *d_offsets, void *stream)
{
    AXT_REQUIRE(d_slots && d_segs && d_bytes && d_packed && d_offsets, "axt_tiff_compact_streams: null argument");
    AXT_REQUIRE(n_segs >= 0 && packed_len >= 0, "axt_tiff_compact_streams: negative size (n_segs %d, packed_len %lld)", n_segs,
                (long long)packed_len);
    if (n_segs == 0) return AXT_OK;
    hipLaunchKernelGGL(tiff_compact_scan_k, dim3(1), dim3(kCompactThreads), 0, (hipStream_t)stream, d_segs, d_bytes, n_segs, d_offsets);
    AXT_LAUNCH_CHECK();
    const int blocks = n_segs < kTiffMaxBlocks ? n_segs : kTiffMaxBlocks;
    hipLaunchKernelGGL(tiff_compact_gather_k, dim3(blocks), dim3(kCompactThreads), 0, (hipStream_t)stream, d_slots, d_segs, d_bytes,
                       n_segs, d_packed, packed_len, d_offsets);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}
