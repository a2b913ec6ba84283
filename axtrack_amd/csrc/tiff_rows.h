// tiff_rows.h -- what csrc/tiff.hip and csrc/tiff_inflate.hip share on the device: the launch shape
// (one wavefront per segment, at most 2048 blocks striding over the segments) and the row pass that ends every segment:
// each row swapped to host order and, with predictor 2, accumulated modulo 2^16, a wave-wide inclusive scan per 64
// samples with the running sum carried from chunk to chunk. `from` may be the segment's own output (in place) or its
// input at any byte address.
#pragma once
#include "tiff_decode.h"

namespace {

constexpr int kTiffWave = 64;
constexpr int kTiffMaxBlocks = 2048;

__device__ __forceinline__ void tiff_finish_rows(const uint8_t *from, uint16_t *out, int rows, int W, int predictor, int big_endian,
                                                 int lane)
{
    for (int r = 0; r < rows; ++r) {
        const size_t row = (size_t)r * W;
        uint16_t carry = 0;
        for (int x0 = 0; x0 < W; x0 += kTiffWave) {                        // (wave-uniform trip count: the shuffles are safe)
            const int x = x0 + lane;
            unsigned v = x < W ? axt_tiff_sample(from + (row + x) * 2, big_endian) : 0u;
            if (predictor == 2) {
                for (int d = 1; d < kTiffWave; d <<= 1) {
                    const unsigned up = __shfl_up(v, d, kTiffWave);
                    if (lane >= d) v += up;
                }
                v += carry;
                carry = (uint16_t)__shfl(v, kTiffWave - 1, kTiffWave);
            }
            if (x < W) out[row + x] = (uint16_t)v;
        }
    }
}

}  // namespace
