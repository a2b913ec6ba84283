/* axt_tiff_inflate.h -- the Deflate companion of include/axtrack_hip_tiff.h, exported from libaxtrack_hip.so and bound by
 * axtrack_amd/_lib.py (INTERNAL_SIGNATURES), but not yet part of the public ABI under include/ (DESIGN.md 6.8h says what
 * moving it there takes). Same conventions: AXT_OK or a negative AXT_E* code, axt_last_error() for the text, `stream` a
 * hipStream_t. */
#ifndef AXT_TIFF_INFLATE_H
#define AXT_TIFF_INFLATE_H

#include "../../include/axtrack_hip.h"

/* ------------------------------------------------------------------------------------------
 * Deflate TIFF strips (Compression 8 and 32946) inflated on the device (csrc/tiff_inflate.hip,
 * csrc/tiff_inflate.h).
 *
 * The arguments are those of axt_tiff_decode_u16 without `compression`: the strips' bytes, still compressed, in d_src
 * [src_len bytes]; a segment is one strip, a zlib stream (RFC 1950: the 2-byte header, Deflate blocks of RFC 1951 --
 * stored, fixed and dynamic --, the Adler-32 of the uncompressed bytes) whose bytes [src_offset, src_offset + src_bytes)
 * hold `rows` rows of W 16-bit samples. They go to d_out [out_len uint16] from element dst_offset on, in host byte order
 * and with the predictor undone. `reserved` is ignored.
 *
 *   predictor    1 none, 2 horizontal differencing of the 16-bit samples (undone after the byte swap, modulo 2^16)
 *   big_endian   != 0: the samples are stored most significant byte first
 *
 * d_status [n_segs] receives per segment
 *   0  ok
 *   1  input exhausted before the final block ended, before the four bytes of the checksum were read, or the stream
 *      ends before rows * W samples were produced
 *   2  invalid stream: a header that is not CM 8 / CINFO <= 7 / check bits / no preset dictionary, block type 3, LEN and
 *      NLEN that do not match, a code set zlib's inflate refuses (HLIT > 286, HDIST > 30, a repeat without a previous
 *      length or past the end, no end-of-block code, over-subscribed, incomplete other than one single 1-bit code),
 *      literal/length symbol 286 / 287, distance symbol 30 / 31, a bit pattern that is no code of an incomplete set, a
 *      distance that reaches before the strip's first output byte
 *   3  a literal, match or stored block would overrun the segment's rows * W samples (also behind the complete output:
 *      only end-of-block codes and blocks without output may follow it)
 *   4  descriptor out of range: a negative field, src_offset + src_bytes > src_len, dst_offset + rows * W > out_len, or
 *      rows * W >= 2^31
 *   5  checksum: the stream's Adler-32 is not that of the bytes produced
 * Unlike the codecs of axt_tiff_decode_u16, a segment whose output is complete is read on to the end of its stream and
 * its checksum, the format's only integrity check; bytes behind the checksum are ignored. A failing segment leaves its
 * own rows * W samples unspecified and touches nothing else; with status 4 it touches nothing at all. Segments must not
 * overlap in d_out. One wavefront inflates one segment; every loop is bounded by the segment's src_bytes, no read falls
 * outside the segment's input and no write outside its output.
 *
 * Asynchronous on `stream`, no copy to or from the host, no allocation. A null pointer, a negative size or a predictor
 * other than 1, 2: AXT_EINVAL with the function's name in axt_last_error(), before any launch. n_segs == 0 launches
 * nothing.
 * ------------------------------------------------------------------------------------------ */
#ifdef __cplusplus
extern "C" {
#endif

int axt_tiff_inflate_u16(const uint8_t *d_src, int64_t src_len, const axt_tiff_segment *d_segs, int n_segs, int W,
                         int predictor, int big_endian, uint16_t *d_out, int64_t out_len, int32_t *d_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
