/* axtrack_hip_tiff.h -- included by axtrack_hip.h; not for inclusion on its own. Same conventions: AXT_OK or a negative
 * AXT_E* code, axt_last_error() for the text, `stream` a hipStream_t. */
#ifndef AXTRACK_HIP_TIFF_H
#define AXTRACK_HIP_TIFF_H

/* ------------------------------------------------------------------------------------------
 * TIFF strips decoded on the device (csrc/tiff.hip, csrc/tiff_decode.h).
 *
 * The host parses the container (axtrack_amd/tiff.py) and copies the strips' bytes, still compressed, into d_src
 * [src_len bytes]. A segment is one strip: its bytes [src_offset, src_offset + src_bytes) of d_src hold `rows` rows of W
 * 16-bit samples, which go to d_out [out_len uint16] from element dst_offset on, in host byte order and with the
 * predictor undone. `reserved` is ignored.
 *
 *   compression  1      none: the rows are gathered into place (the source may start at any byte address)
 *                5      LZW, the TIFF variant: codes most significant bit first, 9 to 12 bits, the width growing one code
 *                       early (when the next free entry + 1 reaches 2^width), Clear 256, EndOfInformation 257
 *                32773  PackBits: header n in 0..127 copies n + 1 bytes, n in -127..-1 repeats the next byte 1 - n times,
 *                       -128 does nothing
 *   predictor    1 none, 2 horizontal differencing of the 16-bit samples (undone after the byte swap, modulo 2^16)
 *   big_endian   != 0: the samples are stored most significant byte first
 *
 * d_status [n_segs] receives per segment
 *   0  ok
 *   1  input exhausted (or EndOfInformation) before rows * W samples were produced
 *   2  invalid code: an LZW code above the next free entry, a first code after Clear that is no literal, a full table
 *   3  the next string or run would overrun the segment's rows * W samples
 *   4  descriptor out of range: a negative field, src_offset + src_bytes > src_len, dst_offset + rows * W > out_len, or
 *      rows * W >= 2^31
 * A failing segment leaves its own rows * W samples unspecified and touches nothing else; with status 4 it touches
 * nothing at all. A segment whose output is complete stops there, whether or not its input goes on. Segments must not
 * overlap in d_out. One wavefront decodes one segment; every loop is bounded by the segment's src_bytes, no read falls
 * outside the segment's input and no write outside its output.
 *
 * Asynchronous on `stream`, no copy to or from the host, no allocation. A null pointer, a negative size, a compression
 * other than 1, 5, 32773 or a predictor other than 1, 2: AXT_EINVAL with the function's name in axt_last_error(), before
 * any launch. n_segs == 0 launches nothing.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int64_t src_offset, src_bytes;
    int64_t dst_offset;                 /* in uint16 elements of d_out */
    int32_t rows, reserved;
} axt_tiff_segment;

int axt_tiff_decode_u16(const uint8_t *d_src, int64_t src_len, const axt_tiff_segment *d_segs, int n_segs, int W,
                        int compression, int predictor, int big_endian, uint16_t *d_out, int64_t out_len, int32_t *d_status,
                        void *stream);

#endif
