/* axt_tiff_deflate.h -- the writing companion of csrc/axt_tiff_inflate.h, exported from libaxtrack_hip.so and bound by
 * axtrack_amd/_lib.py (INTERNAL_SIGNATURES), but not yet part of the public ABI under include/ (DESIGN.md 6.8h says what
 * moving it there takes). Same conventions: AXT_OK or a negative AXT_E* code, axt_last_error() for the text, `stream` a
 * hipStream_t. */
#ifndef AXT_TIFF_DEFLATE_H
#define AXT_TIFF_DEFLATE_H

#include "../../include/axtrack_hip.h"

/* ------------------------------------------------------------------------------------------
 * Strips of a raw uint16 timelapse deflated on the device (DESIGN.md 6.8h "TIFF output", csrc/tiff_deflate.hip,
 * csrc/tiff_deflate.h).
 *
 * The samples are in d_in [in_len uint16]. A segment is one strip, and the roles of axt_tiff_segment's fields are those
 * of the decoders REVERSED:
 *   dst_offset, rows       name the strip's samples: `rows` rows of W samples from element dst_offset of d_in on
 *   src_offset, src_bytes  name the slot in d_slots [slots_len bytes] that receives the stream, and its capacity
 *   reserved               is ignored
 * The stream is one zlib stream (RFC 1950: header 0x78 0x01, Deflate blocks of RFC 1951 -- stored, fixed or dynamic,
 * whichever is smallest for the block --, the Adler-32 of the bytes as stored) of the strip's samples, little-endian,
 * with the predictor applied:
 *   predictor    1 none, 2 horizontal differencing of the 16-bit samples, modulo 2^16
 * It is a function of the strip's samples alone (the parse is stated in csrc/tiff_deflate.h), and never longer than
 * axt_tiff_deflate_bound(2 * rows * W) = raw + 5 * max(1, ceil(raw / 65535)) + 6, the all-stored stream.
 *
 * d_bytes [n_segs] receives the stream's length (0 for a failing segment), d_status [n_segs] per segment
 *   0  ok
 *   3  the stream would overrun its slot (never with a slot of axt_tiff_deflate_bound bytes)
 *   4  descriptor out of range: a negative field, src_offset + src_bytes > slots_len, dst_offset + rows * W > in_len, or
 *      rows * W >= 2^31
 * A failing segment leaves its own slot unspecified and touches nothing else; with status 4 it touches nothing at all.
 * Slots must not overlap. One wavefront deflates one segment; every loop is bounded by the segment's rows * W, no read
 * falls outside the segment's samples and no write outside its slot.
 *
 * axt_tiff_compact_streams puts the streams back to back in segment order: d_offsets [n_segs + 1] receives the exclusive
 * scan of the lengths and, last, their sum; stream k goes to d_packed [packed_len bytes] from d_offsets[k] on. A segment
 * with d_bytes[k] <= 0 (a failing one), or with a length that is not inside its slot, counts as empty and is left out. A
 * stream that would pass packed_len is not copied; the caller sees it from d_offsets[n_segs] > packed_len.
 *
 * All calls are asynchronous on `stream`, no copy to or from the host, no allocation. A null pointer, a negative size or
 * a predictor other than 1, 2: AXT_EINVAL with the function's name in axt_last_error(), before any launch. n_segs == 0
 * launches nothing. axt_tiff_deflate_bound is plain arithmetic (a negative size counts as 0).
 * ------------------------------------------------------------------------------------------ */
#ifdef __cplusplus
extern "C" {
#endif

int64_t axt_tiff_deflate_bound(int64_t raw_bytes);
int axt_tiff_deflate_u16(const uint16_t *d_in, int64_t in_len, const axt_tiff_segment *d_segs, int n_segs, int W, int predictor,
                         uint8_t *d_slots, int64_t slots_len, int64_t *d_bytes, int32_t *d_status, void *stream);
int axt_tiff_compact_streams(const uint8_t *d_slots, const axt_tiff_segment *d_segs, const int64_t *d_bytes, int n_segs,
                             uint8_t *d_packed, int64_t packed_len, int64_t *d_offsets, void *stream);

#ifdef __cplusplus
}
#endif

#endif
