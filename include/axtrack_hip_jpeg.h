/* axtrack_hip_jpeg.h -- included by axtrack_hip.h; not for inclusion on its own. Same conventions: AXT_OK or a negative
 * AXT_E* code, axt_last_error() for the text, `stream` a hipStream_t. */
#ifndef AXTRACK_HIP_JPEG_H
#define AXTRACK_HIP_JPEG_H

/* ------------------------------------------------------------------------------------------
 * RGB frames JPEG-encoded on the device (csrc/jpeg.hip, csrc/jpeg_encode.h).
 *
 * Baseline sequential JPEG (SOF0), 8 bit, Y Cb Cr at 4:4:4, the Annex K quantisation tables scaled by `quality` (1..100,
 * the IJG rule) and the Annex K Huffman tables, a restart interval of one MCU row (ceil(W / 8) MCUs). The device writes
 * only the entropy-coded segment of every frame -- what stands between the SOS header and EOI, the RSTm markers between
 * the MCU rows included; the header is the same for every frame and is the host's (axtrack_amd/jpeg.py: jpeg_header).
 * csrc/jpeg_encode.h states the arithmetic, all of it in integers; the bytes are a function of the pixels alone.
 *
 * d_rgb: n_frames frames of uint8 [H][W][3], frame i at d_rgb + i * frame_stride (bytes, >= 3 * H * W). d_scan: n_frames
 * slots of scan_capacity bytes. d_scan_bytes [n_frames] receives the bytes each frame's segment takes, d_status
 * [n_frames] 0, or 1 for a frame whose segment does not fit its slot: d_scan_bytes then says what it needs
 * (axt_jpeg_scan_bound(H, W) always suffices), the slot's content is unspecified, and nothing outside it is touched. No
 * byte at or beyond a frame's count is written.
 *
 * d_scratch: axt_jpeg_scratch_bytes(n_frames, H, W) bytes, 16-byte aligned, the caller's; its content afterwards is
 * unspecified. About 1000 bytes per 8 x 8 pixels (the coefficients, and a row buffer sized for the worst case).
 *
 * Asynchronous on `stream`, no copy to or from the host, no allocation. A null pointer, a negative size, H or W outside
 * 1..65535, a quality outside 1..100, frame_stride < 3 * H * W, scratch that is smaller than the query or misaligned,
 * n_frames * ceil(H / 8) * ceil(W / 8) >= 2^31: AXT_EINVAL with the function's name in axt_last_error(), before any
 * device call. n_frames == 0 launches nothing. The two queries answer AXT_EINVAL (negative) for sizes out of range.
 * ------------------------------------------------------------------------------------------ */
int64_t axt_jpeg_scan_bound(int H, int W);
int64_t axt_jpeg_scratch_bytes(int n_frames, int H, int W);
int axt_jpeg_encode_rgb8(const uint8_t *d_rgb, int n_frames, int H, int W, int64_t frame_stride, int quality, uint8_t *d_scan,
                         int64_t scan_capacity, int64_t *d_scan_bytes, int32_t *d_status, void *d_scratch, int64_t scratch_bytes,
                         void *stream);

#endif
