"""Rendered frames as baseline JPEGs, encoded on the GPU (axt_jpeg_encode_rgb8, csrc/jpeg.hip), and an MJPEG AVI writer:
the video of a tracking result that ImageJ / Fiji, VLC and ffmpeg-based tools open. DESIGN.md 6.8i states the format --
SOF0, 8 bit, Y Cb Cr 4:4:4, the Annex K tables, a restart interval of one MCU row -- and csrc/jpeg_encode.h the encoder's
integer arithmetic. The device writes every frame's entropy-coded segment; the header, the same for every frame of a
video, is built here once, and only compressed bytes cross to the host."""
import struct

import numpy as np
import torch

from . import hotpath as hp
from .render import _delay

# position in the 8 x 8 block (natural order) of the k-th coefficient in zigzag order
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# ITU-T T.81 Annex K.1 / K.2, natural order
BASE_QUANT = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
     103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99)
    + (99,) * 32)
# Annex K.3 - K.6: (table class << 4 | destination, the number of codes of each length 1..16, the symbols in code order)
HUFFMAN = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
     (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
      36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
      73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131,
      132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
      178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216,
      217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250)),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
     (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
      21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71,
      72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130,
      131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169,
      170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215,
      216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250)),
)
EOI = b'\xff\xd9'
AVI_MAX_BYTES = (1 << 31) - 1
_SCRATCH_BYTES_PER_CALL = 2 << 30        # render_inference's chunk of 256 MB of RGB takes 1.4 GB: one call


def quant_tables(quality):
    """The luminance and the chrominance table at `quality` (1..100), natural order: uint8 [2, 64]. IJG scaling:
    s = 5000 / q below 50, else 200 - 2 q; entry clamp((base s + 50) / 100, 1, 255), integer division."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f'quality must lie in 1..100, got {quality!r}')
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.array(BASE_QUANT, np.int64) * s + 50) // 100, 1, 255).astype(np.uint8)


def _segment(marker, payload):
    return struct.pack('>BBH', 0xFF, marker, len(payload) + 2) + payload


def jpeg_header(H, W, quality=90):
    """SOI through SOS: JFIF APP0, the two DQT, SOF0 (three components, each 1 x 1), the four DHT, DRI (one MCU row),
    SOS. A frame's file is this, its scan segment, and EOI."""
    H, W = int(H), int(W)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f'a JPEG frame is 1..65535 pixels a side, got {H} x {W}')
    qt = quant_tables(quality)
    out = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00' + struct.pack('>BBBHHBB', 1, 1, 0, 1, 1, 0, 0))]
    for k in range(2):
        out.append(_segment(0xDB, bytes([k]) + bytes(int(qt[k][n]) for n in ZIGZAG)))
    out.append(_segment(0xC0, struct.pack('>BHHB', 8, H, W, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for ident, bits, vals in HUFFMAN:
        out.append(_segment(0xC4, bytes([ident]) + bytes(bits) + bytes(vals)))
    out.append(_segment(0xDD, struct.pack('>H', -(-W // 8))))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b''.join(out)


def jpeg_encode(rgb, quality=90, _first_capacity=None):
    """A device uint8 [N, H, W, 3] (or [H, W, 3]) tensor as N baseline JPEG files: a list of bytes, each header + scan
    segment + EOI. The frames are encoded on the tensor's device in calls of at most 2 GiB of scratch; a frame's slot
    starts at the raw size of the frame, and a call with a frame that does not fit (status 1: incompressible content at
    a high quality) is repeated with slots of axt_jpeg_scan_bound. Only the bytes each frame uses are copied to the host."""
    if not (isinstance(rgb, torch.Tensor) and rgb.dtype == torch.uint8 and rgb.dim() in (3, 4) and rgb.shape[-1] == 3):
        raise TypeError('jpeg_encode takes a uint8 tensor [N, H, W, 3] or [H, W, 3]')
    if not rgb.is_cuda:
        raise ValueError('jpeg_encode takes a tensor on the GPU; there is no CPU path')
    if rgb.dim() == 3:
        rgb = rgb[None]
    N, H, W, _ = rgb.shape
    header = jpeg_header(H, W, quality)
    if N == 0:
        return []
    if not rgb[0].is_contiguous() or (N > 1 and rgb.stride(0) < 3 * H * W):
        rgb = rgb.contiguous()
    dev = rgb.device
    bound = hp.jpeg_scan_bound(H, W)
    first = min(bound, max(3 * H * W, 256) if _first_capacity is None else int(_first_capacity))
    per = max(1, _SCRATCH_BYTES_PER_CALL // hp.jpeg_scratch_bytes(1, H, W))
    out = []
    with torch.cuda.device(dev):
        for a in range(0, N, per):
            part = rgb[a:a + per]
            n = part.shape[0]
            scratch = torch.empty(hp.jpeg_scratch_bytes(n, H, W), dtype=torch.uint8, device=dev)
            counts = torch.empty(n, dtype=torch.int64, device=dev)
            status = torch.empty(n, dtype=torch.int32, device=dev)
            for capacity in (first, bound):
                scan = torch.empty((n, capacity), dtype=torch.uint8, device=dev)
                hp.jpeg_encode_launch(part, quality, scan, counts, status, scratch)
                used = counts.cpu().numpy()
                if not status.cpu().numpy().any():
                    break
                if capacity == bound:
                    raise RuntimeError(f'axt_jpeg_encode_rgb8: a frame needs {int(used.max())} bytes, above its bound {bound}')
            flat = torch.cat([scan[i, :int(used[i])] for i in range(n)]).cpu().numpy().tobytes()
            o = 0
            for i in range(n):
                out.append(header + flat[o:o + int(used[i])] + EOI)
                o += int(used[i])
    return out


def _riff_chunk(kind, data):
    return kind + struct.pack('<I', len(data)) + data + (b'\x00' if len(data) & 1 else b'')


def _riff_list(kind, body):
    return b'LIST' + struct.pack('<I', 4 + len(body)) + kind + body


def write_mjpeg_avi(path, jpegs, H, W, fps=6):
    """The JPEG files `jpegs` (each H x W) as the frames of a RIFF AVI 1.0 video at fps frames per second: hdrl with avih
    and one strl (strh 'vids' / 'MJPG', strf a 24-bit BITMAPINFOHEADER), movi with one '00dc' chunk per frame, padded to
    even length, and idx1 with every chunk's offset (from the 'movi' tag) and size, each a key frame. AVI 1.0 ends at
    2^31 - 1 bytes; a larger video is refused. Returns path."""
    n = len(jpegs)
    sizes = [len(j) for j in jpegs]
    movi_bytes = 4 + sum(8 + s + (s & 1) for s in sizes)
    scale, rate = _delay(fps)                                        # fps = rate / scale, the rational of the APNG's delay
    H, W = int(H), int(W)
    biggest = max(sizes, default=0)
    avih = struct.pack('<14I', int(round(1e6 * scale / rate)), int(biggest * rate / scale) + 1, 0, 0x10, n, 0, 1, biggest, W, H,
                       0, 0, 0, 0)
    strh = b'vids' + b'MJPG' + struct.pack('<IHHIIIIIIiI4H', 0, 0, 0, 0, scale, rate, 0, n, biggest, -1, 0, 0, 0, W, H)
    strf = struct.pack('<IiiHH4sIiiII', 40, W, H, 1, 24, b'MJPG', 3 * W * H, 0, 0, 0, 0)
    hdrl = _riff_list(b'hdrl', _riff_chunk(b'avih', avih) + _riff_list(b'strl', _riff_chunk(b'strh', strh) + _riff_chunk(b'strf', strf)))
    total = 12 + len(hdrl) + 8 + movi_bytes + 8 + 16 * n
    if total > AVI_MAX_BYTES:
        raise ValueError(f'the video would take {total} bytes, beyond the {AVI_MAX_BYTES} of an AVI 1.0 file: render a part '
                         f'of the timelapse (t_y_x_slice) or lower the quality')
    index, offset = [], 4
    for s in sizes:
        index.append(b'00dc' + struct.pack('<III', 0x10, offset, s))
        offset += 8 + s + (s & 1)
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', total - 8) + b'AVI ' + hdrl + b'LIST' + struct.pack('<I', movi_bytes) + b'movi')
        for j in jpegs:
            f.write(_riff_chunk(b'00dc', bytes(j)))
        f.write(b'idx1' + struct.pack('<I', 16 * n) + b''.join(index))
    return path
