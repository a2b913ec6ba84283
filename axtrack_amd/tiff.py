"""TIFF timelapses without a third-party reader: the container is parsed here on the host with struct /
numpy over a memory map, the strips are decoded on the GPU (csrc/tiff.hip, and csrc/tiff_inflate.hip for Deflate, through
hotpath.tiff_decode_u16). The one place where the host still decodes pixel data is a pack of fewer than
INFLATE_ON_DEVICE_FROM Deflate strips, where one core running zlib is measurably faster (inflate_on_device).

    info = tiff_info(path)            shape, byte order, compression, predictor and the segment table; reads tags only
    raw  = read_tiff(path)            the stack on the device as int16-viewed uint16 [T,H,W] (what _raw_on_device hands on)
    write_tiff(path, stack)           the stack as a Deflate TIFF, its strips deflated on the GPU (csrc/tiff_deflate.hip); the
                                      container (TiffWriter, build_ifd) is written here on the host

Supported: classic TIFF and BigTIFF, both byte orders, strips, one 16-bit unsigned grayscale plane per page, compression
none / PackBits / LZW / Deflate, predictor none / horizontal, and ImageJ's single-IFD hyperstacks. Anything else raises
TiffUnsupported naming the tag and its value; a truncated or inconsistent file raises TiffError naming the offset."""
import struct
import zlib

import numpy as np

COMPRESSION_NONE, COMPRESSION_LZW, COMPRESSION_DEFLATE, COMPRESSION_ADOBE_DEFLATE, COMPRESSION_PACKBITS = 1, 5, 32946, 8, 32773
DEFLATE = (COMPRESSION_ADOBE_DEFLATE, COMPRESSION_DEFLATE)
SUPPORTED_COMPRESSION = (COMPRESSION_NONE, COMPRESSION_LZW, COMPRESSION_PACKBITS) + DEFLATE
CHUNK_FRAMES = 64                                    # read_tiff packs, copies and decodes at most this many frames at a time
INFLATE_ON_DEVICE_FROM = 64                          # strips in a pack from which Deflate is inflated on the device (inflate_on_device)
DEFLATE_ON_DEVICE_FROM = 64                          # strips in a chunk from which write_tiff deflates on the device (deflate_on_device)

# tag numbers (TIFF 6.0)
NEW_SUBFILE_TYPE, IMAGE_WIDTH, IMAGE_LENGTH, BITS_PER_SAMPLE, COMPRESSION, PHOTOMETRIC = 254, 256, 257, 258, 259, 262
IMAGE_DESCRIPTION, STRIP_OFFSETS, SAMPLES_PER_PIXEL, ROWS_PER_STRIP, STRIP_BYTE_COUNTS = 270, 273, 277, 278, 279
PLANAR_CONFIGURATION, PREDICTOR, TILE_WIDTH, TILE_LENGTH, TILE_OFFSETS, TILE_BYTE_COUNTS, SAMPLE_FORMAT = 284, 317, 322, 323, 324, 325, 339
TAG_NAMES = {254: 'NewSubfileType', 256: 'ImageWidth', 257: 'ImageLength', 258: 'BitsPerSample', 259: 'Compression',
             262: 'PhotometricInterpretation', 270: 'ImageDescription', 273: 'StripOffsets', 277: 'SamplesPerPixel',
             278: 'RowsPerStrip', 279: 'StripByteCounts', 284: 'PlanarConfiguration', 317: 'Predictor', 322: 'TileWidth',
             323: 'TileLength', 324: 'TileOffsets', 325: 'TileByteCounts', 339: 'SampleFormat'}
# field type -> (struct letter, bytes)
FIELD_TYPES = {1: ('B', 1), 2: ('c', 1), 3: ('H', 2), 4: ('I', 4), 5: ('II', 8), 6: ('b', 1), 7: ('B', 1), 8: ('h', 2),
               9: ('i', 4), 10: ('ii', 8), 11: ('f', 4), 12: ('d', 8), 13: ('I', 4), 16: ('Q', 8), 17: ('q', 8), 18: ('Q', 8)}
_INTEGER_TYPES = (1, 3, 4, 6, 8, 9, 13, 16, 17, 18)
MAX_IFD_ENTRIES = 4096
# axt_tiff_segment (include/axtrack_hip_tiff.h)
TIFF_SEGMENT_DTYPE = np.dtype([('src_offset', '<i8'), ('src_bytes', '<i8'), ('dst_offset', '<i8'), ('rows', '<i4'), ('reserved', '<i4')])


class TiffError(ValueError):
    """The file is truncated or contradicts itself, or a strip does not decode."""


class TiffUnsupported(ValueError):
    """A valid TIFF that uses something this reader does not decode; the message names the tag and its value."""


class TiffInfo:
    """What tiff_info returns. Segment k is one strip: bytes [src_offset[k], src_offset[k] + src_bytes[k]) of the file hold
    rows[k] rows of frame[k], starting at row0[k]."""

    def __init__(self, path, shape, byteorder, compression, predictor, bigtiff, imagej, src_offset, src_bytes, frame, row0, rows):
        self.path, self.shape, self.byteorder, self.compression, self.predictor = path, tuple(shape), byteorder, compression, predictor
        self.bigtiff, self.imagej = bigtiff, imagej
        self.src_offset, self.src_bytes = np.asarray(src_offset, np.int64), np.asarray(src_bytes, np.int64)
        self.frame, self.row0, self.rows = (np.asarray(a, np.int32) for a in (frame, row0, rows))

    @property
    def n_segments(self):
        return len(self.src_offset)

    def __repr__(self):
        return (f'TiffInfo(shape={self.shape}, byteorder={self.byteorder!r}, compression={self.compression}, '
                f'predictor={self.predictor}, bigtiff={self.bigtiff}, imagej={self.imagej}, segments={self.n_segments})')


def _need(buf, offset, nbytes, what):
    if offset < 0 or nbytes < 0 or offset + nbytes > len(buf):
        raise TiffError(f'{what} at offset {offset} ({nbytes} bytes) lies outside the file of {len(buf)} bytes')


def _read_ifd(buf, offset, bo, big):
    """-> ({tag: (type, count, where the value bytes are)}, offset of the next IFD)."""
    cnt_fmt, cnt_size, ent_size, off_fmt, off_size = ('Q', 8, 20, 'Q', 8) if big else ('H', 2, 12, 'I', 4)
    _need(buf, offset, cnt_size, 'the IFD')
    n = struct.unpack_from(bo + cnt_fmt, buf, offset)[0]
    if n > MAX_IFD_ENTRIES:
        raise TiffError(f'the IFD at offset {offset} claims {n} entries')
    _need(buf, offset, cnt_size + n * ent_size + off_size, f'the IFD of {n} entries')
    tags = {}
    for i in range(n):
        e = offset + cnt_size + i * ent_size
        tag, ftype = struct.unpack_from(bo + 'HH', buf, e)
        count = struct.unpack_from(bo + off_fmt, buf, e + 4)[0]
        if ftype not in FIELD_TYPES:
            continue                                                      # (an unknown field type: the tag is skipped, as TIFF 6.0 asks)
        nbytes = FIELD_TYPES[ftype][1] * count
        where = e + 4 + off_size
        if nbytes > off_size:
            where = struct.unpack_from(bo + off_fmt, buf, where)[0]
            _need(buf, where, nbytes, f'the value of tag {tag} ({TAG_NAMES.get(tag, "?")})')
        tags[tag] = (ftype, count, where)
    nxt = struct.unpack_from(bo + off_fmt, buf, offset + cnt_size + n * ent_size)[0]
    return tags, nxt


def _ints(buf, bo, tags, tag, default=None):
    """The integer values of a tag as an int64 array, or `default` where the tag is absent."""
    if tag not in tags:
        return default
    ftype, count, where = tags[tag]
    if ftype not in _INTEGER_TYPES:
        raise TiffUnsupported(f'{TAG_NAMES.get(tag, tag)} has field type {ftype}, not an integer type')
    letter, size = FIELD_TYPES[ftype]
    return np.frombuffer(buf, dtype=np.dtype(bo + {'B': 'u1', 'b': 'i1', 'H': 'u2', 'h': 'i2', 'I': 'u4', 'i': 'i4', 'Q': 'u8',
                                                   'q': 'i8'}[letter]), count=count, offset=where).astype(np.int64)


def _one(buf, bo, tags, tag, default):
    v = _ints(buf, bo, tags, tag)
    if v is None:
        return default
    if len(v) != 1:
        raise TiffUnsupported(f'{TAG_NAMES.get(tag, tag)} has {len(v)} values {v[:4].tolist()}')
    return int(v[0])


def _page(buf, bo, tags, ifd_offset):
    """One IFD as (H, W, compression, predictor, strip offsets, strip byte counts, rows per strip, description), after
    every refusal this reader makes."""
    for tag in (TILE_WIDTH, TILE_LENGTH, TILE_OFFSETS, TILE_BYTE_COUNTS):
        if tag in tags:
            raise TiffUnsupported(f'{TAG_NAMES[tag]} is present in the IFD at offset {ifd_offset}: tiled files are not read, strips only')
    spp = _one(buf, bo, tags, SAMPLES_PER_PIXEL, 1)
    if spp != 1:
        raise TiffUnsupported(f'SamplesPerPixel {spp}: one grayscale plane per page is read, not RGB or multi-channel pixels')
    bits = _one(buf, bo, tags, BITS_PER_SAMPLE, 1)
    if bits != 16:
        raise TiffUnsupported(f'BitsPerSample {bits}: 16-bit samples only')
    fmt = _one(buf, bo, tags, SAMPLE_FORMAT, 1)
    if fmt != 1:
        raise TiffUnsupported(f'SampleFormat {fmt}: unsigned integers (1) only')
    photo = _one(buf, bo, tags, PHOTOMETRIC, 1)
    if photo not in (0, 1):
        raise TiffUnsupported(f'PhotometricInterpretation {photo}: grayscale (0 or 1) only')
    comp = _one(buf, bo, tags, COMPRESSION, 1)
    if comp not in SUPPORTED_COMPRESSION:
        raise TiffUnsupported(f'Compression {comp}: supported are 1 (none), 5 (LZW), 8 / 32946 (Deflate), 32773 (PackBits)')
    pred = _one(buf, bo, tags, PREDICTOR, 1)
    if pred not in (1, 2):
        raise TiffUnsupported(f'Predictor {pred}: none (1) or horizontal differencing (2) only')
    W, H = _one(buf, bo, tags, IMAGE_WIDTH, None), _one(buf, bo, tags, IMAGE_LENGTH, None)
    if W is None or H is None or W < 1 or H < 1:
        raise TiffError(f'the IFD at offset {ifd_offset} lacks ImageWidth / ImageLength (got {W}, {H})')
    offs, cnts = _ints(buf, bo, tags, STRIP_OFFSETS), _ints(buf, bo, tags, STRIP_BYTE_COUNTS)
    if offs is None:
        raise TiffError(f'the IFD at offset {ifd_offset} has no StripOffsets')
    rps = _one(buf, bo, tags, ROWS_PER_STRIP, H)
    rps = H if rps < 1 or rps > H else rps
    n = -(-H // rps)
    if cnts is None and comp == COMPRESSION_NONE and len(offs) == 1:
        cnts = np.array([H * W * 2], np.int64)                            # (old writers leave the count out of a one-strip page)
    if cnts is None or len(offs) != n or len(cnts) != n:
        raise TiffError(f'the IFD at offset {ifd_offset} needs {n} strips of {rps} rows for {H} rows but lists '
                        f'{len(offs)} offsets and {0 if cnts is None else len(cnts)} byte counts')
    desc = b''
    if IMAGE_DESCRIPTION in tags and tags[IMAGE_DESCRIPTION][0] == 2:
        _, count, where = tags[IMAGE_DESCRIPTION]
        desc = bytes(buf[where:where + count])
    return H, W, comp, pred, offs, cnts, rps, desc


def tiff_info(path):
    """Parse the container: every kept page's geometry and the table of its strips. Reads headers and tags only; every
    (offset, bytes) of the table has been checked against the file size."""
    try:
        buf = np.memmap(path, dtype=np.uint8, mode='r')
    except ValueError as e:                                               # (numpy refuses to map an empty file)
        raise TiffError(f'the header at offset 0 lies outside the file: {e}') from e
    try:
        return _tiff_info(buf, path)
    finally:
        del buf


def _tiff_info(buf, path):
    size = len(buf)
    _need(buf, 0, 8, 'the header')
    mark = bytes(buf[:2])
    if mark not in (b'II', b'MM'):
        raise TiffError(f'not a TIFF file: the byte-order mark at offset 0 is {mark!r}')
    bo = '<' if mark == b'II' else '>'
    magic = struct.unpack_from(bo + 'H', buf, 2)[0]
    if magic == 42:
        big, first = False, struct.unpack_from(bo + 'I', buf, 4)[0]
    elif magic == 43:
        _need(buf, 0, 16, 'the BigTIFF header')
        osize, zero, first = struct.unpack_from(bo + 'HHQ', buf, 4)
        if osize != 8 or zero != 0:
            raise TiffError(f'BigTIFF header at offset 4: offset size {osize}, constant {zero} (expected 8, 0)')
        big = True
    else:
        raise TiffError(f'not a TIFF file: magic number {magic} at offset 2 (42 = TIFF, 43 = BigTIFF)')
    pages, seen, offset = [], set(), first
    while offset:
        if offset in seen:
            raise TiffError(f'the IFD chain loops back to offset {offset}')
        seen.add(offset)
        tags, nxt = _read_ifd(buf, offset, bo, big)
        if not _one(buf, bo, tags, NEW_SUBFILE_TYPE, 0) & 1:              # bit 0: a reduced-resolution copy of another page
            pages.append(_page(buf, bo, tags, offset) + (offset,))
        offset = nxt
    if not pages:
        raise TiffError('the file holds no full-resolution page')
    H, W, comp, pred = pages[0][:4]
    for k, p in enumerate(pages):
        if p[:4] != (H, W, comp, pred):
            raise TiffUnsupported(f'page {k} (IFD at offset {p[-1]}) is {p[1]} x {p[0]}, Compression {p[2]}, Predictor {p[3]}; '
                                  f'page 0 is {W} x {H}, Compression {comp}, Predictor {pred}: all pages must agree')
    imagej, T = False, len(pages)
    src_offset, src_bytes, frame, row0, rows = [], [], [], [], []
    desc = pages[0][7]
    n_images = 0
    if desc.startswith(b'ImageJ='):
        imagej = True
        for line in desc.split(b'\n'):
            if line.startswith(b'images='):
                try:
                    n_images = int(line[7:].strip(b'\0 \r'))
                except ValueError:
                    raise TiffError(f'ImageDescription of the IFD at offset {pages[0][-1]}: {line!r} is no frame count')
    if imagej and n_images > len(pages) and comp == COMPRESSION_NONE:
        # ImageJ's layout for stacks beyond 4 GB: ONE IFD, the frames back to back behind its first strip
        if len(pages) != 1:
            raise TiffUnsupported(f'ImageDescription images={n_images} with {len(pages)} IFDs: the single-IFD hyperstack layout has one')
        offs, cnts = pages[0][4], pages[0][5]
        if (offs[1:] != offs[:-1] + cnts[:-1]).any():
            raise TiffUnsupported('StripOffsets of an ImageJ hyperstack are not contiguous')
        T = n_images
        src_offset = int(offs[0]) + np.arange(T, dtype=np.int64) * (H * W * 2)
        src_bytes = np.full(T, H * W * 2, np.int64)
        frame, row0, rows = np.arange(T), np.zeros(T), np.full(T, H)
    else:
        for k, p in enumerate(pages):
            offs, cnts, rps = p[4], p[5], p[6]
            r0 = np.arange(len(offs), dtype=np.int64) * rps
            src_offset.append(offs), src_bytes.append(cnts), frame.append(np.full(len(offs), k)), row0.append(r0)
            rows.append(np.minimum(rps, H - r0))
        src_offset, src_bytes, frame, row0, rows = (np.concatenate(a) for a in (src_offset, src_bytes, frame, row0, rows))
    # every segment against the file, before anything is read
    bad = np.flatnonzero((src_offset < 0) | (src_bytes < 0) | (src_offset + src_bytes > size))
    if len(bad):
        k = int(bad[0])
        raise TiffError(f'the strip of frame {int(frame[k])}, row {int(row0[k])} at offset {int(src_offset[k])} '
                        f'({int(src_bytes[k])} bytes) lies outside the file of {size} bytes')
    if comp == COMPRESSION_NONE:
        bad = np.flatnonzero(src_bytes != np.asarray(rows, np.int64) * W * 2)
        if len(bad):
            k = int(bad[0])
            raise TiffError(f'the uncompressed strip of frame {int(frame[k])}, row {int(row0[k])} at offset {int(src_offset[k])} '
                            f'has {int(src_bytes[k])} bytes for {int(rows[k])} rows of {W} samples')
    if comp == COMPRESSION_LZW:
        # old-style LZW (codes least significant bit first): a first byte of 0 with the low bit of the second set, libtiff's test
        for k in np.flatnonzero(src_bytes >= 2):
            o = int(src_offset[k])
            if buf[o] == 0 and buf[o + 1] & 1:
                raise TiffUnsupported(f'Compression 5 in its old LSB-first form (strip of frame {int(frame[k])} at offset {o} '
                                      f'starts 0x00 0x{int(buf[o + 1]):02x}): only MSB-first LZW is decoded')
    return TiffInfo(path, (T, H, W), bo, comp, pred, big, imagej, src_offset, src_bytes, frame, row0, rows)


def _frame_list(frames, T):
    if frames is None:
        return 0, T
    if isinstance(frames, slice):
        frames = range(*frames.indices(T))
    if not isinstance(frames, range) or (len(frames) > 1 and frames.step != 1):
        raise TypeError('frames is a range or slice of consecutive pages')
    if len(frames) == 0 or frames[0] < 0 or frames[-1] >= T:
        raise IndexError(f'frames {frames} outside the {T} pages of the file')
    return frames[0], frames[-1] + 1


def inflate_on_device(n_segments):
    """Whether a pack of n_segments Deflate strips is inflated on the device (csrc/tiff_inflate.hip) or by zlib on the host.
    One wave inflates one strip, so a launch of very few large strips takes as long as one wave needs for its whole
    strip, and one host core is faster there. Where the routes cross is a measurement, profiles/tiff_inflate_timing.json
    ('small_packs': both routes on packs of 1 to 256 strips): the device's time is that of one wave's strip
    whatever the count, the host's grows with it, and from 64 strips on the device wins both for strips of whole 512 x 512
    pages (from 32 on) and for strips of 32 rows (the host still wins at 32)."""
    return n_segments >= INFLATE_ON_DEVICE_FROM


class SegmentPacker:
    """The strips of runs of frames, packed for the device. pack(a, b) -> (bytes as a numpy uint8 view of a pinned torch
    buffer, that buffer, descriptor records for hotpath.tiff_decode_u16 with dst offsets relative to frame a, the
    number of bytes packed). Strips that follow one another in the file are copied as one run, compressed as they are:
    device_compression, what the records are to be decoded with, is the file's own.

    inflate: where Deflate strips are inflated. 'device': they travel compressed like every other strip and
    device_compression is 8 / 32946. 'host': zlib.decompress here, strip by strip; the inflated bytes travel and
    device_compression is 1. None: inflate_on_device(number of strips) decides for every pack call, so device_compression
    is to be read after pack."""

    def __init__(self, info, inflate=None):
        if inflate not in (None, 'device', 'host'):
            raise ValueError(f"inflate is 'device', 'host' or None, not {inflate!r}")
        self.info, self.inflate = info, inflate
        self.buf = np.memmap(info.path, dtype=np.uint8, mode='r')
        self.first = np.searchsorted(info.frame, np.arange(info.shape[0] + 1))       # (the table is in frame order)
        # little-endian, uncompressed, no predictor: where the packed strips also come out in frame order, one plain copy is
        # the whole job (the callers check the order)
        self.plain = info.compression == COMPRESSION_NONE and info.predictor == 1 and info.byteorder == '<'
        self.device_compression = COMPRESSION_NONE if info.compression in DEFLATE and inflate == 'host' else info.compression

    def segments(self, a, b):
        return int(self.first[a]), int(self.first[b])

    def pack(self, a, b, pinned=True):
        import torch
        i = self.info
        _, H, W = i.shape
        s0, s1 = self.segments(a, b)
        off, nbytes = i.src_offset[s0:s1], i.src_bytes[s0:s1]
        segs = np.zeros(s1 - s0, TIFF_SEGMENT_DTYPE)
        segs['dst_offset'] = ((i.frame[s0:s1].astype(np.int64) - a) * H + i.row0[s0:s1]) * W
        segs['rows'] = i.rows[s0:s1]
        on_host = False
        if i.compression in DEFLATE:
            on_host = self.inflate == 'host' or (self.inflate is None and not inflate_on_device(s1 - s0))
            self.device_compression = COMPRESSION_NONE if on_host else i.compression
        if on_host:
            parts = []
            for k in range(s0, s1):
                o, n = int(i.src_offset[k]), int(i.src_bytes[k])
                try:
                    parts.append(zlib.decompress(bytes(self.buf[o:o + n])))
                except zlib.error as e:
                    raise TiffError(f'the Deflate strip of frame {int(i.frame[k])}, row {int(i.row0[k])} at offset {o} does not '
                                    f'inflate: {e}') from e
            sizes = np.array([len(p) for p in parts], np.int64)
            starts = np.concatenate([[0], np.cumsum(sizes)])
            total = int(starts[-1])
            host = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=pinned)
            view = host.numpy()
            view[:total] = np.frombuffer(b''.join(parts), np.uint8)
            segs['src_offset'], segs['src_bytes'] = starts[:-1], sizes
        else:
            starts = np.concatenate([[0], np.cumsum(nbytes)])
            total = int(starts[-1])
            host = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=pinned)
            view = host.numpy()
            breaks = np.flatnonzero(off[1:] != off[:-1] + nbytes[:-1]) + 1          # runs of strips adjacent in the file
            for r0, r1 in zip(np.concatenate([[0], breaks]), np.concatenate([breaks, [len(off)]])):
                if r1 > r0:
                    o, n = int(off[r0]), int(starts[r1] - starts[r0])
                    view[int(starts[r0]):int(starts[r0]) + n] = self.buf[o:o + n]
            segs['src_offset'], segs['src_bytes'] = starts[:-1], nbytes
        return view[:total], host, segs, total


def read_tiff(path, frames=None, device='cuda:0'):
    """The pages of a TIFF timelapse as one stack: int16-viewed uint16 [T,H,W] on `device` (what preprocess and
    estimate_stnd_scaler take as they take an array), or with device='cpu' a numpy uint16 array by the same route plus one
    copy back. frames: a range or slice of consecutive pages. The strips' bytes go to the device as they are in the file,
    at most CHUNK_FRAMES frames at a time through a pinned buffer, and are expanded there; the statuses of all segments
    are read once at the end, and a strip that does not decode -- a Deflate strip that does not inflate or fails its
    Adler-32 included -- raises TiffError naming its frame and row."""
    import torch
    from . import hotpath as hp
    info = tiff_info(path)
    T, H, W = info.shape
    a, b = _frame_list(frames, T)
    to_host = str(device) == 'cpu'
    dev = torch.device('cuda:0' if to_host else device)
    hp._require_gpu()
    packer = SegmentPacker(info)
    out = torch.empty((b - a, H, W), dtype=torch.int16, device=dev)
    s0, s1 = packer.segments(a, b)
    status = torch.zeros(max(s1 - s0, 1), dtype=torch.int32, device=dev)
    keep = []
    with torch.cuda.device(dev):
        for c0 in range(a, b, CHUNK_FRAMES):
            c1 = min(c0 + CHUNK_FRAMES, b)
            view, host, segs, total = packer.pack(c0, c1)
            chunk = out[c0 - a:c1 - a]
            if packer.plain and total == chunk.numel() * 2 and np.array_equal(segs['src_offset'], segs['dst_offset'] * 2):
                chunk.view(torch.uint8).view(-1).copy_(host[:total], non_blocking=True)
            else:
                d_src = host.to(dev, non_blocking=True)
                k0 = packer.segments(a, c0)[1] - s0
                hp.tiff_decode_launch(d_src, segs, W, packer.device_compression, info.predictor, info.byteorder == '>', chunk,
                                      status[k0:k0 + len(segs)])
                keep.append(d_src)
            keep.append(host)
        hp.tiff_raise_on_status(status[:s1 - s0], info.frame[s0:s1], info.row0[s0:s1], path)       # (waits for the stream)
    return out.cpu().numpy().view(np.uint16) if to_host else out


def read_stack(path, device='cuda:0', to_host=True):
    """What the interface's file readers call for a .tif / .tiff name: read_tiff, and where the file uses something this
    reader refuses (TiffUnsupported), tifffile.imread if that package is importable; otherwise the refusal, whose message
    names what the file uses."""
    try:
        return read_tiff(path, device='cpu' if to_host else device)
    except TiffUnsupported:
        try:
            from tifffile import imread
        except ImportError:
            imread = None
        if imread is None:
            raise
        return imread(path)


def is_tiff_name(name):
    return isinstance(name, str) and name.lower().endswith(('.tif', '.tiff'))


# ====================================================================================================== TIFF output
def deflate_on_device(n_strips):
    """Whether write_tiff deflates a chunk of n_strips strips on the device (csrc/tiff_deflate.hip) or with zlib in a
    pool of host threads. One wave deflates one strip, so a launch of few strips takes as long as one wave needs for its
    strip whatever the count, while the host's time grows with the count; where the routes cross is a measurement
    (profiles/tiff_deflate_timing.py, 'small_packs'). That measurement has not been run yet: the threshold is the
    inflater's crossover, taken over as a placeholder (DESIGN.md 6.8h "TIFF output", "Time and routing")."""
    return n_strips >= DEFLATE_ON_DEVICE_FROM


def strip_layout(H, W, rows_per_strip=None):
    """-> (rows per strip, first row of every strip, rows of every strip). None: as many rows as fit 32 KiB, the Deflate
    window, at least one and at most H."""
    if rows_per_strip is None:
        rows_per_strip = min(H, max(1, 32768 // (2 * W)))
    rps = int(rows_per_strip)
    if not 1 <= rps <= H:
        raise ValueError(f'rows_per_strip {rows_per_strip} is not in 1..{H}')
    row0 = np.arange(0, H, rps, dtype=np.int64)
    return rps, row0, np.minimum(rps, H - row0)


def stored_bound(raw_bytes):
    """The all-stored zlib stream of raw_bytes bytes: what axt_tiff_deflate_bound returns."""
    return raw_bytes + 5 * max(1, -(-raw_bytes // 65535)) + 6


def _ifd_size(n_strips, big, desc_len):
    """Bytes of one IFD of build_ifd with its out-of-line values, at most (twelve entries)."""
    tables = 2 * n_strips * (8 if big else 4) if n_strips > 1 else 0
    return (8 + 12 * 20 + 8 if big else 2 + 12 * 12 + 4) + tables + desc_len + (desc_len & 1)


def file_bound(T, H, W, rows_per_strip, big, desc_len=0):
    """The size of the file write_tiff writes if every strip came out stored: what decides between TIFF and BigTIFF."""
    rps, row0, rows = strip_layout(H, W, rows_per_strip)
    page = int(sum(stored_bound(2 * int(r) * W) for r in rows)) + 1 + _ifd_size(len(rows), big, 0)
    return (16 if big else 8) + T * page + desc_len + (desc_len & 1)


def choose_bigtiff(T, H, W, rows_per_strip=None, bigtiff=None, desc_len=0):
    """bigtiff None: classic TIFF where the all-stored bound of the whole file stays below 4 GiB, else BigTIFF. False on
    a file that may not fit raises."""
    fits = file_bound(T, H, W, rows_per_strip, False, desc_len) < 1 << 32
    if bigtiff is None:
        return not fits
    if not bigtiff and not fits:
        raise ValueError(f'{T} pages of {H} x {W} may take {file_bound(T, H, W, rows_per_strip, False, desc_len)} bytes, more than '
                         f'the 4 GiB of classic TIFF offsets: bigtiff=False cannot be kept')
    return bool(bigtiff)


def tiff_header(big, first_ifd=0):
    return struct.pack('<2sHHHQ', b'II', 43, 8, 0, first_ifd) if big else struct.pack('<2sHI', b'II', 42, first_ifd)


def build_ifd(at, H, W, rows_per_strip, predictor, big, strip_offsets, strip_counts, description=None, next_ifd=0):
    """One page's IFD as it stands at the even file offset `at`, its out-of-line values (the strip tables, the description)
    behind it, each at an even offset: little-endian, Compression 8, PhotometricInterpretation 1, SampleFormat 1,
    Predictor only when it is 2, tags in ascending order. -> (bytes, where in them the offset of the next IFD stands)."""
    assert at % 2 == 0 and len(strip_offsets) == len(strip_counts) == -(-H // rows_per_strip)
    otype, ofmt, inline = (16, 'Q', 8) if big else (4, 'I', 4)
    n = len(strip_offsets)
    entries = [(IMAGE_WIDTH, 4, [W]), (IMAGE_LENGTH, 4, [H]), (BITS_PER_SAMPLE, 3, [16]), (COMPRESSION, 3, [COMPRESSION_ADOBE_DEFLATE]),
               (PHOTOMETRIC, 3, [1])]
    if description is not None:
        entries.append((IMAGE_DESCRIPTION, 2, bytes(description) + b'\0'))
    entries += [(STRIP_OFFSETS, otype, list(strip_offsets)), (SAMPLES_PER_PIXEL, 3, [1]), (ROWS_PER_STRIP, 4, [rows_per_strip]),
                (STRIP_BYTE_COUNTS, otype, list(strip_counts))]
    if predictor == 2:
        entries.append((PREDICTOR, 3, [2]))
    entries.append((SAMPLE_FORMAT, 3, [1]))
    head = 8 + 20 * len(entries) + 8 if big else 2 + 12 * len(entries) + 4
    body, extra = struct.pack('<Q' if big else '<H', len(entries)), b''
    for tag, ftype, values in entries:
        if ftype == 2:
            data, count = values, len(values)
        else:
            data, count = struct.pack(f'<{len(values)}{FIELD_TYPES[ftype][0]}', *values), len(values)
        if len(data) > inline:
            where = at + head + len(extra)
            extra += data + b'\0' * (len(data) & 1)
            data = struct.pack('<' + ofmt, where)
        body += struct.pack('<HH' + ofmt, tag, ftype, count) + data.ljust(inline, b'\0')
    next_at = len(body)
    return body + struct.pack('<' + ofmt, next_ifd) + extra, next_at


class TiffWriter:
    """The container of write_tiff: pages of Deflate strips in a file, one IFD behind each page's strips, which follow one
    another without a gap so that a reader copies them as one run. Host only; the strips come compressed."""

    def __init__(self, path, H, W, rows_per_strip=None, predictor=1, big=False, description=None):
        if predictor not in (1, 2):
            raise ValueError(f'predictor {predictor} is not 1 (none) or 2 (horizontal differencing)')
        self.H, self.W, self.predictor, self.big, self.description = H, W, predictor, bool(big), description
        self.rps, self.row0, self.rows = strip_layout(H, W, rows_per_strip)
        self.f = open(path, 'wb')
        self.f.write(tiff_header(self.big))
        self.pos = 16 if self.big else 8
        self.link = 8 if self.big else 4                                  # where the offset of the next IFD is to be written
        self.pages, self.strip_bytes, self.ifd_bytes = 0, 0, 0

    def add_page(self, strips):
        if len(strips) != len(self.rows):
            raise ValueError(f'a page has {len(self.rows)} strips, not {len(strips)}')
        offsets, counts = [], []
        for s in strips:
            offsets.append(self.pos), counts.append(len(s))
            self.f.write(s)
            self.pos += len(s)
        self.strip_bytes += sum(counts)
        if self.pos & 1:
            self.f.write(b'\0')
            self.pos += 1
            self.ifd_bytes += 1
        if not self.big and self.pos + _ifd_size(len(strips), False, len(self.description or b'') + 1) >= 1 << 32:
            raise TiffError(f'page {self.pages} ends beyond the 4 GiB of classic TIFF offsets')
        ifd, next_at = build_ifd(self.pos, self.H, self.W, self.rps, self.predictor, self.big, offsets, counts,
                                 self.description if self.pages == 0 else None)
        self.f.write(ifd)
        self.f.seek(self.link)
        self.f.write(struct.pack('<Q' if self.big else '<I', self.pos))
        self.f.seek(0, 2)
        self.link = self.pos + next_at
        self.pos += len(ifd)
        self.ifd_bytes += len(ifd)
        self.pages += 1

    def close(self):
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def apply_predictor(a, predictor):
    """uint16 [..., W] as stored: with predictor 2 every sample minus its left neighbour, modulo 2^16."""
    a = np.asarray(a, np.uint16)
    if predictor == 2:
        d = a.copy()
        d[..., 1:] -= a[..., :-1]
        a = d
    return a


def _deflate_on_host(raw, row0, rows, predictor, level):
    """raw: uint16 [frames, H, W] on the host -> every strip's zlib stream, frame by frame, in a pool of threads."""
    from concurrent.futures import ThreadPoolExecutor
    from .render import _POOL_THREADS
    stored = np.ascontiguousarray(apply_predictor(raw, predictor), '<u2')
    jobs = [(t, int(r0), int(r)) for t in range(len(stored)) for r0, r in zip(row0, rows)]
    with ThreadPoolExecutor(max_workers=_POOL_THREADS) as pool:
        return list(pool.map(lambda j: zlib.compress(stored[j[0], j[1]:j[1] + j[2]].data, level), jobs))


def write_tiff(path, stack, rows_per_strip=None, predictor=1, bigtiff=None, deflate=None, description=None, level=6):
    """Write a timelapse as a Deflate TIFF (Compression 8), one page per frame, the strips deflated on the GPU
    (csrc/tiff_deflate.hip): what tifffile's imsave(..., photometric='minisblack', compression='deflate') is used for.

    stack: uint16 -- or the int16-viewed raw counts read_tiff returns -- [T,H,W] or [H,W], a device tensor, a host tensor
    or a numpy array (uploaded one chunk of CHUNK_FRAMES frames at a time). rows_per_strip None: as many rows as fit the
    32 KiB Deflate window (16 strips for a 512 x 512 page); any value 1..H. predictor 2: horizontal differencing. bigtiff
    None: classic TIFF where the file cannot pass 4 GiB, else BigTIFF. deflate 'device' / 'host' / None: where the strips
    are deflated; None asks deflate_on_device for every chunk; the host route is zlib at `level` in a pool of threads,
    behind a copy of the raw chunk to the host. description: bytes for page 0's ImageDescription.
    Returns the TiffWriter (closed): pages, strip_bytes, ifd_bytes."""
    import torch
    from . import hotpath as hp
    if deflate not in (None, 'device', 'host'):
        raise ValueError(f"deflate is 'device', 'host' or None, not {deflate!r}")
    on_host_array = not isinstance(stack, torch.Tensor)
    if on_host_array:
        stack = np.asarray(stack)
        if stack.dtype not in (np.uint16, np.int16):
            raise TypeError(f'stack is {stack.dtype}, not uint16 (or int16-viewed raw counts)')
        stack = torch.from_numpy(np.ascontiguousarray(stack).view(np.int16))
    elif stack.dtype not in (torch.int16, getattr(torch, 'uint16', torch.int16)):
        raise TypeError(f'stack is {stack.dtype}, not uint16 (or int16-viewed raw counts)')
    elif stack.dtype != torch.int16:
        stack = stack.view(torch.int16)
    if stack.dim() == 2:
        stack = stack[None]
    if stack.dim() != 3 or 0 in stack.shape:
        raise ValueError(f'stack has shape {tuple(stack.shape)}, not [T,H,W] or [H,W]')
    T, H, W = stack.shape
    rps, row0, rows = strip_layout(H, W, rows_per_strip)
    desc = None if description is None else (description.encode() if isinstance(description, str) else bytes(description))
    big = choose_bigtiff(T, H, W, rps, bigtiff, 0 if desc is None else len(desc) + 1)      # (raises before anything is written)
    hp._require_gpu()
    dev = stack.device if stack.is_cuda else torch.device('cuda:0')
    per_page = len(rows)
    with TiffWriter(path, H, W, rps, predictor, big, desc) as w, torch.cuda.device(dev):
        for c0 in range(0, T, CHUNK_FRAMES):
            c1 = min(c0 + CHUNK_FRAMES, T)
            n = (c1 - c0) * per_page
            on_device = deflate == 'device' or (deflate is None and deflate_on_device(n))
            if on_device:
                chunk = stack[c0:c1].contiguous().to(dev, non_blocking=True)
                segs = np.zeros(n, TIFF_SEGMENT_DTYPE)
                frame = np.repeat(np.arange(c0, c1), per_page)
                segs['dst_offset'] = ((frame - c0) * H + np.tile(row0, c1 - c0)) * W
                segs['rows'] = np.tile(rows, c1 - c0)
                data, offsets = hp.tiff_deflate_strips(chunk, segs, W, predictor, frame, np.tile(row0, c1 - c0))
                strips = [data[int(offsets[k]):int(offsets[k + 1])] for k in range(n)]
            else:
                raw = stack[c0:c1].cpu().numpy().view(np.uint16)
                strips = _deflate_on_host(raw, row0, rows, predictor, level)
            for t in range(c1 - c0):
                w.add_page(strips[t * per_page:(t + 1) * per_page])
    return w
