"""Input container of the hot path: the timelapse as ONE dense f32 tensor in HBM.

Mirrors the attributes of the reference's Timelapse (axtrack/Timelapse.py) that the inference
path reads -- name, sizet/sizey/sizex, tilesize, mask, len() -- but keeps only what the
detector consumes: channel 0 of `X` (Timelapse.py:426-433; the two motion channels are all
zeros for USE_MOTION_DATA='exclude', :366-367), context-padded: T_all = sizet + 2*context.
"""
import os

import numpy as np
import torch


class Timelapse:
    def __init__(self, frames, name='timelapse', mask=None, temporal_context=2, tilesize=512,
                 device='cuda:0', pixelsize=None, dt=None, incubation_time=None, labels=None, stnd_scaler=None):
        """frames: preprocessed f32 [T_all,H,W] (numpy or torch); mask: bool [H,W] or None (all ones).
        labels: None, or one entry per DETECTION frame, (x, y) or (x, y, ids) integer arrays as load_labels_csv returns
        them and AxonDetections.set_groundtruth / fine_tune_head take them. stnd_scaler: the scaler the frames were
        standardised with, (name, (var_scalar, mean_scalar)) or (name, None) for frame-wise scales (Timelapse.py:300-302)."""
        if temporal_context != 2:
            raise ValueError('the deployed detector has 5 input channels: temporal_context must be 2')
        f = torch.as_tensor(frames)
        if f.dim() != 3:
            raise ValueError(f'frames must be [T_all,H,W], got {tuple(f.shape)}')
        if f.shape[0] < 2 * temporal_context + 1:
            raise ValueError('need at least 5 frames (2 context frames either side of one detection frame)')
        self.frames = f.to(device=device, dtype=torch.float32).contiguous()
        self.name = name
        self.temporal_context = temporal_context
        self.tilesize = tilesize
        self.sizet = self.frames.shape[0] - 2 * temporal_context
        self.sizey, self.sizex = int(self.frames.shape[1]), int(self.frames.shape[2])
        self.ytiles, self.xtiles = -(-self.sizey // tilesize), -(-self.sizex // tilesize)
        # mask: one for the whole timelapse, or one per input frame (Timelapse.py:210-217 stacks a 2-D mask to [T,H,W];
        # AxonDetections._get_maskweights(t) then reads mask[t], AxonDetections.py:587-598). mask2d is the static
        # mask (None = all ones); mask3d is set only when the mask really changes over time.
        self.mask2d, self.mask3d = None, None
        if mask is not None:
            mask = np.asarray(mask).astype(bool)
            if mask.ndim == 3:
                if mask.shape != (self.frames.shape[0], self.sizey, self.sizex):
                    raise ValueError(f'a time-varying mask must be [T_all,H,W] = {tuple(self.frames.shape)}, got {mask.shape}')
                if (mask == mask[0]).all():
                    mask = mask[0]
            if mask.ndim == 2:
                if mask.shape != (self.sizey, self.sizex):
                    raise ValueError('mask must be [H,W] or [T_all,H,W]')
                self.mask2d = None if mask.all() else mask
            elif mask.ndim == 3:
                self.mask3d = mask
            else:
                raise ValueError('mask must be [H,W] or [T_all,H,W]')
        self.pixelsize, self.dt, self.incubation_time = pixelsize, dt, incubation_time
        self.timepoints = np.arange(temporal_context, temporal_context + self.sizet)
        if labels is not None:
            labels = [tuple(np.asarray(a, np.int64) for a in l) for l in labels]
            if len(labels) != self.sizet:
                raise ValueError(f'{len(labels)} label frames for {self.sizet} detection frames')
        self.labels, self.stnd_scaler = labels, stnd_scaler

    @property
    def labelled(self):
        return self.labels is not None

    def __len__(self):
        return self.sizet

    @property
    def masked(self):
        return self.mask2d is not None or self.mask3d is not None

    def mask_groups(self, quirk=True):
        """Time-varying masks: (list of distinct [H,W] masks, index i32 [sizet]) -- which mask the reference searches the
        paths on that END in detection frame t. With quirk=True (default) that is mask[t], the mask of INPUT frame t:
        _get_maskweights(t) indexes the context-padded frame list with the detection-frame index (AxonDetections.py:557,
        598; Timelapse.py:408), two frames before the one detection frame t shows. quirk=False takes mask[t + context]."""
        m = self.mask3d
        keys, masks, index = {}, [], np.zeros(self.sizet, np.int32)
        for t in range(self.sizet):
            f = m[t if quirk else t + self.temporal_context]
            k = f.tobytes()
            if k not in keys:
                keys[k] = len(masks)
                masks.append(f)
            index[t] = keys[k]
        return masks, index

    def to_cache(self, directory):
        """'{name}_dataset_cached.pkl' (Timelapse._caching, Timelapse.py:435-449): the reference pickles its whole
        __dict__ (sparse tensors of all three channels); this writes the same file name with what the hot path keeps --
        the preprocessed frames, the mask, the metadata and, of a labelled dataset, the labels and the scaler."""
        import os
        import pickle
        os.makedirs(directory, exist_ok=True)
        self.make_resident()
        d = dict(_axtrack_amd_cache=1, name=self.name, frames=self.frames.cpu().numpy(),
                 mask=self.mask3d if self.mask3d is not None else self.mask2d, temporal_context=self.temporal_context,
                 tilesize=self.tilesize, pixelsize=self.pixelsize, dt=self.dt, incubation_time=self.incubation_time,
                 labels=self.labels, stnd_scaler=self.stnd_scaler)
        with open(f'{directory}/{self.name}_dataset_cached.pkl', 'wb') as file:
            pickle.dump(d, file, protocol=4)

    @classmethod
    def from_cache(cls, directory, name, device='cuda:0'):
        """Read '{name}_dataset_cached.pkl': this package's own format, or a file the reference wrote (its __dict__: `X` a
        sparse tensor [T_all, 3, H, W] whose channel 0 is the preprocessed image, `mask` a list of scipy coo matrices)."""
        import os
        import pickle
        fname = f'{directory}/{name}_dataset_cached.pkl'
        assert os.path.exists(fname), f'\n\nNo cached dataset found: {fname}'
        with open(fname, 'rb') as file:
            d = pickle.load(file)
        if d.get('_axtrack_amd_cache'):
            return cls(d['frames'], name=d['name'], mask=d['mask'], temporal_context=d['temporal_context'],
                       tilesize=d['tilesize'], device=device, pixelsize=d['pixelsize'], dt=d['dt'],
                       incubation_time=d['incubation_time'], labels=d.get('labels'), stnd_scaler=d.get('stnd_scaler'))
        X = d['X']
        X = X.to_dense() if X.is_sparse else X
        mask = np.stack([np.asarray(m.todense()) if hasattr(m, 'todense') else np.asarray(m) for m in d['mask']]).astype(bool)
        return cls(X[:, 0].contiguous(), name=d.get('name', name), mask=mask, temporal_context=d.get('temporal_context', 2),
                   tilesize=d.get('tilesize', 512), device=device, pixelsize=d.get('pixelsize'), dt=d.get('dt'),
                   incubation_time=d.get('incubation_time'))

    # ------------------------------------------------------------------ host-resident input (Timelapse.py:205-326 + 492-566)
    @classmethod
    def from_host_u16(cls, raw, name='timelapse', mask=None, offset=121, clip=55, log_correct=True, scale=0.015176106,
                      chunk_frames=96, device='cuda:0', **kw):
        """A timelapse whose raw uint16 frames [T_all,H,W] still sit in HOST memory (pinned here if they are not), as the
        reference's inference() starts from (its Timelapse is a host object; construct_tiles copies to the device,
        Timelapse.py:492-566). Nothing is copied yet: AxonDetections.detect_dataset() streams the frames in chunks of
        `chunk_frames` -- H2D copies on a second stream into two staging buffers, the fused preprocessing pass
        (axt_preprocess_u16) into this object's frame buffer and the CNN of the detection frames a chunk completes, so the
        copy of chunk k + 1 runs beside the kernels of chunk k. Afterwards the object is an ordinary resident Timelapse.
        mask: [H,W] or None (a mask per frame needs the resident path: prepare_input_data)."""
        a = raw if isinstance(raw, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(raw)).view(np.int16))
        if a.dtype == torch.uint16:
            a = a.view(torch.int16)
        if a.dtype != torch.int16 or a.dim() != 3:
            raise TypeError('raw timelapses are uint16 [T_all,H,W]')
        if mask is not None and np.asarray(mask).ndim != 2:
            raise ValueError('from_host_u16 takes a static [H,W] mask; a mask per frame goes through prepare_input_data')
        self = cls.__new__(cls)
        T, H, W = a.shape
        dev = torch.device(device)
        frames = torch.empty((T, H, W), dtype=torch.float32, device=dev)
        cls.__init__(self, frames, name=name, mask=mask, device=device, **kw)
        self.frames = frames                                            # (the constructor keeps the same storage)
        self._host_raw = a if a.is_pinned() else a.pin_memory()
        self._source = _HostFrames(self._host_raw)
        self._set_streaming(mask, offset, clip, log_correct, scale, chunk_frames, dev)
        return self

    def _set_streaming(self, mask, offset, clip, log_correct, scale, chunk_frames, dev):
        off = 0.0 if not offset else (offset / 2 ** 16 if isinstance(offset, int) else float(offset))
        lo = 0.0 if not clip else (clip / 2 ** 16 if isinstance(clip, int) else float(clip))
        m = None if mask is None else torch.from_numpy(np.ascontiguousarray(np.asarray(mask).astype(np.uint8))).to(dev)
        self._pre = (m, off, lo, bool(log_correct), float(scale))
        self._chunk = max(int(chunk_frames), 2 * self.temporal_context + 1)
        self._pending = True

    @classmethod
    def from_tiff(cls, path, name='timelapse', mask=None, offset=121, clip=55, log_correct=True, scale=0.015176106,
                  chunk_frames=96, device='cuda:0', **kw):
        """The streaming twin of from_host_u16 for a TIFF file (tiff.py): nothing is read yet but the tags. In
        stream_chunks each 64-frame piece is "H2D of that piece's strip bytes, still compressed, then the decode launch into
        the raw buffer" on the copy stream, followed by the piece's event; everything downstream of the raw buffer is the
        same. The strips' statuses are read once after the last chunk: a strip that does not decode raises TiffError
        there. A file this reader refuses raises TiffUnsupported here."""
        from .tiff import tiff_info
        if mask is not None and np.asarray(mask).ndim != 2:
            raise ValueError('from_tiff takes a static [H,W] mask; a mask per frame goes through prepare_input_data')
        info = tiff_info(path)
        self = cls.__new__(cls)
        dev = torch.device(device)
        frames = torch.empty(info.shape, dtype=torch.float32, device=dev)
        cls.__init__(self, frames, name=name, mask=mask, device=device, **kw)
        self.frames = frames
        self._host_raw = None
        self._source = _TiffStrips(info, dev)
        self._set_streaming(mask, offset, clip, log_correct, scale, chunk_frames, dev)
        return self

    def stream_chunks(self):
        """Generator over the chunks of a host-resident timelapse (from_host_u16) or of one still in its TIFF file (from_tiff:
        where this says "copy", read "copy of the strips' bytes and their decode launch"). All H2D copies are enqueued at once on a copy stream, in
        pieces of 16 frames (64 from a TIFF file) into a device buffer for the raw timelapse (2 bytes per pixel; no staging buffer to recycle), each
        followed by an event. The compute (current) stream then takes the frames in chunks that GROW -- 16, 32, 48, 64, 80 frames,
        then `chunk_frames` -- so that the first kernels start after ~0.17 ms of copying while later chunks are large enough
        for full launches (PCIe delivers a 512x512 frame in 10.6 us, the detector needs ~14 us for it: the copies stay ahead
        of a schedule that grows no faster than that ratio allows; profiles/r03j_trace). Per chunk: wait for its last piece, the fused preprocessing pass into the frame buffer, the
        tile occupancy; then yields (first frame, one past last frame, occupancy bytes so far) so that the caller can
        enqueue the work the chunk completes. Leaves the frames resident."""
        from . import hotpath as hp
        dev = self.frames.device
        T, H, W = self.frames.shape
        source = self._source                            # where the raw pieces come from: host frames, or a TIFF file's strips
        piece = source.piece
        ramp = tuple(int(v) for v in os.environ.get('AXT_STREAM_RAMP', '16,32,48,64,80').split(','))      # tuning knob (bench experiments)
        copy_stream = _copy_stream(dev)
        compute = torch.cuda.current_stream(dev)
        copy_stream.wait_stream(compute)                 # (the stream is shared between timelapses: start behind what is queued)
        d_raw = torch.empty((T, H, W), dtype=torch.int16, device=dev)
        landed = []

        def enqueue_copies(upto):                       # pieces covering frames [.., upto)
            with torch.cuda.stream(copy_stream):
                while len(landed) * piece < min(upto, T):
                    a0 = len(landed) * piece
                    source.enqueue(d_raw, a0, min(a0 + piece, T))
                    landed.append(copy_stream.record_event())
        m, off, lo, logc, scale = self._pre
        a, k = 0, 0
        sizes = lambda kk: min(ramp[kk], self._chunk) if kk < len(ramp) else self._chunk
        while a < T:
            n = sizes(k)
            b = min(a + n, T)
            if T - b < 16:                               # (no tail chunk of a few frames)
                b = T
            # the copies of this chunk and of the next one are in the copy queue before this chunk's kernels are enqueued (all
            # of them up front would keep the host busy for ~0.5 ms before the first kernel launch)
            enqueue_copies(b + sizes(k + 1) + piece)
            compute.wait_event(landed[(b - 1) // piece])
            hp.preprocess_u16(d_raw[a:b], m, off, lo, logc, scale, out=self.frames[a:b])
            occ = None
            if b == T:
                # the kept-tile list (one pass over the finished frames) goes to the host on the copy stream, behind this
                # point of the compute stream only: the host does not wait for the CNN launches the caller enqueues for
                # this last chunk
                occ = hp.tile_occupancy_bytes(self.frames)
                ready = compute.record_event()
                self._occ_host = _pinned_bytes(int(occ.numel()))
                with torch.cuda.stream(copy_stream):
                    copy_stream.wait_event(ready)
                    self._occ_host.copy_(occ, non_blocking=True)
                    self._occ_done = copy_stream.record_event()
            yield a, b, occ
            a, k = b, k + 1
        d_raw.record_stream(copy_stream)
        source.finish()                                  # (a TIFF source reads its statuses here, once; raises on a bad strip)
        self._pending = False
        self._host_raw = self._source = None

    def make_resident(self):
        """A host-resident timelapse (from_host_u16) holds an UNINITIALISED frame buffer until its chunks have been streamed:
        everything that reads `frames` other than detect_dataset's own streaming loop (the tile list, the dataset cache, the
        appearance histograms, the occupancy all-reduce) calls this first. A no-op for a resident timelapse."""
        if getattr(self, '_pending', False):
            for _ in self.stream_chunks():
                pass
        return self

    @property
    def tile_yx(self):
        """Row-major list of the (tile_row, tile_col) that hold a non-zero pixel at some time point: the reference's
        tile_info, which construct_tiles computes once when the dataset is built (Timelapse.py:551-558), not in
        inference(). Computed on the GPU (axt_tile_occupancy) on first use and kept with the timelapse."""
        if getattr(self, '_tile_yx', None) is None:
            from . import hotpath as hp
            self.make_resident()
            self._tile_yx = hp.tile_occupancy(self.frames)
        return self._tile_yx

    def sync_tile_occupancy(self, group=None):
        """Frame-sharded runs: this object holds one rank's block of frames, but the reference decides which tiles
        are empty over the WHOLE timelapse (non_empty_tiles.any over all time points, Timelapse.py:551-558). One MAX
        all-reduce of the occupancy bytes gives every rank the timelapse-wide tile list -- and with it the same
        n_tiles, hence the same detection capacity, which the all-gather of the detections relies on."""
        import torch.distributed as dist
        from . import hotpath as hp
        self.make_resident()
        occ = hp.tile_occupancy_bytes(self.frames)
        # this object holds one rank's block of frames (what reads whole timelapses, training.fine_tune_head, refuses it)
        self.frame_sharded = dist.is_initialized() and dist.get_world_size(group) > 1
        if dist.is_initialized() and dist.get_world_size(group) > 1:
            if dist.get_backend(group) == 'gloo':
                occ_h = occ.cpu()
                dist.all_reduce(occ_h, op=dist.ReduceOp.MAX, group=group)
                occ = occ_h
            else:
                dist.all_reduce(occ, op=dist.ReduceOp.MAX, group=group)
        self._tile_yx = hp.tile_list(occ, self.sizey, self.sizex)
        return self._tile_yx

    @property
    def device(self):
        return self.frames.device


class _HostFrames:
    """Piece source of stream_chunks: raw frames in pinned host memory, 16 frames a piece. enqueue() runs on the copy stream."""
    piece = 16

    def __init__(self, host_raw):
        self.host_raw = host_raw

    def enqueue(self, d_raw, a0, a1):
        d_raw[a0:a1].copy_(self.host_raw[a0:a1], non_blocking=True)

    def finish(self):
        pass


class _TiffStrips:
    """Piece source of stream_chunks: the strips of a TIFF file (tiff.SegmentPacker). A piece is the H2D copy of its strips'
    packed bytes and the decode launch into the raw buffer, both on the copy stream; a little-endian uncompressed file
    without predictor is the copy alone. The pinned buffers live until finish(), which reads every status once.
    64 frames a piece: one wave decodes one strip, and a launch over the few hundred strips of 16 frames leaves most of
    the device idle for as long as one strip takes (the decode against the number of segments)."""
    piece = 64

    def __init__(self, info, dev):
        from .tiff import SegmentPacker
        self.info, self.packer, self.keep = info, SegmentPacker(info), []
        self.status = torch.zeros(max(info.n_segments, 1), dtype=torch.int32, device=dev)

    def enqueue(self, d_raw, a0, a1):
        from . import hotpath as hp
        info, packer = self.info, self.packer
        view, host, segs, total = packer.pack(a0, a1)
        chunk = d_raw[a0:a1]
        self.keep.append(host)
        if packer.plain and total == chunk.numel() * 2 and np.array_equal(segs['src_offset'], segs['dst_offset'] * 2):
            chunk.view(torch.uint8).view(-1).copy_(host[:total], non_blocking=True)
            return
        d_src = host.to(d_raw.device, non_blocking=True)
        s0, s1 = packer.segments(a0, a1)
        d_segs = hp.tiff_decode_launch(d_src, segs, info.shape[2], packer.device_compression, info.predictor,
                                       info.byteorder == '>', chunk, self.status[s0:s1])
        self.keep += [d_src, d_segs]

    def finish(self):
        from . import hotpath as hp
        info = self.info
        try:
            hp.tiff_raise_on_status(self.status[:info.n_segments], info.frame, info.row0, info.path)
        finally:
            self.keep = []


_PINNED = {}
_COPY_STREAMS = {}


def _copy_stream(dev):
    """One copy stream per device, created once (creating a stream costs as much as a small kernel)."""
    key = str(dev)
    if key not in _COPY_STREAMS:
        _COPY_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _COPY_STREAMS[key]


def _pinned_bytes(n):
    """A pinned host byte buffer of n bytes, allocated once per size (pinning costs ~100 us, more than the copy it serves)."""
    if n not in _PINNED:
        _PINNED[n] = torch.empty((n,), dtype=torch.uint8, pin_memory=True)
    return _PINNED[n]


def _raw_on_device(imseq, mask, offset, clip, device):
    """What preprocess and estimate_stnd_scaler hand to the kernels: (raw counts on the device as int16 bits [T,H,W], the
    static mask as a u8 tensor or None, offset and clip in [0,1] units). A mask per frame zeroes the raw counts."""
    if isinstance(imseq, torch.Tensor):          # read_tiff's output: already raw counts, on a device or not; no host round trip
        a = imseq.view(torch.int16) if imseq.dtype == torch.uint16 else imseq
        if a.dtype != torch.int16:
            raise TypeError(f'raw timelapses are uint16 (got {imseq.dtype}); pass preprocessed float32 frames to Timelapse directly')
        if a.dim() != 3:
            raise ValueError(f'raw timelapses are [T,H,W], got {tuple(a.shape)}')
        raw = a.to(device)
    else:
        a = np.asarray(imseq)
        if a.dtype != np.uint16:
            raise TypeError(f'raw timelapses are uint16 (got {a.dtype}); pass preprocessed float32 frames to Timelapse directly')
        if a.ndim != 3:
            raise ValueError(f'raw timelapses are [T,H,W], got {a.shape}')
        raw = torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(device)
    off = 0.0 if not offset else (offset / 2 ** 16 if isinstance(offset, int) else float(offset))
    lo = 0.0 if not clip else (clip / 2 ** 16 if isinstance(clip, int) else float(clip))
    m = None
    if mask is not None:
        mk = np.asarray(mask).astype(bool)
        if mk.ndim == 3:                      # a mask per frame: zero the raw counts, which is what masking the floats does
            if mk.shape != tuple(a.shape):
                raise ValueError(f'a time-varying mask must match the timelapse {tuple(a.shape)}, got {mk.shape}')
            raw = raw * torch.from_numpy(mk).to(device=device, dtype=torch.int16)
        else:
            m = torch.from_numpy(np.ascontiguousarray(mk.astype(np.uint8)))
    return raw.contiguous(), m, off, lo


def preprocess(imseq, mask=None, offset=121, clip=55, log_correct=True, scale=0.015176106, device='cuda:0', pad=None):
    """Dense preprocessing of a raw uint16 timelapse as Timelapse._read_tiff / _clip_image_values /
    _log_adjust_image / _standardize do it (Timelapse.py:205-326), as one fused HIP pass
    (axt_preprocess_u16): u16 -> f32 in [0,1], mask, subtract offset/2^16 and clamp at 0, zero below
    clip/2^16, log2(1+x), divide by the train-set std. `img_as_float32` and `adjust_log` are skimage
    functions that are absent here: their arithmetic (x * (1/65535), log2(1+x)) is restated from the
    published skimage 0.18 behaviour, PARITY UNPINNED (a "next" row).
    mask: [H,W] or one per frame [T,H,W] (Timelapse.py:210-217). pad: None or (top, right, bottom, left) -- zero
    margins added after masking and offsetting (Timelapse.py:224-234); zero stays zero through the clip, the log and
    the scaling, so the margins are added to the finished frames. Returns f32 [T, H + top + bottom, W + left + right].
    scale: one number, or one per frame (STANDARDIZE_FRAMEWISE, Timelapse.py:309-312: axt_preprocess_u16_framewise)."""
    from . import hotpath as hp
    raw, m, off, lo = _raw_on_device(imseq, mask, offset, clip, device)
    if np.ndim(scale) == 0:
        out = hp.preprocess_u16(raw, m, off, lo, bool(log_correct), float(scale))
    else:
        out = hp.preprocess_u16_framewise(raw, scale, m, off, lo, bool(log_correct))
    if pad is not None and any(pad):
        top, right, bottom, left = (int(v) for v in pad)
        out = torch.nn.functional.pad(out, (left, right, top, bottom)).contiguous()
    return out


STANDARDIZE_MODES = ('zscore', '0to1')


def scaler_from_stats(n, sum_, sumsq, max_, standardize='zscore', framewise=False):
    """Timelapse._standardize's scaler (Timelapse.py:286-302) from the per-frame statistics of the preprocessed, not yet
    scaled frames -- n non-zero values, their sum, their sum of squares, the frame's maximum -- in f64 on the host:
    mean = sum / n, std = sqrt(sumsq / n - mean^2), the population std np.std(frame.data) takes of the non-zero values.
    -> (stnd_scaler, per_frame DataFrame (n, mean, std, max), frame scales f64 [T] for framewise or None).
    'zscore': var_scalar = mean of the stds, mean_scalar = mean of the means; '0to1': var_scalar = max of the maxima,
    mean_scalar = 0. Not framewise: (name, (var_scalar, mean_scalar)); framewise: (name, None) and the per-frame std /
    max are the scales. Where the reference would divide by NaN or 0 -- 'zscore' with a frame without a non-zero pixel, a
    scale of 0 -- this raises ValueError naming the frames."""
    import pandas as pd
    if standardize not in STANDARDIZE_MODES:
        raise ValueError(f'standardize must be one of {STANDARDIZE_MODES}, got {standardize!r}')
    n = np.asarray(n, np.int64)
    s, q, mx = (np.asarray(v, np.float64) for v in (sum_, sumsq, max_))
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = s / n
        # sumsq / n - mean^2 cancels: what it leaves of a frame of equal values is summation error, at most a few
        # n * 2^-53 of sumsq / n. A variance down there is 0 (and then refused as a frame scale), not a tiny scale.
        var = q / n - mean * mean
        std = np.sqrt(np.where(var <= 4.0 * n * 2.0 ** -53 * (q / n), 0.0, var))
    per_frame = pd.DataFrame({'n': n, 'mean': mean, 'std': std, 'max': mx})
    if standardize == 'zscore' and (n == 0).any():
        raise ValueError(f"'zscore' needs a non-zero pixel in every frame; frames {np.flatnonzero(n == 0).tolist()} have none "
                         f'(the reference would scale by NaN)')
    frame_scale = std if standardize == 'zscore' else mx
    if framewise:
        bad = ~(np.isfinite(frame_scale) & (frame_scale > 0))
        if bad.any():
            raise ValueError(f'frame-wise {standardize!r}: the scale of frames {np.flatnonzero(bad).tolist()} would be 0')
        return (standardize, None), per_frame, frame_scale.copy()
    if standardize == 'zscore':
        var_scalar, mean_scalar = float(np.mean(std)), float(np.mean(mean))
    else:
        var_scalar, mean_scalar = float(np.max(mx)), 0.0
    if not (np.isfinite(var_scalar) and var_scalar > 0):
        raise ValueError(f'{standardize!r}: the scale of the timelapse would be {var_scalar} (frames without contrast)')
    return (standardize, (var_scalar, mean_scalar)), per_frame, None


def estimate_stnd_scaler(imseq, mask=None, offset=None, clip=None, log_correct=True, standardize='zscore', framewise=False,
                         device='cuda:0'):
    """The standardisation scaler of a raw uint16 timelapse [T,H,W], as Timelapse._standardize computes it from the
    training data (Timelapse.py:277-302) -> (stnd_scaler, per_frame). One pass over the raw counts
    (axt_preprocess_stats_u16: the preprocessing arithmetic of `preprocess` at scale 1, reduced per frame to n, sum,
    sumsq, max without writing a frame); the rest is scaler_from_stats on the host. All frames take part. per_frame:
    DataFrame (n, mean, std, max), one row per input frame; with framewise=True its 'std' ('zscore') or 'max' ('0to1')
    column is what `preprocess(scale=...)` takes as the frames' scales."""
    from . import hotpath as hp
    if standardize not in STANDARDIZE_MODES:
        raise ValueError(f'standardize must be one of {STANDARDIZE_MODES}, got {standardize!r}')
    raw, m, off, lo = _raw_on_device(imseq, mask, offset, clip, device)
    st = hp.preprocess_stats_u16(raw, m, off, lo, bool(log_correct))
    scaler, per_frame, _ = scaler_from_stats(st['n'], st['sum'], st['sumsq'], st['max'], standardize, framewise)
    return scaler, per_frame


def frame_scales(stnd_scaler, per_frame):
    """What `preprocess(scale=...)` takes for a scaler: the one number, or for (name, None) the per-frame column."""
    if stnd_scaler[1] is not None:
        return float(stnd_scaler[1][0])
    return per_frame['std' if stnd_scaler[0] == 'zscore' else 'max'].to_numpy(np.float64)


def load_labels_csv(fname, pad=None, shape=None):
    """The reference's axon_anchor_labels.csv as Timelapse._load_bboxes reads it (Timelapse.py:377-383): two header rows
    (axon name, property), the frame number as index; the (axon, 'anchor_x' | 'anchor_y') columns are kept, the rows sorted
    by index and renumbered, pad[0] added to y and pad[3] to x (pad: top, right, bottom, left).
    -> per input frame (x, y, ids), int64 arrays. NaN means the axon is absent in that frame; values are truncated toward
    zero (construct_tiles' fillna(-1).astype(int), :514). A label left of or above the frame is dropped, and with
    shape=(H, W) of the padded frame so is one right of or below it: construct_tiles assigns those to no tile (:532-534).
    ids: the trailing integer of the axon's column name when every name has one and they are distinct, else the column
    position."""
    import re
    import pandas as pd
    bboxes = pd.read_csv(fname, index_col=0, header=[0, 1])
    bboxes = bboxes.loc[:, (slice(None), ['anchor_x', 'anchor_y'])].sort_index().reset_index(drop=True)
    names = list(dict.fromkeys(bboxes.columns.get_level_values(0)))
    lone = [a for a in names if not {(a, 'anchor_x'), (a, 'anchor_y')} <= set(bboxes.columns)]
    if lone:
        raise ValueError(f'{fname}: axons {lone} lack anchor_x or anchor_y')
    tails = [re.search(r'(\d+)$', str(a)) for a in names]
    ids = np.array([int(m.group(1)) for m in tails], np.int64) if all(tails) else None
    if ids is None or len(set(ids.tolist())) != len(ids):
        ids = np.arange(len(names), dtype=np.int64)
    x = np.stack([bboxes[(a, 'anchor_x')].to_numpy(np.float64) for a in names], 1) if names else np.zeros((len(bboxes), 0))
    y = np.stack([bboxes[(a, 'anchor_y')].to_numpy(np.float64) for a in names], 1) if names else np.zeros((len(bboxes), 0))
    if pad is not None and (pad[0] or pad[3]):
        y, x = y + int(pad[0]), x + int(pad[3])
    present = ~(np.isnan(x) | np.isnan(y))
    xi = np.where(present, np.trunc(np.nan_to_num(x)), -1).astype(np.int64)
    yi = np.where(present, np.trunc(np.nan_to_num(y)), -1).astype(np.int64)
    keep = present & (xi >= 0) & (yi >= 0)
    if shape is not None:
        keep &= (xi < int(shape[1])) & (yi < int(shape[0]))
    return [(xi[t, keep[t]], yi[t, keep[t]], ids[keep[t]]) for t in range(len(bboxes))]


def contiguous_runs(timepoints):
    """Sorted distinct time points -> list of (first, last) of their runs of consecutive numbers."""
    tp = sorted({int(t) for t in timepoints})
    runs = []
    for t in tp:
        if runs and t == runs[-1][1] + 1:
            runs[-1][1] = t
        else:
            runs.append([t, t])
    return [tuple(r) for r in runs]


def pad_mask(mask, pad, shape):
    """The mask of a padded timelapse (Timelapse.py:231-234): zeros in the margins; an absent mask becomes the all-ones
    mask of the unpadded frame, so the margins are off the mask for the path searches exactly as in the reference."""
    top, right, bottom, left = (int(v) for v in pad)
    T, H, W = shape
    m = np.ones((H, W), bool) if mask is None else np.asarray(mask).astype(bool)
    width = ((top, bottom), (left, right))
    return np.pad(m, width if m.ndim == 2 else ((0, 0),) + width)
