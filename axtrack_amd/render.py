"""Annotated frames of a tracking result (video_plotting.py: draw_all, setup_frame_drawing, draw_frame, draw_detections)
and a dependency-free PNG / APNG writer. The pixels are drawn by one HIP kernel (axt_render_frames, csrc/render.hip);
this module gathers what it draws -- boxes, labels, header, trail cells -- and bins it by output tile. DESIGN.md 6.8b
states the rules.

Layout constants (output pixels, s = the font scale):
  label: glyphs of f'Ax{n:03}' from (x0, y0 - 8s), x0 / y0 the box's top-left corner (one s gap above the box);
  text: 5 x 7 glyphs at scale s, advance 6s; header lines right-aligned to Wo - 4s, line k from y = 4s + 9s k;
  scale bar: rint(200 / pixelsize) x 2s at y = 4s + 9s n_lines + s, right end Wo - 4s, caption '200 um' 2s below it."""
import colorsys
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np
import torch

from . import hotpath as hp

# the reference's hsv colormap with 20 entries (video_plotting.py:292-293), as the pure HSV hues k/20
PALETTE = np.array([[int(round(c * 255)) for c in colorsys.hsv_to_rgb(k / 20, 1.0, 1.0)] for k in range(20)], np.uint8)
WHITE_ALPHA_GRID, WHITE_ALPHA_GT, BG_ALPHA_DIM = 38, 154, 26
HEADER_RGB = (107, 107, 107)
LAYER_BOX, LAYER_LABEL, LAYER_HEADER = 1, 2, 3
P_DASHED, P_SOLID, P_GLYPH, P_RECT, P_TARGET = 0, 1, 2, 3, 4
TARGET_PATH_RGB, TARGET_RGB = (217, 217, 217), (255, 255, 255)
TGT_PATH, TGT_CELL = 1, 2          # keys of the P_TARGET rectangles

# 5 x 7 font of printable ASCII 32..126: five column bytes per glyph, bit 0 = top row (the classic LCD character set)
_FONT_COLUMNS = bytes.fromhex(
    '0000000000' '00005f0000' '0007000700' '147f147f14' '242a7f2a12' '2313086462' '3649552250' '0005030000'
    '001c224100' '0041221c00' '082a1c2a08' '08083e0808' '0050300000' '0808080808' '0060600000' '2010080402'
    '3e5149453e' '00427f4000' '4261514946' '2141454b31' '1814127f10' '2745454539' '3c4a494930' '0171090503'
    '3649494936' '064949291e' '0036360000' '0056360000' '0814224100' '1414141414' '0041221408' '0201510906'
    '324979413e' '7e1111117e' '7f49494936' '3e41414122' '7f4141221c' '7f49494941' '7f09090101' '3e41415132'
    '7f0808087f' '00417f4100' '2040413f01' '7f08142241' '7f40404040' '7f0204027f' '7f0408107f' '3e4141413e'
    '7f09090906' '3e4151215e' '7f09192946' '4649494931' '01017f0101' '3f4040403f' '1f2040201f' '7f2018207f'
    '6314081463' '0304780403' '6151494543' '007f414100' '0204081020' '0041417f00' '0402010204' '4040404040'
    '0001020400' '2054545478' '7f48444438' '3844444420' '384444487f' '3854545418' '087e090102' '0814545478'
    '7f08040478' '00447d4000' '2040443d00' '007f102844' '00417f4000' '7c04180478' '7c08040478' '3844444438'
    '7c14141408' '081414187c' '7c08040408' '4854545420' '043f444020' '3c4040207c' '1c2040201c' '3c4030403c'
    '4428102844' '0c5050503c' '4464544c44' '0008364100' '00007f0000' '0041360800' '1008081008')


def _glyph_rows():
    cols = np.frombuffer(_FONT_COLUMNS, np.uint8).reshape(95, 5)
    rows = np.zeros((95, 7), np.uint8)
    for r in range(7):
        for c in range(5):
            rows[:, r] |= ((cols[:, c] >> r) & 1) << (4 - c)
    return rows


GLYPH_ROWS = _glyph_rows()          # u8 [95, 7]: row r of glyph (char - 32), bit 4 = leftmost column
_TABLES = {}


def _tables(device):
    key = str(device)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(np.concatenate([PALETTE.ravel(), GLYPH_ROWS.ravel()])).to(device)
    return _TABLES[key]


def font_scale(H, W):
    """Text scale of a frame (not of a slice, so that a slice stays a crop)."""
    return max(1, min(int(H), int(W)) // 512)


def label_text(n):
    """'Axon_007'.replace('on_', '') (video_plotting.py:298)."""
    return f'Ax{int(n):03}'


def header_lines(description, t, T, dt=None, incubation_time=None):
    """The header of detection frame t of T: the description (if any), 'frame t/T', and with dt and incubation_time the
    DIV of Timelapse.get_DIV_point (relativedelta(minutes=incubation + dt t): whole days, then hours)."""
    lines = [description] if description else []
    lines.append(f'frame {t:03}/{T:03}')
    if dt and incubation_time:
        m = float(incubation_time) + float(dt) * t
        lines.append(f'DIV {int(m // 1440)} days - {int((m % 1440) // 60)} hours')
    return lines


def scalebar_px(pixelsize):
    return int(np.rint(200.0 / float(pixelsize)))


def _text_prims(strings, frame_idx, x0, y0, s, key):
    """Glyph primitives of one string per entry (left edge x0, top y0): rows (i, x, y, kind, a, b, key)."""
    if not len(strings):
        return np.zeros((0, 7), np.int64)
    lens = np.array([len(t) for t in strings], np.int64)
    codes = np.frombuffer(''.join(strings).encode('utf-32-le'), np.uint32).astype(np.int64) if lens.sum() else np.zeros(0, np.int64)
    which = np.repeat(np.arange(len(strings)), lens)
    k = np.arange(len(codes)) - np.repeat(np.cumsum(lens) - lens, lens)
    ok = (codes >= 32) & (codes <= 126) & (codes != 32)           # (a space draws nothing; it only advances)
    which, k, codes = which[ok], k[ok], codes[ok]
    n = len(codes)
    return np.stack([np.asarray(frame_idx, np.int64)[which], np.asarray(x0, np.int64)[which] + 6 * s * k,
                     np.asarray(y0, np.int64)[which], np.full(n, P_GLYPH), codes - 32, np.full(n, s),
                     np.asarray(key, np.int64)[which]], 1)


def _bin(i, x0, y0, w, h, Ho, Wo, rt, n_out):
    """Every (output frame i, tile) a primitive's box [x0, x0+w) x [y0, y0+h) touches: (element index, bin) sorted by bin."""
    xa, xb = np.maximum(x0, 0), np.minimum(x0 + w, Wo) - 1
    ya, yb = np.maximum(y0, 0), np.minimum(y0 + h, Ho) - 1
    keep = (xa <= xb) & (ya <= yb)
    idx = np.nonzero(keep)[0]
    tx0, tx1, ty0, ty1 = xa[idx] // rt, xb[idx] // rt, ya[idx] // rt, yb[idx] // rt
    wt = tx1 - tx0 + 1
    cnt = wt * (ty1 - ty0 + 1)
    rep = np.repeat(np.arange(len(idx)), cnt)
    k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ntx = -(-Wo // rt)
    tiles = (ty0[rep] + k // wt[rep]) * ntx + tx0[rep] + k % wt[rep]
    bins = np.asarray(i, np.int64)[idx[rep]] * (ntx * -(-Ho // rt)) + tiles
    order = np.argsort(bins, kind='stable')
    return idx[rep][order], bins[order]


def _csr(bins, n_bins):
    return np.concatenate([[0], np.cumsum(np.bincount(bins, minlength=n_bins))]).astype(np.int32)


def _boxes(dets, which_dets, ts, subset):
    """(output index i, x, y, n) of the boxes of get_frame_dets(which_dets, t) for the output frames ts."""
    inv = np.full(len(dets), -1, np.int64)
    inv[ts] = np.arange(len(ts))
    if which_dets == 'IDed':
        frame, ids, _, x, y = dets.ided_arrays()          # the rows of _IDed_detections (true frame, no label quirk)
        frame, ids, x, y = (np.asarray(a, np.int64) for a in (frame, ids, x, y))
        sel = inv[frame] >= 0
        i, x, y, n = inv[frame[sel]], x[sel], y[sel], ids[sel]
        if subset is not None:
            ok = np.isin(n, subset)
            i, x, y, n = i[ok], x[ok], y[ok], n[ok]
        return i, x, y, n
    parts = []
    for k, t in enumerate(ts):
        d = dets.get_frame_dets(which_dets, int(t))
        if not len(d):
            continue
        pos = np.arange(len(d), dtype=np.int64)
        if subset is not None:
            pos = pos[np.isin(np.array([_number(a) for a in d.index]), subset)]
        parts.append((np.full(len(pos), k, np.int64), d.anchor_x.to_numpy(np.int64)[pos], d.anchor_y.to_numpy(np.int64)[pos],
                      pos))
    if not parts:
        return tuple(np.zeros(0, np.int64) for _ in range(4))
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(4))


def _number(name):
    return int(str(name).split('_')[-1])


def _trail_cells(dets, t_last, subset):
    """(frame, key, x, y, colour index) of every cell get_axon_reconstructions(t=t_last, include_history=True) returns:
    key = 1 + rank of the segment's (head frame, axon number), so the larger pair has the larger key."""
    from .detections import _recon_segments
    r = dets.reconstruction_arrays(True)
    seg = _recon_segments(r, True)
    keep = (seg['n'] > 0) & (seg['frame'] <= t_last)
    if subset is not None:
        keep &= np.isin(seg['axon'], subset)
    axon, frame, start, n = seg['axon'][keep], seg['frame'][keep], seg['start'][keep], seg['n'][keep]
    order = np.lexsort((axon, frame))
    key = np.empty(len(order), np.int64)
    key[order] = np.arange(1, len(order) + 1)
    col = np.zeros(len(order) + 1, np.uint8)
    col[key] = (axon % 20).astype(np.uint8)
    segi = np.repeat(np.arange(len(n)), n)
    c = r['cells'][start[segi] + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)]
    W = r['shape'][1]
    return frame[segi], key[segi], c % W, c // W, col


def _run_rects(ys, xs, pid):
    """The 5 x 5 squares of the cells of paths, with every straight run merged: cells (ys, xs) of all paths one after the
    other, pid = the path of every cell. A horizontal or vertical run of k cells becomes ONE (k + 4) x 5 (5 x (k + 4))
    rectangle; cells that only diagonal steps touch keep their own square. Returns (first cell index, x0, y0, w, h) of the
    rectangles: together exactly the pixels of the per-cell squares."""
    ys, xs, pid = (np.asarray(a, np.int64) for a in (ys, xs, pid))
    n = len(ys)
    if n == 0:
        return tuple(np.zeros(0, np.int64) for _ in range(5))
    dy, dx = np.diff(ys), np.diff(xs)
    straight = (pid[1:] == pid[:-1]) & (np.abs(dy) + np.abs(dx) == 1)
    cont = np.zeros(n - 1, bool)                                   # step k continues the run of step k - 1
    cont[1:] = straight[1:] & straight[:-1] & (dy[1:] == dy[:-1]) & (dx[1:] == dx[:-1])
    first = np.nonzero(straight & ~cont)[0]
    goes_on = np.zeros(n - 1, bool)                                # step k + 1 continues the run of step k
    goes_on[:-1] = cont[1:]
    last = np.nonzero(straight & ~goes_on)[0] + 1                  # (index of the run's last CELL)
    covered = np.zeros(n, bool)
    covered[:-1] |= straight
    covered[1:] |= straight
    single = np.nonzero(~covered)[0]
    a = np.r_[first, single]
    b = np.r_[last, single]
    return (a, np.minimum(xs[a], xs[b]) - 2, np.minimum(ys[a], ys[b]) - 2, np.abs(xs[b] - xs[a]) + 5,
            np.abs(ys[b] - ys[a]) + 5)


def _target_prims(dets, ts, subset, ymin, xmin):
    """The target layer's rectangles, rows (i, x0, y0, kind, a, b, key): the target paths of the drawn axons' detections
    (get_trg_path(t) of every output frame), then the target cells of every output frame."""
    W = dets.dataset.sizex
    inv = np.full(len(dets), -1, np.int64)
    inv[ts] = np.arange(len(ts))
    cnt = dets._host_dets()[0]
    cap = int(dets.d_x.shape[1])
    frame_of = np.repeat(np.arange(len(cnt)), cnt)
    idx_in = np.arange(len(frame_of)) - dets._offs[frame_of]
    track = dets._track_flat
    sel = (track >= 0) & (inv[frame_of] >= 0)
    if subset is not None:
        sel &= np.isin(track, subset)
    slots = frame_of[sel] * cap + idx_in[sel]
    ptr, cells = dets._target_paths()
    n = ptr[slots + 1] - ptr[slots]
    pid = np.repeat(np.arange(len(slots)), n)
    c = cells[np.repeat(ptr[slots], n) + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)]
    k, x0, y0, w, h = _run_rects(c // W - ymin, c % W - xmin, pid)
    i = inv[frame_of[sel]][pid[k]] if len(k) else k
    rows = [np.stack([i, x0, y0, np.full(len(k), P_TARGET), w, h, np.full(len(k), TGT_PATH)], 1)]
    tc = dets._target_cells
    _, x0, y0, w, h = _run_rects(tc // W - ymin, tc % W - xmin, np.zeros(len(tc), np.int64))
    one = np.stack([np.zeros(len(x0), np.int64), x0, y0, np.full(len(x0), P_TARGET), w, h, np.full(len(x0), TGT_CELL)], 1)
    for j in range(len(ts)):
        r = one.copy()
        r[:, 0] = j
        rows.append(r)
    return rows


def render_frames(dets, which_dets='IDed', t_y_x_slice=(None, None, None), draw_grid=True, draw_scalebar=False,
                  draw_axon_reconstructions=False, draw_true_dets=False, draw_brightened_bg=False, axon_subset=None,
                  description='', annotate=True, draw_target_paths=False, _frames=None):
    """AxonDetections.render_frames (see there). _frames: the detection frames to draw (render_inference's chunks)."""
    ds = dets.dataset
    if dets._shard is not None:
        raise NotImplementedError('rendering a frame-sharded run is not implemented: render in a single process '
                                  '(AxonDetections without gather_detections)')
    if which_dets not in ('IDed', 'confident', 'all', 'groundtruth'):
        raise ValueError(f"which_dets must be 'IDed', 'confident', 'all' or 'groundtruth', got {which_dets!r}")
    T = len(dets)
    if ds.sizet != T:
        raise ValueError(f'the timelapse has {ds.sizet} detection frames, the detections {T}: render the timelapse the '
                         f'detections were made on')
    if draw_scalebar and not getattr(ds, 'pixelsize', None):
        raise ValueError('draw_scalebar needs the timelapse\'s pixelsize')
    if (draw_true_dets or which_dets == 'groundtruth') and not dets.labelled:
        raise ValueError('no labels: call set_groundtruth() first')
    if draw_axon_reconstructions and which_dets != 'IDed':
        raise ValueError("draw_axon_reconstructions goes with which_dets='IDed' (the reconstructions are the IDed tracks')")
    if draw_target_paths and which_dets != 'IDed':
        raise ValueError("draw_target_paths goes with which_dets='IDed' (the paths start at the IDed detections)")
    if which_dets == 'IDed' and not dets._solved:
        raise ValueError('no identities: run assign_ids() first (or the association was infeasible)')
    if draw_target_paths:
        dets._require_target(ids=True)
    H, W = ds.sizey, ds.sizex
    (tmin, tmax), (ymin, ymax), (xmin, xmax) = ((0, n) if v is None else tuple(v) for v, n in zip(t_y_x_slice, (T, H, W)))
    if not (0 <= tmin <= tmax <= T and 0 <= ymin < ymax <= H and 0 <= xmin < xmax <= W):
        raise ValueError(f't_y_x_slice {t_y_x_slice} lies outside the timelapse [0, {T}) x [0, {H}) x [0, {W})')
    ts = np.arange(tmin, tmax, dtype=np.int64) if _frames is None else np.asarray(_frames, np.int64)
    Ho, Wo = ymax - ymin, xmax - xmin
    ds.make_resident()
    dev = ds.frames.device
    if len(ts) == 0:
        return torch.empty((0, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    subset = None if axon_subset is None else np.array([_number(a) for a in axon_subset], np.int64)
    rt = hp.render_tile_size()
    ntiles = -(-Wo // rt) * -(-Ho // rt)
    s = font_scale(H, W)
    b = int(dets.axon_box_size)
    rows = []                                                     # (i, x0, y0, kind, a, b, key), output coordinates
    if draw_true_dets:
        gi, gx, gy, _ = _boxes(dets, 'groundtruth', ts, None)
        rows.append(np.stack([gi, gx - b // 2 - xmin, gy - b // 2 - ymin, np.full(len(gi), P_SOLID), np.full(len(gi), b),
                              np.zeros(len(gi), np.int64), np.zeros(len(gi), np.int64)], 1))
    i, x, y, n = _boxes(dets, which_dets, ts, subset)
    if len(n) and int(n.max()) >= (1 << 24) - 1:
        raise ValueError('axon numbers must stay below 2**24 - 1 to be drawn')
    bx, by = x - b // 2 - xmin, y - b // 2 - ymin
    rows.append(np.stack([i, bx, by, np.full(len(i), P_DASHED), np.full(len(i), b), np.zeros(len(i), np.int64),
                          (LAYER_BOX << 24) | (n + 1)], 1))
    if annotate:
        rows.append(_text_prims([label_text(v) for v in n], i, bx, by - 8 * s, s, (LAYER_LABEL << 24) | (n + 1)))
        strings, fi, hx, hy = [], [], [], []
        for k, t in enumerate(ts):
            lines = header_lines(description, int(t), T, getattr(ds, 'dt', None), getattr(ds, 'incubation_time', None))
            for j, line in enumerate(lines):
                strings.append(line); fi.append(k); hx.append(Wo - 4 * s - (6 * s * len(line) - s)); hy.append(4 * s + 9 * s * j)
        rows.append(_text_prims(strings, fi, hx, hy, s, np.full(len(strings), LAYER_HEADER << 24)))
        n_lines = len(header_lines(description, 0, T, getattr(ds, 'dt', None), getattr(ds, 'incubation_time', None)))
    else:
        n_lines = 0
    if draw_scalebar:
        L = scalebar_px(ds.pixelsize)
        yb = 4 * s + 9 * s * n_lines + s
        k = np.arange(len(ts))
        rows.append(np.stack([k, np.full(len(k), Wo - 4 * s - L), np.full(len(k), yb), np.full(len(k), P_RECT),
                              np.full(len(k), L), np.full(len(k), 2 * s), np.full(len(k), LAYER_HEADER << 24)], 1))
        cap = '200 um'
        rows.append(_text_prims([cap] * len(k), k, np.full(len(k), Wo - 4 * s - (6 * s * len(cap) - s)),
                                np.full(len(k), yb + 4 * s), s, np.full(len(k), LAYER_HEADER << 24)))
    if draw_target_paths:
        rows += _target_prims(dets, ts, subset, ymin, xmin)
    pr = np.concatenate([r.reshape(-1, 7) for r in rows]).astype(np.int64)
    ext_w = np.where(pr[:, 3] == P_GLYPH, 5 * pr[:, 5], pr[:, 4])
    ext_h = np.where(pr[:, 3] == P_GLYPH, 7 * pr[:, 5], np.where((pr[:, 3] == P_RECT) | (pr[:, 3] == P_TARGET), pr[:, 5], pr[:, 4]))
    idx, bins = _bin(pr[:, 0], pr[:, 1], pr[:, 2], ext_w, ext_h, Ho, Wo, rt, len(ts))
    prims = np.zeros((len(idx), 8), np.int32)
    prims[:, :6] = pr[idx, 1:7]
    prim_ptr = _csr(bins, len(ts) * ntiles)
    if draw_axon_reconstructions:
        tf, tk, tx, ty, tcol = _trail_cells(dets, int(ts.max()), subset)
        tx, ty = tx - xmin, ty - ymin
        cidx, cbin = _bin(np.zeros(len(tf), np.int64), tx - 2, ty - 2, np.full(len(tf), 5), np.full(len(tf), 5), Ho, Wo, rt, 1)
        order = np.lexsort((tf[cidx], cbin))                      # per tile, by frame
        cidx, cbin = cidx[order], cbin[order]
        trail = np.stack([tf[cidx], tk[cidx], tx[cidx], ty[cidx]], 1).astype(np.int32)
        trail_ptr = _csr(cbin, ntiles)
    else:
        trail, trail_ptr, tcol = np.zeros((0, 4), np.int32), np.zeros(ntiles + 1, np.int32), np.zeros(1, np.uint8)
    tc = ds.temporal_context
    mask, stride = None, 0
    if draw_brightened_bg:
        mask, stride = _mask_u8(ds)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return hp.render_frames(ds.frames[tc:], mask, stride, up(ts.astype(np.int32)), H, W, ymin, xmin, Ho, Wo,
                            ds.tilesize if draw_grid else 0, draw_brightened_bg, up(trail_ptr), up(trail), up(tcol),
                            up(prim_ptr), up(prims), _tables(dev))


def _mask_u8(ds):
    """(u8 device mask whose detection frame t starts t * stride elements in, stride): the mask of the detection frame
    itself (mask3d[t + context]; no mask-frame quirk), else mask2d, else None (all ones). Kept with the timelapse."""
    if ds.mask3d is None and ds.mask2d is None:
        return None, 0
    if getattr(ds, '_render_mask', None) is None:
        H, W = ds.sizey, ds.sizex
        if ds.mask3d is not None:
            m = torch.from_numpy(np.ascontiguousarray(ds.mask3d[ds.temporal_context:], np.uint8)).to(ds.frames.device)
            ds._render_mask = (m, H * W)
        else:
            ds._render_mask = (torch.from_numpy(np.ascontiguousarray(ds.mask2d, np.uint8)).to(ds.frames.device), 0)
    return ds._render_mask


# ---------------------------------------------------------------------------------------------- PNG / APNG writer
_PNG_SIG = b'\x89PNG\r\n\x1a\n'
_POOL_THREADS = 16                  # zlib releases the GIL; never sized from the machine's CPU count


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def _idat_payload(rgb, level=6):
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    raw = np.zeros((H, 1 + 3 * W), np.uint8)                      # filter type 0 (None) on every row
    raw[:, 1:] = rgb.reshape(H, 3 * W)
    return zlib.compress(raw.tobytes(), level)


def _ihdr(H, W):
    return _chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0))


def png_bytes(rgb):
    """One uint8 [H, W, 3] frame as PNG bytes."""
    H, W = rgb.shape[:2]
    return _PNG_SIG + _ihdr(H, W) + _chunk(b'IDAT', _idat_payload(rgb)) + _chunk(b'IEND', b'')


def _delay(fps):
    d = (Fraction(1) / Fraction(fps).limit_denominator(1000)).limit_denominator(65535)
    return d.numerator, d.denominator


def apng_bytes(payloads, H, W, fps=6):
    """An animated PNG from compressed frame payloads (_idat_payload): acTL (looping forever), fcTL before every frame with
    the delay 1/fps, frame 0 as IDAT (the still image), the others as fdAT."""
    num, den = _delay(fps)
    out = [_PNG_SIG, _ihdr(H, W), _chunk(b'acTL', struct.pack('>II', len(payloads), 0))]
    seq = 0
    for k, data in enumerate(payloads):
        out.append(_chunk(b'fcTL', struct.pack('>IIIIIHHBB', seq, W, H, 0, 0, num, den, 0, 0)))
        seq += 1
        if k == 0:
            out.append(_chunk(b'IDAT', data))
        else:
            out.append(_chunk(b'fdAT', struct.pack('>I', seq) + data))
            seq += 1
    out.append(_chunk(b'IEND', b''))
    return b''.join(out)


# the reference's draw_all keywords that have no meaning here, with their defaults (video_plotting.py:17-24)
_UNSUPPORTED = dict(show=False, dpi=160, save_single_tiles=False, dets_kwargs=None, scnd_dets_kwargs=None, draw_trg_paths=None)
_FRAME_BYTES_PER_CHUNK = 256 << 20


def render_inference(axon_dets, which_dets='IDed', dest_dir=None, animated=False, fps=6, anim_fname_postfix='',
                     t_y_x_slice=(None, None, None), video=False, quality=90, **kwargs):
    """visualize_inference / video_plotting.draw_all (interface.py:217-320, video_plotting.py:17-113) on the GPU: renders
    the frames with AxonDetections.render_frames in chunks of frames (at most 256 MB of RGB on the device at once) and
    writes '{dest_dir}/{name}_frame{t:03}of{T:03}.png' per frame, or with animated=True one animated PNG
    '{dest_dir}/{name}_dets{anim_fname_postfix}.png' at fps frames per second, or with video=True one MJPEG AVI
    '{dest_dir}/{name}_dets{anim_fname_postfix}.avi' (the reference's video name with this container's extension) whose
    frames are JPEG-encoded on the GPU at `quality` (jpeg.py). dest_dir: default the detections' directory. The drawing
    keywords are those of render_frames. Returns the list of paths written."""
    if video and animated:
        raise ValueError('video=True writes an MJPEG AVI, animated=True an animated PNG: ask for one of them')
    if video and not 1 <= int(quality) <= 100:
        raise ValueError(f'quality must lie in 1..100, got {quality!r}')
    for k, default in _UNSUPPORTED.items():
        if k in kwargs:
            v = kwargs.pop(k)
            if not (v is default or v == default):
                raise ValueError(f'{k}={v!r} has no meaning in axtrack_amd.render_inference (frames, APNG and MJPEG AVI only; '
                                 f'DESIGN.md section 9)')
    allowed = {'draw_grid', 'draw_scalebar', 'draw_axon_reconstructions', 'draw_true_dets', 'draw_brightened_bg',
               'axon_subset', 'description', 'annotate', 'draw_target_paths'}
    bad = set(kwargs) - allowed
    if bad:
        raise TypeError(f'render_inference got unexpected keywords {sorted(bad)}')
    dest_dir = dest_dir if dest_dir is not None else axon_dets.dir
    if not dest_dir:
        raise ValueError('render_inference needs dest_dir (the detections have no directory)')
    os.makedirs(dest_dir, exist_ok=True)
    T = len(axon_dets)
    ds = axon_dets.dataset
    tmin, tmax = (0, T) if t_y_x_slice[0] is None else tuple(t_y_x_slice[0])
    if not 0 <= tmin <= tmax <= T:
        raise ValueError(f't_y_x_slice {t_y_x_slice} lies outside the timelapse [0, {T})')
    ymin, ymax = (0, ds.sizey) if t_y_x_slice[1] is None else tuple(t_y_x_slice[1])
    xmin, xmax = (0, ds.sizex) if t_y_x_slice[2] is None else tuple(t_y_x_slice[2])
    per = max(1, _FRAME_BYTES_PER_CHUNK // max(1, 3 * (ymax - ymin) * (xmax - xmin)))
    name = axon_dets.name
    if video:
        from .jpeg import jpeg_encode, write_mjpeg_avi
        jpegs = []
        for a in range(tmin, tmax, per):
            jpegs += jpeg_encode(render_frames(axon_dets, which_dets, t_y_x_slice, _frames=np.arange(a, min(a + per, tmax)), **kwargs),
                                 quality)
        return [write_mjpeg_avi(f'{dest_dir}/{name}_dets{anim_fname_postfix}.avi', jpegs, ymax - ymin, xmax - xmin, fps)]
    paths, payloads = [], []
    with ThreadPoolExecutor(max_workers=_POOL_THREADS) as pool:
        for a in range(tmin, tmax, per):
            ts = np.arange(a, min(a + per, tmax))
            rgb = render_frames(axon_dets, which_dets, t_y_x_slice, _frames=ts, **kwargs).cpu().numpy()
            payloads += list(pool.map(_idat_payload, rgb))
        H, W = (ymax - ymin), (xmax - xmin)
        if animated:
            path = f'{dest_dir}/{name}_dets{anim_fname_postfix}.png'
            with open(path, 'wb') as f:
                f.write(apng_bytes(payloads, H, W, fps))
            return [path]

        def write(k):
            path = f'{dest_dir}/{name}_frame{tmin + k:03}of{T:03}.png'
            with open(path, 'wb') as f:
                f.write(_PNG_SIG + _ihdr(H, W) + _chunk(b'IDAT', payloads[k]) + _chunk(b'IEND', b''))
            return path
        paths = list(pool.map(write, range(len(payloads))))
    return paths
