"""Rendering of tracking results (AxonDetections.render_frames, axtrack_amd.render_inference; the reference's
video_plotting.draw_all) and the PNG / APNG writer.

The oracle below is an independent numpy restatement of the drawing rules. It reads only
get_frame_dets, get_axon_reconstructions and Timelapse.frames, plus the font table (data). Layout constants restated
from DESIGN.md 6.8b: label glyphs from (x0, y0 - 8s); glyph advance 6s; header lines right-aligned to Wo - 4s, line k
at y = 4s + 9s k; scale bar rint(200 / pixelsize) x 2s at y = 4s + 9s n_lines + s, right end Wo - 4s, caption '200 um'
at the bar's y + 4s."""
import colorsys
import struct
import zlib

import numpy as np
import pytest

from axtrack_amd import synth, params
from axtrack_amd import render as rnd

TC = 2
BOX = 70


# ------------------------------------------------------------------------------------------------- stdlib PNG decoder
def _decode_png(data):
    """(frames [n, H, W, 3] u8, chunk names, acTL (n, plays) or None, delays [(num, den)])."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, names, idat, frames, actl, delays = 8, [], b'', [], None, []
    W = H = None
    cur = None
    while pos < len(data):
        n, = struct.unpack('>I', data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF
        names.append(kind.decode())
        pos += 12 + n
        if kind == b'IHDR':
            W, H, depth, ctype, comp, filt, inter = struct.unpack('>IIBBBBB', body)
            assert (depth, ctype, comp, filt, inter) == (8, 2, 0, 0, 0)
        elif kind == b'acTL':
            actl = struct.unpack('>II', body)
        elif kind == b'fcTL':
            if cur is not None:
                frames.append(cur)
            f = struct.unpack('>IIIIIHHBB', body)
            delays.append((f[5], f[6]))
            cur = b''
        elif kind == b'IDAT':
            if cur is None:
                idat += body
            else:
                cur += body
        elif kind == b'fdAT':
            cur += body[4:]
    if cur is not None:
        frames.append(cur)
    if not frames:
        frames = [idat]
    out = []
    for z in frames:
        raw = np.frombuffer(zlib.decompress(z), np.uint8).reshape(H, 1 + 3 * W)
        assert (raw[:, 0] == 0).all()
        out.append(raw[:, 1:].reshape(H, W, 3))
    return np.stack(out), names, actl, delays


# ------------------------------------------------------------------------------------------------- numpy oracle
def _palette():
    return np.array([[int(round(c * 255)) for c in colorsys.hsv_to_rgb(k / 20, 1, 1)] for k in range(20)], np.int64)


def _blend(a, C, c):
    return (a * C + (256 - a) * c + 128) >> 8


def _box_blur(a, axis):
    n = a.shape[axis]
    pad = [(0, 0), (0, 0)]
    pad[axis] = (4, 4)
    p = np.pad(a, pad, mode='edge')
    s = sum(np.take(p, np.arange(k, k + n), axis=axis) for k in range(9))
    return (s + 4) // 9


def _paint(img, y0, y1, x0, x1, rgb):
    H, W = img.shape[:2]
    y0, y1, x0, x1 = max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)
    if y0 < y1 and x0 < x1:
        img[y0:y1, x0:x1] = rgb


def _text(img, text, x, y, s, rgb):
    for k, ch in enumerate(text):
        c = ord(ch)
        if not 32 <= c <= 126:
            continue
        rows = rnd.GLYPH_ROWS[c - 32]
        for gy in range(7):
            for gx in range(5):
                if (int(rows[gy]) >> (4 - gx)) & 1:
                    _paint(img, y + gy * s, y + gy * s + s, x + (6 * k + gx) * s, x + (6 * k + gx) * s + s, rgb)


def _border(b, dashed):
    u, v = np.meshgrid(np.arange(b), np.arange(b))
    on = (u == 0) | (v == 0) | (u == b - 1) | (v == b - 1)
    if dashed:
        on &= ((u + v) // 4) % 2 == 0
    return v[on], u[on]


def _rows(ad, which, t, subset):
    d = ad.get_frame_dets(which, t)
    if not len(d):
        return []
    names = list(d.index)
    n = [int(a.split('_')[-1]) for a in names] if which == 'IDed' else list(range(len(d)))
    rows = list(zip(n, d.anchor_x.to_numpy(np.int64), d.anchor_y.to_numpy(np.int64), names))
    if subset is not None:
        rows = [r for r in rows if r[3] in subset]
    return sorted(rows)


def _trails(img, rec, pal):
    """5 x 5 squares of every cell; where they overlap, the larger (frame, axon number) wins."""
    H, W = img.shape[:2]
    segs = sorted({(int(f), int(a.split('_')[-1]), a) for a, _, f in rec.columns})
    keys, xs, ys, cols = [], [], [], []
    for k, (f, n, a) in enumerate(segs):
        x, y = rec[(a, 'X', f)].dropna().astype(int).to_numpy(), rec[(a, 'Y', f)].dropna().astype(int).to_numpy()
        keys.append(np.full(len(x), k + 1)); xs.append(x); ys.append(y); cols.append(n % 20)
    if not segs:
        return
    key, x, y = np.concatenate(keys), np.concatenate(xs), np.concatenate(ys)
    canvas = np.zeros((H, W), np.int64)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            yy, xx = y + dy, x + dx
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            np.maximum.at(canvas, (yy[ok], xx[ok]), key[ok])
    on = canvas > 0
    img[on] = pal[np.array([0] + cols)[canvas[on]]]


def oracle(ad, t, which_dets='IDed', t_y_x_slice=(None, None, None), draw_grid=True, draw_scalebar=False,
           draw_axon_reconstructions=False, draw_true_dets=False, draw_brightened_bg=False, axon_subset=None,
           description='', annotate=True):
    ds = ad.dataset
    H, W, T = ds.sizey, ds.sizex, len(ad)
    (ymin, ymax), (xmin, xmax) = ((0, n) if v is None else v for v, n in zip(t_y_x_slice[1:], (H, W)))
    pal = _palette()
    v = ds.frames[t + TC].cpu().numpy()
    R8 = np.rint(np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.int64)
    img = np.zeros((H, W, 3), np.int64)
    img[..., 0] = R8
    if draw_brightened_bg:
        m = ds.mask3d[t + TC] if ds.mask3d is not None else (ds.mask2d if ds.mask2d is not None else np.ones((H, W), bool))
        M8 = np.where(m, 255, 0)
        a = np.where((R8 > 0) & (R8 <= 30), 26, 256)
        for axis in (1, 1, 1, 0, 0, 0):
            a = _box_blur(a, axis)
        img[..., 0] = _blend(a, R8, M8)
        img[..., 1] = img[..., 2] = _blend(a, 0, M8)
    if draw_grid:
        Y, X = np.mgrid[:H, :W]
        on = (X % ds.tilesize == 0) | (Y % ds.tilesize == 0)
        img[on] = _blend(38, 255, img[on])
    if draw_axon_reconstructions:
        _trails(img, ad.get_axon_reconstructions(t=t, include_history=True, axon_name=axon_subset), pal)
    if draw_true_dets:
        flag = np.zeros((H, W), bool)
        for _, x, y, _ in _rows(ad, 'groundtruth', t, None):
            vv, uu = _border(BOX, False)
            yy, xx = vv + y - BOX // 2, uu + x - BOX // 2
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            flag[yy[ok], xx[ok]] = True
        img[flag] = _blend(154, 255, img[flag])
    rows = _rows(ad, which_dets, t, axon_subset)
    s = max(1, min(H, W) // 512)
    for n, x, y, _ in rows:
        vv, uu = _border(BOX, True)
        yy, xx = vv + y - BOX // 2, uu + x - BOX // 2
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        img[yy[ok], xx[ok]] = pal[n % 20]
    if annotate:
        for n, x, y, _ in rows:
            _text(img, f'Ax{n:03}', x - BOX // 2, y - BOX // 2 - 8 * s, s, pal[n % 20])
    out = img[ymin:ymax, xmin:xmax].copy()
    Wo = xmax - xmin
    grey = np.array([107, 107, 107])
    lines = []
    if annotate:
        lines = ([description] if description else []) + [f'frame {t:03}/{T:03}']
        if ds.dt and ds.incubation_time:
            mins = ds.incubation_time + ds.dt * t
            lines.append(f'DIV {int(mins // 1440)} days - {int((mins % 1440) // 60)} hours')
        for k, line in enumerate(lines):
            _text(out, line, Wo - 4 * s - (6 * s * len(line) - s), 4 * s + 9 * s * k, s, grey)
    if draw_scalebar:
        L = int(np.rint(200 / ds.pixelsize))
        yb = 4 * s + 9 * s * len(lines) + s
        _paint(out, yb, yb + 2 * s, Wo - 4 * s - L, Wo - 4 * s, grey)
        _text(out, '200 um', Wo - 4 * s - (6 * s * 6 - s), yb + 4 * s, s, grey)
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------------------------- CPU
def test_png_and_apng_round_trip_exact_bytes():
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (3, 17, 23, 3), dtype=np.uint8)
    dec, names, actl, _ = _decode_png(rnd.png_bytes(frames[0]))
    assert names == ['IHDR', 'IDAT', 'IEND'] and actl is None and np.array_equal(dec[0], frames[0])
    data = rnd.apng_bytes([rnd._idat_payload(f) for f in frames], 17, 23, fps=6)
    dec, names, actl, delays = _decode_png(data)
    assert actl == (3, 0)                                    # three frames, looping forever
    assert names == ['IHDR', 'acTL', 'fcTL', 'IDAT', 'fcTL', 'fdAT', 'fcTL', 'fdAT', 'IEND']
    assert delays == [(1, 6)] * 3
    assert np.array_equal(dec, frames)
    assert rnd._delay(2.5) == (2, 5)


def test_png_readable_by_pil():
    Image = pytest.importorskip('PIL.Image')
    import io
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
    im = Image.open(io.BytesIO(rnd.png_bytes(frames[0])))
    assert np.array_equal(np.asarray(im.convert('RGB')), frames[0])
    im = Image.open(io.BytesIO(rnd.apng_bytes([rnd._idat_payload(f) for f in frames], 9, 11, fps=4)))
    assert getattr(im, 'n_frames', 1) == 2
    for k in range(2):
        im.seek(k)
        assert np.array_equal(np.asarray(im.convert('RGB')), frames[k])


def test_palette_is_twenty_hsv_hues():
    assert np.array_equal(rnd.PALETTE.astype(np.int64), _palette())
    assert rnd.PALETTE.shape == (20, 3) and tuple(rnd.PALETTE[0]) == (255, 0, 0)


def test_font_table():
    g = rnd.GLYPH_ROWS
    assert g.shape == (95, 7)                                # printable ASCII 32..126
    assert (g < 32).all()                                    # at most 5 bits wide
    assert not g[0].any() and all(g[k].any() for k in range(1, 95))
    digits = {g[ord(c) - 32].tobytes() for c in '0123456789'}
    assert len(digits) == 10
    assert rnd.label_text(7) == 'Ax007' and rnd.label_text(1234) == 'Ax1234'
    assert rnd.font_scale(512, 512) == 1 and rnd.font_scale(1024, 2048) == 2 and rnd.font_scale(100, 100) == 1


def test_oracle_hand_checks():
    vv, uu = _border(8, True)
    drawn = set(zip(uu.tolist(), vv.tolist()))
    # perimeter 4b - 4 = 28 pixels, dashed: ((u + v) // 4) even
    assert len(_border(8, False)[0]) == 28
    assert drawn == {(u, v) for u in range(8) for v in range(8) if (u in (0, 7) or v in (0, 7)) and ((u + v) // 4) % 2 == 0}
    assert (0, 0) in drawn and (3, 0) in drawn and (4, 0) not in drawn and (7, 1) in drawn
    a = np.full((13, 9), 26)
    for axis in (1, 1, 1, 0, 0, 0):
        a = _box_blur(a, axis)
    assert (a == 26).all()                                   # the blur of a constant map is that constant
    assert _blend(256, 200, 7) == 200 and _blend(0, 200, 7) == 7 and _blend(38, 255, 0) == 38
    assert rnd.header_lines('', 3, 10) == ['frame 003/010']
    assert rnd.header_lines('x', 2, 10, 30, 1440 + 90)[2] == 'DIV 1 days - 2 hours'
    assert rnd.scalebar_px(0.62) == 323


def test_unsupported_keywords_raise_before_any_work():
    import axtrack_amd
    with pytest.raises(ValueError, match='dpi'):
        axtrack_amd.render_inference(None, dpi=100)
    with pytest.raises(ValueError, match='show'):
        axtrack_amd.render_inference(None, show=True)
    with pytest.raises(ValueError, match='draw_trg_paths'):
        axtrack_amd.render_inference(None, draw_trg_paths=[1])
    assert 'render_inference' in axtrack_amd.__all__


# ------------------------------------------------------------------------------------------------- GPU
def _ad(d, H, W, frames=None, mask=None, pixelsize=None, dt=None, incubation_time=None, seed=1):
    import torch
    import axtrack_amd
    dev = torch.device('cuda', 0)
    F = len(d['count'])
    if frames is None:
        frames = synth.synth_frames(F + 2 * TC, H, W, seed=seed)
    tl = axtrack_amd.Timelapse(frames, name='render', mask=mask, device=dev, pixelsize=pixelsize, dt=dt,
                               incubation_time=incubation_time)
    P = params.load_parameters()
    P['MCF_MAX_FLOW'] = 100000
    P['MCF_MIN_FLOW'] = 1
    ad = axtrack_amd.AxonDetections(None, tl, P, None)
    ad.set_detections(*(torch.from_numpy(d[k]).to(dev) for k in ('conf', 'x', 'y', 'count')))
    ad.assign_ids()
    return ad


def _two_axons(F=6):
    conf = np.zeros((F, 4), np.float32); x = np.zeros((F, 4), np.int32); y = np.zeros((F, 4), np.int32)
    count = np.full(F, 2, np.int32)
    for t in range(F):
        conf[t, :2] = (0.95, 0.9)
        x[t, :2] = (60 + 6 * t, 150 + 4 * t)                 # the boxes overlap
        y[t, :2] = (80 + 3 * t, 100 - 5 * t)
    return dict(conf=conf, x=x, y=y, count=count)


def _check(ad, frames, **kw):
    got = ad.render_frames(**kw).cpu().numpy()
    tmin = kw.get('t_y_x_slice', (None,))[0]
    t0 = 0 if tmin is None else tmin[0]
    for t in frames:
        exp = oracle(ad, t, **kw)
        g = got[t - t0]
        assert g.shape == exp.shape
        bad = np.argwhere((g != exp).any(-1))
        assert len(bad) == 0, (f'frame {t}: {len(bad)} pixels differ, first at {bad[:3].tolist()}: '
                               f'{g[tuple(bad[0])]} vs {exp[tuple(bad[0])]}')
    return got


LAYERS = dict(draw_grid=True, draw_scalebar=True, draw_axon_reconstructions=True, draw_brightened_bg=True, annotate=True,
              description='two axons')


@pytest.mark.gpu
def test_two_axon_scene_each_layer_alone_and_all():
    ad = _ad(_two_axons(), 200, 260, pixelsize=0.62, dt=31, incubation_time=4000)
    assert ad.n_ids == 2
    F = len(ad)
    base = dict(draw_grid=False, annotate=False)
    got = _check(ad, range(F), **base)
    assert got[..., 0].any() and (got[..., 1] == got[..., 2]).mean() > 0.9     # mostly the red background
    for layer in ('draw_grid', 'draw_scalebar', 'draw_axon_reconstructions', 'draw_brightened_bg', 'annotate'):
        _check(ad, range(F), **dict(base, **{layer: True}))
    _check(ad, range(F), **LAYERS)


@pytest.mark.gpu
def test_config3_scene_end_to_end_sampled_frames():
    import torch
    import axtrack_amd
    sd = synth.synth_state_dict(42)
    frames = synth.synth_frames(256 + 2 * TC, 512, 512, seed=3)
    model = axtrack_amd.Detector(sd, max_batch=64)
    P = params.load_parameters()
    P['MCF_MIN_FLOW'] = 1
    tl = axtrack_amd.Timelapse(frames, name='c3', pixelsize=0.62, dt=31, incubation_time=3000)
    ad = axtrack_amd.AxonDetections(model, tl, P, None)
    ad.detect_dataset()
    ad.assign_ids()
    cnt, _, x, y = ad._host_dets()
    ad.set_groundtruth([(x[t, :cnt[t]] + 3, y[t, :cnt[t]] - 2) for t in range(len(ad))])
    kw = dict(LAYERS, draw_true_dets=True, description='config 3')
    got = ad.render_frames(**kw).cpu().numpy()
    assert got.shape == (256, 512, 512, 3)
    for t in (0, 1, 37, 100, 128, 201, 254, 255):
        assert np.array_equal(got[t], oracle(ad, t, **kw)), f'frame {t}'
    again = ad.render_frames(**kw).cpu().numpy()
    assert np.array_equal(got, again)
    del again
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_time_varying_mask_brightening_uses_each_frames_mask():
    F, H, W = 6, 160, 200
    d = synth.synth_detections(F, H, W, n_alive=4, seed=2, min_dist=30)
    m = np.stack([synth.corridor_mask(H, W, width=20 + 4 * k, pitch=64) for k in range(F + 2 * TC)])
    ad = _ad(d, H, W, mask=m)
    assert ad.dataset.mask3d is not None
    got = _check(ad, range(F), draw_brightened_bg=True, draw_grid=False, annotate=False)
    assert not np.array_equal(got[0], got[3])


@pytest.mark.gpu
def test_slice_is_a_crop_of_the_full_render():
    d = synth.synth_detections(12, 300, 420, n_alive=8, seed=4)
    ad = _ad(d, 300, 420)
    kw = dict(draw_grid=True, draw_axon_reconstructions=True, draw_brightened_bg=True, annotate=False)
    full = ad.render_frames(**kw).cpu().numpy()
    sl = ((3, 9), (37, 251), (70, 333))
    part = _check(ad, range(3, 9), t_y_x_slice=sl, **kw)
    assert part.shape == (6, 214, 263, 3)
    assert np.array_equal(part, full[3:9, 37:251, 70:333])


@pytest.mark.gpu
def test_other_selections_true_dets_and_subset():
    d = synth.synth_detections(8, 256, 300, n_alive=10, seed=5)
    ad = _ad(d, 256, 300)
    cnt, _, x, y = ad._host_dets()
    ad.set_groundtruth([(x[t, :cnt[t]], y[t, :cnt[t]] + 5, np.arange(cnt[t]) + 100) for t in range(len(ad))])
    for which in ('confident', 'all', 'groundtruth'):
        _check(ad, range(len(ad)), which_dets=which)
    _check(ad, range(len(ad)), draw_true_dets=True)
    names = list(ad.IDed_dets_all.index[::3])
    got = _check(ad, range(len(ad)), axon_subset=names, draw_axon_reconstructions=True)
    full = ad.render_frames(draw_axon_reconstructions=True).cpu().numpy()
    assert not np.array_equal(got, full)


@pytest.mark.gpu
def test_host_resident_timelapse_renders_the_same_bytes():
    import torch
    import axtrack_amd
    from axtrack_amd.timelapse import preprocess
    F, H, W = 10, 256, 256
    raw = (np.random.default_rng(3).integers(0, 4000, (F + 2 * TC, H, W))).astype(np.uint16)
    d = synth.synth_detections(F, H, W, n_alive=5, seed=6)
    P = params.load_parameters()
    P['MCF_MIN_FLOW'] = 1
    dev = torch.device('cuda', 0)
    out = []
    for host in (False, True):
        tl = axtrack_amd.Timelapse.from_host_u16(raw, name='h') if host else axtrack_amd.Timelapse(preprocess(raw), name='r')
        ad = axtrack_amd.AxonDetections(None, tl, P, None)
        ad.set_detections(*(torch.from_numpy(d[k]).to(dev) for k in ('conf', 'x', 'y', 'count')))
        ad.assign_ids()
        out.append(ad.render_frames(draw_brightened_bg=True).cpu().numpy())
    assert np.array_equal(out[0], out[1])


@pytest.mark.gpu
def test_render_inference_files_and_apng(tmp_path):
    import axtrack_amd
    d = synth.synth_detections(7, 128, 160, n_alive=4, seed=7, min_dist=30)
    ad = _ad(d, 128, 160)
    paths = axtrack_amd.render_inference(ad, dest_dir=str(tmp_path), draw_axon_reconstructions=True)
    assert [p.split('/')[-1] for p in paths] == [f'render_frame{t:03}of007.png' for t in range(7)]
    assert len(list(tmp_path.glob('*.png'))) == 7
    ref = ad.render_frames(draw_axon_reconstructions=True).cpu().numpy()
    for t, p in enumerate(paths):
        with open(p, 'rb') as f:
            assert np.array_equal(_decode_png(f.read())[0][0], ref[t])
    paths = axtrack_amd.render_inference(ad, dest_dir=str(tmp_path), animated=True, fps=4, anim_fname_postfix='_x',
                                         draw_axon_reconstructions=True, t_y_x_slice=((2, 6), None, None))
    assert paths == [f'{tmp_path}/render_dets_x.png']
    with open(paths[0], 'rb') as f:
        dec, names, actl, delays = _decode_png(f.read())
    assert actl == (4, 0) and delays == [(1, 4)] * 4
    assert np.array_equal(dec, ref[2:6])


@pytest.mark.gpu
def test_config4_share_chunked_sampled_frames():
    import torch
    H = W = 1024
    F = 128
    d = synth.synth_detections(F, H, W, n_alive=120, seed=0)
    ad = _ad(d, H, W, mask=synth.corridor_mask(H, W), pixelsize=0.62, seed=2)
    kw = dict(LAYERS, description='config 4 share')
    got = ad.render_frames(**kw)
    assert got.shape == (F, H, W, 3)
    for t in (0, 127):
        assert np.array_equal(got[t].cpu().numpy(), oracle(ad, t, **kw)), f'frame {t}'
    del got
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_error_cases():
    import torch
    import axtrack_amd
    ad = _ad(_two_axons(), 200, 260)
    with pytest.raises(ValueError, match='which_dets'):
        ad.render_frames('FP_FN')
    with pytest.raises(ValueError, match='outside'):
        ad.render_frames(t_y_x_slice=(None, (0, 300), None))
    with pytest.raises(ValueError, match='outside'):
        ad.render_frames(t_y_x_slice=((2, 9), None, None))
    with pytest.raises(ValueError, match='pixelsize'):
        ad.render_frames(draw_scalebar=True)
    with pytest.raises(ValueError, match='set_groundtruth'):
        ad.render_frames(draw_true_dets=True)
    with pytest.raises(ValueError, match='IDed'):
        ad.render_frames('all', draw_axon_reconstructions=True)
    # recon_timing.py's stand-in: a 5-frame timelapse under detections of 6 frames
    short = axtrack_amd.AxonDetections(None, axtrack_amd.Timelapse(torch.zeros((5, 200, 260))), ad.P, None)
    short.set_detections(ad.d_conf, ad.d_x, ad.d_y, ad.d_count)
    short.assign_ids()
    with pytest.raises(ValueError, match='detection frames'):
        short.render_frames()
    ad._shard = (0, 3, None)
    with pytest.raises(NotImplementedError, match='single process'):
        ad.render_frames()
    with pytest.raises(NotImplementedError, match='out of scope'):
        axtrack_amd.visualize_inference(ad)
