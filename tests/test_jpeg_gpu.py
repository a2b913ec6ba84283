"""Frames JPEG-encoded on the GPU (csrc/jpeg.hip, include/axtrack_hip_jpeg.h). The encoder is integer
work, so every comparison is exact: the bytes of every case of tests/jpeg_cases.py against the per-block, per-bit
reference of tests/jpeg_reference.py, in sentinel-filled buffers; then the Python layer, and the video of a small scene
end to end, its frames decoded by Pillow."""
import io

import numpy as np
import pytest

from axtrack_amd import _lib, hotpath as hp, jpeg, render as rnd

import jpeg_cases as jc
import jpeg_reference as ref

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = 0x5A, 64
PSNR_MARGIN_DB = 0.25               # the bound of test_jpeg_cpu.py


def _case(name):
    return next(c for c in jc.cases() if c[0] == name)


def _device_frames(rgb, pad, dev):
    """The case's frames on the device, `pad` bytes of 0xA5 behind each: (the flat buffer, a [N, H, W, 3] view of it)."""
    import torch
    N, H, W, _ = rgb.shape
    stride = 3 * H * W + pad
    host = np.full((N, stride), 0xA5, np.uint8)
    host[:, :3 * H * W] = rgb.reshape(N, -1)
    flat = torch.from_numpy(host).to(dev)
    return flat, flat.as_strided((N, H, W, 3), (stride, 3 * W, 3, 1))


def _encode(name, capacity=None):
    """The case through axt_jpeg_encode_rgb8 with every buffer poisoned: (scan [N, capacity + GUARD] as the host sees it,
    counts, status, capacity). The slots are `capacity` bytes apart; GUARD sentinel bytes follow the last one."""
    import torch
    dev = torch.device('cuda', 0)
    _, rgb, quality, pad = _case(name)
    N, H, W, _ = rgb.shape
    want = [s for s, _ in jc.reference(name)]
    capacity = max(len(s) for s in want) + 13 if capacity is None else capacity
    flat, view = _device_frames(rgb, pad, dev)
    scan = torch.full((N * capacity + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    counts = torch.full((N,), -1, dtype=torch.int64, device=dev)
    status = torch.full((N,), -1, dtype=torch.int32, device=dev)
    scratch = torch.full((hp.jpeg_scratch_bytes(N, H, W),), 0xCD, dtype=torch.uint8, device=dev)
    lib = _lib.load()
    out = []
    for _ in range(2):                                      # the second run finds the first one's scratch
        rc = lib.axt_jpeg_encode_rgb8(view.data_ptr(), N, H, W, 3 * H * W + pad, quality, scan.data_ptr(), capacity,
                                      counts.data_ptr(), status.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.axt_last_error()
        torch.cuda.synchronize()
        out.append((scan.cpu().numpy().copy(), counts.cpu().numpy().copy(), status.cpu().numpy().copy()))
        assert (flat.cpu().numpy().reshape(N, -1)[:, 3 * H * W:] == 0xA5).all()
    assert all(np.array_equal(a, b) for a, b in zip(*out)), 'two runs differ'
    return out[0] + (capacity, want)


@pytest.mark.parametrize('name', jc.case_names())
def test_every_case_equals_the_reference(name):
    scan, counts, status, cap, want = _encode(name)
    assert status.tolist() == [0] * len(want)
    assert counts.tolist() == [len(s) for s in want]
    for k, s in enumerate(want):
        slot = scan[k * cap:(k + 1) * cap]
        got = slot[:len(s)].tobytes()
        if got != s:
            at = next(i for i in range(len(s)) if got[i] != s[i])
            raise AssertionError(f'{name} frame {k}: first difference at byte {at} of {len(s)}: {got[at:at + 8].hex()} vs {s[at:at + 8].hex()}')
        assert (slot[len(s):] == SENTINEL).all(), f'{name} frame {k}: bytes written beyond the frame\'s count'
    assert (scan[len(want) * cap:] == SENTINEL).all()


def test_a_slot_one_byte_short():
    want = [s for s, _ in jc.reference('three_frames_strided')]
    big = int(np.argmax([len(s) for s in want]))
    assert big == 1 and all(len(s) < len(want[1]) - 1 for k, s in enumerate(want) if k != 1)
    cap = len(want[1]) - 1
    scan, counts, status, _, _ = _encode('three_frames_strided', capacity=cap)
    assert status.tolist() == [0, 1, 0]
    assert counts.tolist() == [len(s) for s in want]       # what the frame needs
    for k in (0, 2):
        slot = scan[k * cap:(k + 1) * cap]
        assert slot[:len(want[k])].tobytes() == want[k] and (slot[len(want[k]):] == SENTINEL).all()
    assert (scan[3 * cap:] == SENTINEL).all()               # nothing behind the last slot


def test_side_stream_and_poisoned_outputs():
    """The call is asynchronous on ITS stream: the input holds a decoy until a copy enqueued on a side stream, behind a
    delay, replaces it. A kernel launched on any other stream would run during the delay and code the decoy."""
    import torch
    dev = torch.device('cuda', 0)
    name = 'scene'
    _, rgb, quality, _ = _case(name)
    N, H, W, _ = rgb.shape
    want = jc.reference(name)[0][0]
    real = torch.from_numpy(np.ascontiguousarray(rgb)).pin_memory()
    d_rgb = torch.zeros((N, H, W, 3), dtype=torch.uint8, device=dev)                  # the decoy: black
    cap = len(want) + 7
    scan = torch.full((cap,), SENTINEL, dtype=torch.uint8, device=dev)
    counts = torch.full((1,), -1, dtype=torch.int64, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    scratch = torch.full((hp.jpeg_scratch_bytes(N, H, W),), 0xFF, dtype=torch.uint8, device=dev)
    a = torch.randn((2048, 2048), device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(20):                                 # the delay: plain work of known length
            a = (a @ a) * 1e-3
        d_rgb.copy_(real, non_blocking=True)
        hp.jpeg_encode_launch(d_rgb, quality, scan.view(1, cap), counts, status, scratch)
    side.synchronize()
    assert status.item() == 0 and counts.item() == len(want)
    got = scan.cpu().numpy()
    assert got[:len(want)].tobytes() == want and (got[len(want):] == SENTINEL).all()


def test_jpeg_encode_returns_whole_files(monkeypatch):
    import torch
    dev = torch.device('cuda', 0)
    for name in ('one_pixel', 'scene', 'three_frames_strided'):
        _, rgb, quality, _ = _case(name)
        files = jpeg.jpeg_encode(torch.from_numpy(rgb).to(dev), quality)
        assert files == [ref.header(rgb.shape[1], rgb.shape[2], quality) + s + b'\xff\xd9' for s, _ in jc.reference(name)]
    _, rgb, quality, _ = _case('scene')
    assert jpeg.jpeg_encode(torch.from_numpy(rgb[0]).to(dev), quality) == [ref.encode(rgb[0], quality)]   # [H, W, 3]
    assert jpeg.jpeg_encode(torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=dev)) == []
    # the retry: noise at quality 100 in slots that start small
    capacities = []
    launch = hp.jpeg_encode_launch
    monkeypatch.setattr(hp, 'jpeg_encode_launch', lambda rgb, q, scan, *a: (capacities.append(scan.shape[1]), launch(rgb, q, scan, *a))[1])
    _, rgb, quality, _ = _case('noise_q100')
    whole = [ref.header(rgb.shape[1], rgb.shape[2], quality) + jc.reference('noise_q100')[0][0] + b'\xff\xd9']
    bound = hp.jpeg_scan_bound(rgb.shape[1], rgb.shape[2])
    assert jpeg.jpeg_encode(torch.from_numpy(rgb).to(dev), quality, _first_capacity=4096) == whole
    assert capacities == [4096, bound]
    capacities.clear()
    assert len(whole[0]) > 3 * rgb.shape[1] * rgb.shape[2]                            # noise at quality 100 outgrows its pixels:
    assert jpeg.jpeg_encode(torch.from_numpy(rgb).to(dev), quality) == whole         # the default first capacity retries too
    assert capacities == [3 * rgb.shape[1] * rgb.shape[2], bound]
    capacities.clear()
    _, rgb, quality, _ = _case('scene')
    jpeg.jpeg_encode(torch.from_numpy(rgb).to(dev), quality)                          # an image fits the first time
    assert capacities == [3 * rgb.shape[1] * rgb.shape[2]]


def test_video_of_a_small_scene_end_to_end(tmp_path):
    import axtrack_amd
    from PIL import Image
    from test_render import _ad, _two_axons, LAYERS
    ad = _ad(_two_axons(), 200, 260, pixelsize=0.62, dt=31, incubation_time=4000)
    F = len(ad)
    frames = ad.render_frames(**LAYERS).cpu().numpy()
    paths = axtrack_amd.render_inference(ad, dest_dir=str(tmp_path), video=True, fps=12.5, anim_fname_postfix='_x', **LAYERS)
    assert paths == [f'{tmp_path}/render_dets_x.avi']
    data = open(paths[0], 'rb').read()
    jpegs = jc.check_avi(data, F, 200, 260, 2, 25)
    header = jpeg.jpeg_header(200, 260, 90)
    for t, j in enumerate(jpegs):
        assert j[:len(header)] == header and j[-2:] == b'\xff\xd9'
        im = Image.open(io.BytesIO(j))
        im.load()
        assert im.size == (260, 200) and im.mode == 'RGB'
        ours = ref.psnr(np.asarray(im), frames[t])
        buf = io.BytesIO()
        Image.fromarray(frames[t]).save(buf, 'JPEG', qtables=[list(q) for q in ref.quant_tables(90)], subsampling=0, optimize=False)
        theirs = ref.psnr(np.asarray(Image.open(io.BytesIO(buf.getvalue()))), frames[t])
        print(f'frame {t}: {len(j)} bytes, {ours:.3f} dB, Pillow {theirs:.3f} dB, difference {ours - theirs:+.3f} dB')
        assert ours >= theirs - PSNR_MARGIN_DB
    # a slice and another quality; the rate of fps = 6
    paths = axtrack_amd.render_inference(ad, dest_dir=str(tmp_path), video=True, quality=50,
                                         t_y_x_slice=((1, 4), (10, 111), (20, 141)), **LAYERS)
    assert paths == [f'{tmp_path}/render_dets.avi']
    jpegs = jc.check_avi(open(paths[0], 'rb').read(), 3, 101, 121, 1, 6)
    assert all(Image.open(io.BytesIO(j)).size == (121, 101) for j in jpegs)
    # video=False: the PNG route as it was
    paths = axtrack_amd.render_inference(ad, dest_dir=str(tmp_path), **LAYERS)
    assert paths == [f'{tmp_path}/render_frame{t:03}of{F:03}.png' for t in range(F)]
    for t, p in enumerate(paths):
        assert open(p, 'rb').read() == rnd.png_bytes(frames[t])
    paths = axtrack_amd.render_inference(ad, dest_dir=str(tmp_path), animated=True, fps=4, **LAYERS)
    assert paths == [f'{tmp_path}/render_dets.png']
    assert open(paths[0], 'rb').read() == rnd.apng_bytes([rnd._idat_payload(f) for f in frames], 200, 260, 4)
