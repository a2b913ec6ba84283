"""Timing of the Deflate route of the native TIFF reader, on the timelapse and by the method of
profiles/tiff_decode_timing.py: 256 frames of 512 x 512 from axtrack_amd.synth, 2 warm-up runs, then the median of 7 (min
and max kept), a host clock around work that ends in a device synchronise, device events for a launch alone, files in the
page cache.

  read_tiff               the Deflate file (RowsPerStrip 32: 4096 strips), and the same with predictor 2, inflated on the
                          device (csrc/tiff_inflate.hip) against zlib on the host -- the second is the route the reader
                          had before, so this is the comparison with it.
  launch_vs_segments      the launch alone on strips already on the device, 64 frames as 64 / 256 / 1024 / 4096 / 16384
                          strips (the sweep tiff_decode_timing.json has for LZW).
  single_page_vs_host_zlib  one 512 x 512 page as 1, 4 and 16 strips: pack + H2D of the compressed strips + the launch, against
                          zlib.decompress of the same strips on one host core + H2D of the inflated bytes + the row launch.
  small_packs             the same comparison on packs of 1 to 64 whole-page strips and of 16 to 256 strips of 32 rows.
                          This is where tiff.inflate_on_device takes its threshold from.
  detect_dataset          Timelapse.from_tiff to the end of AxonDetections.detect_dataset(): Deflate on either route, LZW,
                          uncompressed.

Files are written by the test writer (tests/tiff_cases.py; its LZW encoder is pure Python and slow) into --cache and
reused when present; --prepare writes them and stops, which needs no GPU. Writes profiles/tiff_inflate_timing.json (or --out).

    python profiles/tiff_inflate_timing.py [--cache DIR] [--out FILE] [--frames 256] [--prepare]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

import tiff_cases as tc                                        # noqa: E402
import tiff_decode_timing as base                              # noqa: E402
import axtrack_amd                                             # noqa: E402
from axtrack_amd import hotpath, params, synth, tiff           # noqa: E402

H = W = base.H
WARMUP, REPEATS = base.WARMUP, base.REPEATS
SWEEP_RPS = (512, 128, 32, 8, 2)


def forced(route):
    """tiff.inflate_on_device pinned to one route; returns the function to restore."""
    old = tiff.inflate_on_device
    tiff.inflate_on_device = lambda n: route == 'device'
    return old


def launch_only(path, inflate=None):
    """The decode launch alone (device events) on a file's strips, already on the device."""
    info = tiff.tiff_info(path)
    T = info.shape[0]
    packer = tiff.SegmentPacker(info, inflate=inflate)
    view, host, segs, total = packer.pack(0, T)
    d_src = host.cuda()
    out = torch.empty(info.shape, dtype=torch.int16, device='cuda')
    status = torch.empty(len(segs), dtype=torch.int32, device='cuda')
    args = (W, packer.device_compression, info.predictor, info.byteorder == '>', out, status)
    d_segs = hotpath.tiff_decode_launch(d_src, segs, *args)
    torch.cuda.synchronize()
    assert not status.any()
    ms = []
    for i in range(WARMUP + REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hotpath.tiff_decode_launch(d_src, d_segs, *args)
        e1.record()
        e1.synchronize()
        if i >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return {'segments': len(segs), 'compressed_bytes': total, 'median_ms': round(statistics.median(ms), 3),
            'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3),
            'output_GB_per_s': round(out.numel() * 2 / statistics.median(ms) / 1e6, 2)}, out


def pack_routes(path, n_frames, want):
    """The first n_frames of a file as one pack: compressed strips to the device and inflated there, against zlib here
    and the inflated bytes sent; each timed from pack() to the end of the launch."""
    info = tiff.tiff_info(path)
    out = torch.empty((n_frames,) + info.shape[1:], dtype=torch.int16, device='cuda')
    n = int(np.searchsorted(info.frame, n_frames))
    status = torch.zeros(n, dtype=torch.int32, device='cuda')
    res = {'segments': n, 'frames': n_frames, 'compressed_bytes': int(info.src_bytes[:n].sum())}
    for route in ('device', 'host'):
        packer = tiff.SegmentPacker(info, inflate=route)

        def run():
            view, host, segs, total = packer.pack(0, n_frames)
            d_src = host.to('cuda', non_blocking=True)
            return hotpath.tiff_decode_launch(d_src, segs, W, packer.device_compression, info.predictor, False, out, status), d_src
        res[f'pack_h2d_launch_{route}'] = base.timed(run)
        assert not status.any() and np.array_equal(out.cpu().numpy().view(np.uint16), want[:n_frames]), route
    res['device_faster'] = res['pack_h2d_launch_device']['median_ms'] < res['pack_h2d_launch_host']['median_ms']
    return res


def single_page(path, page):
    """One page: pack_routes, zlib.decompress of its strips alone, and the launch alone."""
    info = tiff.tiff_info(path)
    res = pack_routes(path, 1, page[None])
    strips = [bytes(np.memmap(path, np.uint8, 'r')[o:o + n]) for o, n in zip(info.src_offset, info.src_bytes)]
    res['zlib_decompress_alone'] = base.timed(lambda: [zlib.decompress(s) for s in strips], sync=False)
    res['launch_alone'], _ = launch_only(path, 'device')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cache', default=os.path.join(tempfile.gettempdir(), 'axtrack_tiff_timing'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tiff_inflate_timing.json'))
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--prepare', action='store_true', help='write the files into --cache and stop')
    args = ap.parse_args()
    os.makedirs(args.cache, exist_ok=True)
    T = args.frames
    T2 = min(64, T)
    raw = base.raw_timelapse(T)
    files = {'deflate': base.cached_tiff(args.cache, f'deflate_{T}.tif', raw, rows_per_strip=32, compression=tc.ADOBE_DEFLATE),
             'deflate_predictor2': base.cached_tiff(args.cache, f'deflate_pred2_{T}.tif', raw, rows_per_strip=32,
                                                    compression=tc.ADOBE_DEFLATE, predictor=2)}
    sweep = {rps: base.cached_tiff(args.cache, f'deflate_{T2}_rps{rps}.tif', raw[:T2], rows_per_strip=rps, compression=tc.ADOBE_DEFLATE)
             for rps in SWEEP_RPS}
    pages = {rps: base.cached_tiff(args.cache, f'deflate_page_rps{rps}.tif', raw[:1], rows_per_strip=rps, compression=tc.ADOBE_DEFLATE)
             for rps in (512, 128, 32)}
    lzw = base.cached_tiff(args.cache, f'lzw_{T}.tif', raw, rows_per_strip=32, compression=tc.LZW)
    none = base.cached_tiff(args.cache, f'none_{T}.tif', raw, rows_per_strip=32, compression=tc.NONE)
    if args.prepare:
        return
    assert torch.cuda.is_available(), 'this measures the GPU path: no device, no numbers'
    res = {'shape': [T, H, W], 'raw_bytes': int(raw.nbytes), 'nonzero_fraction': round(float((raw != 0).mean()), 4),
           'warmup': WARMUP, 'repeats': REPEATS, 'device': torch.cuda.get_device_name(0), 'read_tiff': {}}

    # ---- read_tiff, device route against host route
    for name, path in files.items():
        r = {'file_bytes': os.path.getsize(path), 'segments': tiff.tiff_info(path).n_segments}
        for route in ('device', 'host'):
            old = forced(route)
            try:
                got = axtrack_amd.read_tiff(path)
                assert np.array_equal(got.cpu().numpy().view(np.uint16), raw), (name, route)
                r[f'read_tiff_{route}'] = base.timed(lambda: axtrack_amd.read_tiff(path))
            finally:
                tiff.inflate_on_device = old
        r['launch_only_device'], out = launch_only(path, 'device')
        assert np.array_equal(out.cpu().numpy().view(np.uint16), raw), name
        res['read_tiff'][name] = r
        print(name, json.dumps(r), flush=True)

    # ---- the launch alone against the number of segments (64 frames)
    res['launch_vs_segments'] = {'frames': T2, 'output_bytes': int(raw[:T2].nbytes), 'rows_per_strip': {}}
    for rps, path in sweep.items():
        r, out = launch_only(path, 'device')
        assert np.array_equal(out.cpu().numpy().view(np.uint16), raw[:T2]), rps
        res['launch_vs_segments']['rows_per_strip'][str(rps)] = r
        print('rps', rps, json.dumps(r), flush=True)

    # ---- one page as 1, 4, 16 strips: where the host's zlib and the device cross
    res['single_page_vs_host_zlib'] = {}
    for rps, path in pages.items():
        r = single_page(path, raw[0])
        res['single_page_vs_host_zlib'][str(rps)] = r
        print('page rps', rps, json.dumps(r), flush=True)

    # ---- packs of few strips, whole pages and 32 rows each: the threshold of tiff.inflate_on_device
    res['small_packs'] = {'strips_of_512_rows': {}, 'strips_of_32_rows': {}}
    for key, rps, frames in (('strips_of_512_rows', 512, (1, 4, 16, 32, 64)), ('strips_of_32_rows', 32, (1, 2, 4, 16))):
        for k in frames:
            r = pack_routes(sweep[rps], k, raw)
            res['small_packs'][key][str(r['segments'])] = r
            print(key, json.dumps(r), flush=True)
    res['inflate_on_device_from'] = tiff.INFLATE_ON_DEVICE_FROM

    # ---- from_tiff to the end of detect_dataset
    model = axtrack_amd.Detector(synth.synth_state_dict(42), max_batch=256)
    P = params.load_parameters()
    kw = dict(name='t', offset=121, clip=55, scale=params.DEPLOYED_STND_SCALER[1][0])

    def detect(path, route=None):
        def run():
            old = forced(route) if route else None
            try:
                ad = axtrack_amd.AxonDetections(model, axtrack_amd.Timelapse.from_tiff(path, **kw), P, None)
                ad.detect_dataset(cache=None)
            finally:
                if route:
                    tiff.inflate_on_device = old
            return ad
        return run
    runs = {'from_tiff_deflate_device': detect(files['deflate'], 'device'), 'from_tiff_deflate_host': detect(files['deflate'], 'host'),
            'from_tiff_lzw': detect(lzw), 'from_tiff_none': detect(none)}
    ref = runs['from_tiff_none']()._yolo
    for name, run in runs.items():
        assert torch.equal(run()._yolo, ref), name
    res['detect_dataset'] = {name: base.timed(run) for name, run in runs.items()}
    print(json.dumps(res['detect_dataset']), flush=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
