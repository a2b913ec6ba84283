"""Sizes and timing of the Deflate TIFF writer (DESIGN.md 6.8h "TIFF output"), by the method of
profiles/tiff_inflate_timing.py: 2 warm-up runs, then the median of 7 (min and max kept), a host clock around work that ends
in a device synchronise, device events for a launch alone; where two routes are compared their runs alternate.

  sizes              bytes of the device streams (csrc/tiff_deflate.hip) against zlib level 1 and level 6, per frame type of
                     tests/tiff_deflate_cases.py at 512 x 512 with the default strips (16 of 32 rows), predictor 1 and 2.
                     A property of the parse, so --sizes-only produces it without a GPU, with the host program.
  launch_vs_strips   the deflate launch alone on 1 .. 4096 strips of 32 x 512, sparse and camera frames.
  write_tiff         a 256 x 512 x 512 device stack (axtrack_amd.synth, raw counts) written on the device route against
                     the host route at zlib level 1 and 6 in the pool of 16 threads, its D2H of the raw stack included.
  small_packs        both routes for 1 .. 256 strips of 32 x 512: strips on the device -> compressed bytes on the host.
                     This is where tiff.deflate_on_device takes its threshold from.

    python profiles/tiff_deflate_timing.py [--out FILE] [--frames 256] [--sizes-only]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

import tiff_deflate_cases as dc                                # noqa: E402

H = W = 512
WARMUP, REPEATS = 2, 7
KINDS = ('sparse', 'blobs', 'zeros', 'camera', 'noise')


def sizes_on_the_host():
    """The table of sizes from the host program (the device's streams byte for byte: tests/test_tiff_deflate_gpu.py)."""
    tmp = tempfile.mkdtemp()
    exe = dc.build_host_program(tmp, sanitize=False)
    table = {}
    for predictor in (1, 2):
        for kind in KINDS:
            frame = dc.FRAME_KINDS[kind]((H, W), 0)
            strips = [dc.DeflateCase(f'{kind}{k}', np.ascontiguousarray(frame[r:r + 32]), predictor) for k, r in enumerate(range(0, H, 32))]
            res, streams = dc.run_host_program(exe, strips, tmp, f'{kind}{predictor}')
            assert res.returncode == 0
            raw = [dc.stored_bytes(s.a, predictor) for s in strips]
            assert all(zlib.decompress(s) == r for (_, s, _), r in zip(streams, raw))
            ours, z1, z6 = (sum(len(s) for _, s, _ in streams), sum(len(zlib.compress(r, 1)) for r in raw),
                            sum(len(zlib.compress(r, 6)) for r in raw))
            table[f'{kind}_predictor{predictor}'] = {'raw_bytes': H * W * 2, 'device_stream_bytes': ours, 'zlib_level1_bytes': z1,
                                                     'zlib_level6_bytes': z6, 'against_level1': round(ours / z1, 3),
                                                     'against_level6': round(ours / z6, 3)}
    return table


def alternating(fns):
    """{name: fn} run in turn, WARMUP + REPEATS rounds -> {name: dict(median_ms, min_ms, max_ms)}."""
    import torch
    ms = {k: [] for k in fns}
    for i in range(WARMUP + REPEATS):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms[k].append((time.perf_counter() - t) * 1e3)
    return {k: {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tiff_deflate_timing.json'))
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--sizes-only', action='store_true', help='the table of sizes from the host program; needs no GPU')
    args = ap.parse_args()
    res = {'sizes': sizes_on_the_host()}
    print(json.dumps(res['sizes']), flush=True)
    if args.sizes_only:
        if os.path.exists(args.out):                                      # keep the measured parts of an earlier run
            old = json.load(open(args.out))
            old['sizes'] = res['sizes']
            res = old
        json.dump(res, open(args.out, 'w'), indent=1)
        return
    import torch
    import tiff_decode_timing as base
    from axtrack_amd import hotpath, tiff
    assert torch.cuda.is_available(), 'this measures the GPU path: no device, no numbers'
    res.update({'warmup': WARMUP, 'repeats': REPEATS, 'device': torch.cuda.get_device_name(0)})
    seg_dtype = tiff.TIFF_SEGMENT_DTYPE

    def strips_of(kind, n):
        """n strips of 32 x 512 on the device, every one a different frame's worth of `kind`."""
        a = np.concatenate([dc.FRAME_KINDS[kind]((32 * min(n, 64), W), s) for s in range(-(-n // 64))])[:32 * n]
        segs = np.zeros(n, seg_dtype)
        segs['rows'], segs['dst_offset'] = 32, np.arange(n) * 32 * W
        return torch.from_numpy(a.view(np.int16)).cuda(), a, segs

    # ---- the launch alone against the number of strips
    res['launch_vs_strips'] = {}
    for kind in ('sparse', 'camera'):
        res['launch_vs_strips'][kind] = {}
        for n in (1, 4, 16, 64, 256, 1024, 4096):
            d, a, segs = strips_of(kind, n)
            cap = dc.bound(32 * W * 2)
            segs['src_bytes'], segs['src_offset'] = cap, np.arange(n) * cap
            slots = torch.empty(n * cap, dtype=torch.uint8, device='cuda')
            nbytes, status = torch.zeros(n, dtype=torch.int64, device='cuda'), torch.zeros(n, dtype=torch.int32, device='cuda')
            d_segs = hotpath.tiff_deflate_launch(d, segs, W, 1, slots, nbytes, status)
            torch.cuda.synchronize()
            assert not status.any()
            ms = []
            for i in range(WARMUP + REPEATS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hotpath.tiff_deflate_launch(d, d_segs, W, 1, slots, nbytes, status)
                e1.record()
                e1.synchronize()
                if i >= WARMUP:
                    ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            r = {'strips': n, 'raw_bytes': n * 32 * W * 2, 'stream_bytes': int(nbytes.sum()), 'median_ms': round(med, 3),
                 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3), 'input_GB_per_s': round(n * 32 * W * 2 / med / 1e6, 3)}
            res['launch_vs_strips'][kind][str(n)] = r
            print(kind, json.dumps(r), flush=True)

    # ---- small packs: strips on the device -> their streams on the host, both routes
    res['small_packs'] = {}
    row0, rows = np.zeros(1, np.int64), np.full(1, 32, np.int64)
    for kind in ('sparse', 'camera'):
        res['small_packs'][kind] = {}
        for n in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            d, a, segs = strips_of(kind, n)

            def host_route(level):
                raw = d.cpu().numpy().view(np.uint16).reshape(n, 32, W)
                return tiff._deflate_on_host(raw, row0, rows, 1, level)
            got = hotpath.tiff_deflate_strips(d, segs, W, 1)
            assert zlib.decompress(got[0][int(got[1][0]):int(got[1][1])].tobytes()) == a[:32].tobytes()
            r = alternating({'device': lambda: hotpath.tiff_deflate_strips(d, segs, W, 1), 'host_level1': lambda: host_route(1),
                             'host_level6': lambda: host_route(6)})
            r['strips'] = n
            r['device_faster_than_level1'] = r['device']['median_ms'] < r['host_level1']['median_ms']
            r['device_faster_than_level6'] = r['device']['median_ms'] < r['host_level6']['median_ms']
            res['small_packs'][kind][str(n)] = r
            print('small_packs', kind, json.dumps(r), flush=True)
    res['deflate_on_device_from'] = tiff.DEFLATE_ON_DEVICE_FROM

    # ---- write_tiff of the timelapse
    raw = base.raw_timelapse(args.frames)
    stack = torch.from_numpy(raw.view(np.int16)).cuda()
    tmp = tempfile.mkdtemp()
    paths = {k: os.path.join(tmp, f'{k}.tif') for k in ('device', 'host_level1', 'host_level6')}
    r = alternating({'device': lambda: tiff.write_tiff(paths['device'], stack, deflate='device'),
                     'host_level1': lambda: tiff.write_tiff(paths['host_level1'], stack, deflate='host', level=1),
                     'host_level6': lambda: tiff.write_tiff(paths['host_level6'], stack, deflate='host', level=6)})
    for k, p in paths.items():
        r[k]['file_bytes'] = os.path.getsize(p)
        assert np.array_equal(tiff.read_tiff(p, device='cpu'), raw), k
    r.update({'shape': list(raw.shape), 'raw_bytes': int(raw.nbytes), 'strips': tiff.tiff_info(paths['device']).n_segments})
    res['write_tiff'] = r
    print('write_tiff', json.dumps(r), flush=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
