"""The inputs of the JPEG tests (test_jpeg_cpu.py, test_jpeg_gpu.py): for every route of csrc/jpeg.hip the smallest input
that reaches it, and the fact that proves it does, asserted on the reference's stream (jpeg_reference.py). The launch
constants of the kernels are restated here; test_jpeg_cpu.py checks them against the source.

A case is (name, rgb uint8 [N, H, W, 3], quality, stride_pad): stride_pad bytes of sentinel between the frames."""
import functools
import struct

import numpy as np

import jpeg_reference as ref

THREADS = 256                      # kJpegThreads
MCUS_PER_THREAD = 1                # kJpegMcusPerThread
STUFF_BYTES_PER_THREAD = 4         # kJpegStuffBytesPerThread
STUFF_CHUNK = THREADS * STUFF_BYTES_PER_THREAD
MCUS_PER_STEP = THREADS * MCUS_PER_THREAD
LDS_BYTES = 160 * 1024             # a CU's whole LDS on gfx950: no staging buffer can be larger
NOISE_SEED, PAD_SEED = 1, 1
NOISE_MCUS = 701                   # x 262 bytes or so of noise at quality 100: a row beyond LDS_BYTES


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _smooth(H, W, seed):
    """A few low-frequency waves per channel plus a little noise: compresses like an image, every block differs."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    out = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(3):
            fy, fx, ph = rng.uniform(0.01, 0.15), rng.uniform(0.01, 0.15), rng.uniform(0, 6.28)
            out[..., c] += 40 * np.sin(fy * y + fx * x + ph)
    return np.clip(out + 128 + rng.normal(0, 3, out.shape), 0, 255).astype(np.uint8)


def scene(H=64, W=96, seed=5):
    """What render.hip draws, in small: a dim red background with structure, 1-px coloured dashed boxes, 5 x 7 glyphs."""
    rng = np.random.default_rng(seed)
    img = np.zeros((H, W, 3), np.uint8)
    y, x = np.mgrid[:H, :W]
    img[..., 0] = np.clip(30 + 25 * np.sin(x / 9.0) * np.cos(y / 7.0) + rng.normal(0, 4, (H, W)), 0, 255)
    for k, (y0, x0) in enumerate(((8, 10), (30, 50), (20, 28))):
        col = [(255, 0, 0), (0, 255, 77), (51, 0, 255)][k]
        for d in range(0, 21):
            if d // 3 % 2 == 0:
                img[y0, x0 + d] = img[y0 + 20, x0 + d] = img[y0 + d, x0] = img[y0 + d, x0 + 20] = col
        for gx in range(5):
            for gy in range(7):
                if (gx * 7 + gy + k) % 3:
                    img[y0 - 8 + gy, x0 + gx] = col
    img[4:11:2, W - 40:W - 4:2] = (107, 107, 107)
    return img


def _single_coefficient_block():
    """One block that holds (almost) only the highest frequency: 62 zeros before coefficient 63."""
    k = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    return np.clip(128 + 100 * np.outer(k, k), 0, 255).astype(np.uint8)[..., None].repeat(3, -1)


def _checker():
    img = np.zeros((8, 32, 3), np.uint8)
    img[:, 8:16] = 255                                                   # DC from -1024 to +1016
    y, x = np.mgrid[:8, :8]
    img[:, 16:24] = (255 * ((x + y) & 1))[..., None]
    img[:, 24:32] = (255 * ((x + y + 1) & 1))[..., None]
    return img


@functools.lru_cache(None)
def cases():
    three = np.stack([_smooth(10, 13, 3), _noise((10, 13, 3), 2), np.zeros((10, 13, 3), np.uint8)])
    wide = 8 * (MCUS_PER_STEP + 1)
    return [
        ('one_pixel', _noise((1, 1, 1, 3), 7), 90, 0),
        ('one_block', _smooth(8, 8, 8)[None], 90, 0),
        ('replicate_7x9', _smooth(7, 9, 9)[None], 90, 0),
        ('dc_prediction_8x16', (_smooth(8, 16, 10) // 4 + 180)[None], 90, 0),
        ('dc_reset_16x8', (_smooth(16, 8, 11) // 4 + 180)[None], 90, 0),
        ('nine_rows_72x8', _smooth(72, 8, 12)[None], 90, 0),
        ('ten_rows_80x8', _smooth(80, 8, 13)[None], 90, 0),
        ('strided_loop', _smooth(8, wide, 14)[None], 75, 0),
        ('black', np.zeros((1, 16, 24, 3), np.uint8), 90, 0),
        ('zrl', _single_coefficient_block()[None], 90, 0),
        ('checker_q100', _checker()[None], 100, 0),
        ('noise_q100', _noise((24, 8 * NOISE_MCUS, 3), NOISE_SEED)[None], 100, 0),
        ('pad_bits', _noise((1, 64, 8, 3), PAD_SEED), 50, 0),
        ('scene', scene()[None], 90, 0),
        ('three_frames_strided', three, 90, 37),
        ('low_quality', _smooth(24, 40, 15)[None], 1, 0),
    ]


@functools.lru_cache(None)
def reference(name):
    """[(scan segment, facts)] per frame of the case."""
    _, rgb, quality, _ = next(c for c in cases() if c[0] == name)
    return [ref.encode_scan(f, quality) for f in rgb]


def case_names():
    return [c[0] for c in cases()]


def check_facts():
    """Every case reaches the route it is here for: asserted on the reference's stream."""
    f = lambda name, k=0: reference(name)[k][1]
    assert len(f('one_pixel')['row_bits']) == 1 and len(f('one_block')['row_bits']) == 1
    assert len(f('one_pixel')['dc_diffs']) == 3
    assert len(f('dc_prediction_8x16')['row_bits']) == 1 and len(f('dc_prediction_8x16')['dc_diffs']) == 6
    # (both images are bright: a block's luminance DC is above 100. Predicted from its left neighbour it leaves a small
    # difference; the first block of the second row is predicted from 0 again)
    d = f('dc_prediction_8x16')['dc_diffs']
    assert d[0] > 100 and abs(d[3]) < 30
    d = f('dc_reset_16x8')['dc_diffs']
    assert len(f('dc_reset_16x8')['row_bits']) == 2 and d[0] > 100 and d[3] > 100
    assert f('nine_rows_72x8')['markers'] == [0xD0 + k for k in range(8)]              # RST0..RST7: all eight
    assert f('ten_rows_80x8')['markers'] == [0xD0 + k for k in range(8)] + [0xD0]      # and the wrap to RST0
    assert cases()[7][1].shape[2] == 8 * (MCUS_PER_STEP + 1)
    assert f('black')['eob_only'] == 6 * 3 and set(f('black')['dc_diffs']) == {-341, 0}        # -1024 / 3, once
    assert f('zrl')['zrl'] >= 3
    assert f('checker_q100')['dc_cat'] == 11 and f('checker_q100')['ac_cat'] == 10
    n = f('noise_q100')
    assert NOISE_MCUS > 2 * MCUS_PER_STEP and NOISE_MCUS % MCUS_PER_STEP
    assert all((b + 7) // 8 > LDS_BYTES for b in n['row_bits'])                          # a row no LDS could stage
    assert sum(len(r) for r in n['ff_at']) > 100
    # a 0xFF as the last byte of a thread's 4 and as the last byte of a step's chunk: its 0x00 lands in the next one's range
    assert any(i % STUFF_BYTES_PER_THREAD == STUFF_BYTES_PER_THREAD - 1 for r in n['ff_at'] for i in r)
    assert any(i % STUFF_CHUNK == STUFF_CHUNK - 1 for r in n['ff_at'] for i in r)
    assert any(i % STUFF_CHUNK == 0 for r in n['ff_at'] for i in r)
    pads = {-b % 8 for b in f('pad_bits')['row_bits']}
    assert 0 in pads and len(pads - {0}) >= 3                                           # a row that ends on a byte, rows that do not
    assert cases()[14][1].shape[0] == 3 and cases()[14][3] > 0


def write_case_file(path):
    """For tests/jpeg_encode_host.cpp: int32 n_cases; per case int32 n_frames, H, W, quality, then per frame the 3 H W
    pixel bytes, int64 the scan segment's length, and its bytes."""
    with open(path, 'wb') as f:
        f.write(struct.pack('<i', len(cases())))
        for name, rgb, quality, _ in cases():
            N, H, W, _ = rgb.shape
            f.write(struct.pack('<4i', N, H, W, quality))
            for k in range(N):
                scan = reference(name)[k][0]
                f.write(np.ascontiguousarray(rgb[k]).tobytes() + struct.pack('<q', len(scan)) + scan)


# ------------------------------------------------------------------------------------------------ a RIFF / AVI parser
def parse_riff(data):
    """A RIFF file as nested lists: ('RIFF' or 'LIST', kind, [children]) and (fourcc, offset of the chunk header, payload).
    Asserts what the format demands: sizes that add up, even padding."""
    def walk(a, b):
        out = []
        while a < b:
            assert b - a >= 8, 'a chunk header is cut'
            cc, n = data[a:a + 4], struct.unpack('<I', data[a + 4:a + 8])[0]
            assert a + 8 + n <= b, f'chunk {cc} at {a} overruns its parent'
            if cc in (b'RIFF', b'LIST'):
                out.append((cc.decode(), data[a + 8:a + 12].decode(), walk(a + 12, a + 8 + n), a))
            else:
                out.append((cc.decode(), a, data[a + 8:a + 8 + n]))
                if n & 1:
                    assert data[a + 8 + n] == 0, 'the pad byte'
            a += 8 + n + (n & 1)
        assert a == b, 'children do not fill their parent'
        return out
    top = walk(0, len(data))
    assert len(top) == 1 and top[0][:2] == ('RIFF', 'AVI ')
    return top[0][2]


def check_avi(data, n_frames, H, W, scale, rate):
    """The structure the issue asks for; returns the frames' JPEG bytes."""
    kids = parse_riff(data)
    assert [k[:2] if k[0] == 'LIST' else k[0] for k in kids] == [('LIST', 'hdrl'), ('LIST', 'movi'), 'idx1']
    hdrl, movi, idx1 = kids
    assert [k[0] for k in hdrl[2]] == ['avih', 'LIST'] and hdrl[2][1][1] == 'strl'
    avih = struct.unpack('<14I', hdrl[2][0][2])
    assert avih[0] == round(1e6 * scale / rate) and avih[3] & 0x10 and avih[4] == n_frames and avih[6] == 1
    assert avih[8:10] == (W, H)
    strl = hdrl[2][1][2]
    assert [k[0] for k in strl] == ['strh', 'strf']
    strh = strl[0][2]
    assert len(strh) == 56 and strh[:8] == b'vidsMJPG'
    assert struct.unpack('<II', strh[20:28]) == (scale, rate) and struct.unpack('<I', strh[32:36])[0] == n_frames
    assert struct.unpack('<4H', strh[48:56]) == (0, 0, W, H)
    bih = struct.unpack('<IiiHH4sIiiII', strl[1][2])
    assert bih[:6] == (40, W, H, 1, 24, b'MJPG')
    chunks = movi[2]
    assert len(chunks) == n_frames and all(c[0] == '00dc' for c in chunks)
    assert all(c[1] % 2 == 0 for c in chunks)
    movi_tag = movi[3] + 8                                                           # where the 'movi' fourcc stands
    assert data[movi_tag:movi_tag + 4] == b'movi'
    assert len(idx1[2]) == 16 * n_frames
    for k, c in enumerate(chunks):
        cc, flags, off, size = struct.unpack('<4sIII', idx1[2][16 * k:16 * k + 16])
        assert cc == b'00dc' and flags == 0x10 and movi_tag + off == c[1] and size == len(c[2])
        assert data[movi_tag + off:movi_tag + off + 4] == b'00dc'
    return [c[2] for c in chunks]
