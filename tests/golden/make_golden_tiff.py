"""Writes tests/golden/tiff/: TIFF files from an encoder that is not this project's -- Pillow with libtiff -- and the arrays
they were made from. Runs only where Pillow has libtiff (PIL.features.check('libtiff')); the tests read the files, never
this script.

    noise_64x80       three frames of 64 x 80 uniform noise
    sparse_50x77      three frames of 50 x 77 at 10 % density, written with STRIP_SIZE = 16 * 154 bytes: four strips, the
                      last of two rows

each as raw, tiff_lzw, packbits and tiff_adobe_deflate, and with Predictor 2 where libtiff accepts the tag (LZW and
Deflate). MANIFEST.txt lists what was written and with which versions."""
import os
import sys

import numpy as np
from PIL import Image, TiffImagePlugin, features
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'tiff')


def arrays():
    rng = np.random.default_rng(20240917)
    noise = rng.integers(0, 65536, (3, 64, 80)).astype(np.uint16)
    vals = rng.integers(1, 65536, (3, 50, 77)).astype(np.uint16)
    sparse = np.where(rng.random((3, 50, 77)) < 0.10, vals, 0).astype(np.uint16)
    return {'noise_64x80': noise, 'sparse_50x77': sparse}


def main():
    if not features.check('libtiff'):
        sys.exit('Pillow without libtiff: the golden files need its encoders')
    os.makedirs(OUT, exist_ok=True)
    lines = [f'Pillow {PIL.__version__}, libtiff {features.version("libtiff")}']
    for name, a in arrays().items():
        np.save(os.path.join(OUT, f'{name}.npy'), a)
        TiffImagePlugin.STRIP_SIZE = 16 * 154 if name.startswith('sparse') else 65536
        for comp in ('raw', 'tiff_lzw', 'packbits', 'tiff_adobe_deflate'):
            for pred in (1, 2):
                if pred == 2 and comp in ('raw', 'packbits'):
                    continue                                              # (libtiff: the tag belongs to LZW and Deflate only)
                fname = f'{name}_{comp}' + ('_pred2' if pred == 2 else '') + '.tif'
                ims = [Image.fromarray(f) for f in a]
                kw = dict(tiffinfo={317: 2}) if pred == 2 else {}
                try:
                    ims[0].save(os.path.join(OUT, fname), save_all=True, append_images=ims[1:], compression=comp, **kw)
                except Exception as e:                                    # the encoder refuses the tag: say so, write nothing
                    lines.append(f'{fname}: refused by the encoder ({type(e).__name__}: {e})')
                    continue
                size = os.path.getsize(os.path.join(OUT, fname))
                assert size < 65536, (fname, size)
                lines.append(f'{fname}: {size} bytes')
    with open(os.path.join(OUT, 'MANIFEST.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
