#!/usr/bin/env python3
"""Writes tests/golden/j2_jpeg_encode.npz: source pixels and the files Pillow (libjpeg-turbo) encodes them to, for
tests/test_jpeg_encode.py and tests/test_gpu_jpeg_encode.py.  Needs Pillow; the tests do not.

    python tools/make_jpeg_encode_golden.py

Keys: src_names / src_<j>_bgr (uint8 [h, w, 3] BGR pictures), case_names / case_src / case_quality / case_sampling ('4:4:4', ...) /
case_<i>_jpg (the bytes of Image.save(..., 'JPEG', quality=q, subsampling=s) of picture case_src[i]), pillow_version,
libjpeg_turbo_version.
"""
import io
import os

import numpy as np
import PIL
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (w, h): every remainder mod 16 in {0, 1, 8, 15} on both sides, even and odd counts of 8 x 8 blocks, one-pixel strips
SIZES = [(1, 1), (8, 8), (15, 17), (16, 16), (17, 15), (33, 24), (47, 63), (64, 48), (81, 80), (1, 40), (144, 96), (95, 65),
         (104, 88), (40, 1)]
KINDS = ['smooth', 'noise', 'edges', 'primaries']
QUALITIES = [1, 30, 75, 95, 100]
SAMPLINGS = ['4:4:4', '4:2:2', '4:2:0']


def picture(rng, w, h, kind):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == 'smooth':
        img = np.stack([128 + 100 * np.sin(x / 7.0 + y / 13.0), 255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1)], -1)
    elif kind == 'noise':
        img = rng.integers(0, 256, (h, w, 3)).astype(np.float64)
    else:
        img = np.zeros((h, w, 3)) + rng.integers(0, 256, 3)
        for _ in range(6):
            x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
            x1, y1 = x0 + int(rng.integers(1, w // 2 + 2)), y0 + int(rng.integers(1, h // 2 + 2))
            img[y0:y1, x0:x1] = rng.integers(0, 256, 3) if kind == 'edges' else 255 * rng.integers(0, 2, 3)      # saturated primaries
    return np.clip(img, 0, 255).astype(np.uint8)


def main():
    rng = np.random.default_rng(20240614)
    out = {'pillow_version': np.array(PIL.__version__), 'libjpeg_turbo_version': np.array(str(features.version('libjpeg_turbo')))}
    src_names, case_names, case_src, case_quality, case_sampling = [], [], [], [], []
    for i, (w, h) in enumerate(SIZES):
        # every size with two kinds, every kind with seven sizes; the biggest pictures are not the noise ones (file size)
        for kind in (KINDS[i % 4], KINDS[(i + 2) % 4]):
            j = len(src_names)
            bgr = picture(rng, w, h, kind)
            src_names.append('%s_%dx%d' % (kind, w, h))
            out['src_%d_bgr' % j] = bgr
            for s in SAMPLINGS:
                for q in QUALITIES:
                    buf = io.BytesIO()
                    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, 'JPEG', quality=q, subsampling=s)
                    out['case_%d_jpg' % len(case_names)] = np.frombuffer(buf.getvalue(), np.uint8)
                    case_names.append('%s_%s_q%d' % (src_names[j], s.replace(':', ''), q))
                    case_src.append(j); case_quality.append(q); case_sampling.append(s)
    out.update(src_names=np.array(src_names), case_names=np.array(case_names), case_src=np.array(case_src, np.int32),
               case_quality=np.array(case_quality, np.int32), case_sampling=np.array(case_sampling))
    path = os.path.join(ROOT, 'tests', 'golden', 'j2_jpeg_encode.npz')
    np.savez_compressed(path, **out)
    print('%s: %d pictures, %d files, %d bytes (Pillow %s, libjpeg-turbo %s)' % (path, len(src_names), len(case_names), os.path.getsize(path),
                                                                                 out['pillow_version'], out['libjpeg_turbo_version']))


if __name__ == '__main__':
    main()
