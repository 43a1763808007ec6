#!/usr/bin/env python3
"""What the 1000 grid costs the COCO numbers.  This library's boxes are integers on a 1000 x 1000 grid (the
decode's, and prop2abs of every ground-truth box); pycocotools evaluates float pixels.  The CPU oracle of tests/coco_ref.py
runs twice on one seeded set of 640 x 480 images with COCO-like box sizes: on the float pixel boxes themselves (sample_scale 1,
the grid IS the pixel grid), and on the same boxes taken through abs2prop / prop2abs onto the 1000 grid (sample_scale W*H/1e6).
The annotation areas, confidences, classes and crowd flags are the same in both.  No GPU is needed.

    python tools/coco_grid_error.py [--images 500] [--seeds 3] [--out profiles/coco_grid_error.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
W, H = 640, 480


def load_utils():
    """ssd_tensorflow_amd/utils.py alone: the package itself loads the HIP library"""
    import importlib.util
    spec = importlib.util.spec_from_file_location('ssd_utils_only', os.path.join(ROOT, 'ssd_tensorflow_amd', 'utils.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pixel_set(rng, nimg, ncls):
    """float pixel boxes (xmin, xmax, ymin, ymax): areas log-uniform over 30 .. 1e5 px^2; a detection is its box shifted and
    scaled by a few per cent to some tens of per cent, so that IoUs fall on both sides of every threshold"""
    gb, gk, gs, gf, ga, db, dk, ds, dc = [], [], [], [], [], [], [], [], []
    for s in range(nimg):
        for _ in range(int(rng.integers(1, 12))):
            area = 10.0 ** rng.uniform(1.5, 5.0)
            w = min(np.sqrt(area) * rng.uniform(0.5, 2.0), W - 1.0); h = min(area / w, H - 1.0)
            x0 = rng.uniform(0, W - w); y0 = rng.uniform(0, H - h)
            k = int(rng.integers(0, ncls))
            crowd = rng.random() < 0.01
            gb.append([x0, x0 + w, y0, y0 + h]); gk.append(k); gs.append(s); gf.append(3 if crowd else 0); ga.append(w * h * rng.uniform(0.5, 1.0))
            for _rep in range(int(rng.integers(0, 3))):
                e = rng.choice([0.03, 0.1, 0.2]) * rng.standard_normal(4)
                db.append([x0 + e[0] * w, x0 + w + e[1] * w, y0 + e[2] * h, y0 + h + e[3] * h])
                dk.append(k if rng.random() < 0.9 else int(rng.integers(0, ncls))); ds.append(s); dc.append(rng.random())
        for _ in range(int(rng.integers(0, 6))):
            w, h = rng.uniform(5, 300), rng.uniform(5, 300); x0, y0 = rng.uniform(0, W - w), rng.uniform(0, H - h)
            db.append([x0, x0 + w, y0, y0 + h]); dk.append(int(rng.integers(0, ncls))); ds.append(s); dc.append(rng.random() * 0.6)
    return dict(det_box=np.array(db), det_conf=np.array(dc, np.float32), det_cls=np.array(dk), det_sample=np.array(ds), gt_box=np.array(gb),
                gt_cls=np.array(gk), gt_sample=np.array(gs), gt_flags=np.array(gf), gt_area=np.array(ga), ncls=ncls)


def on_grid(boxes, U):
    img, grid = U.Size(W, H), U.Size(1000, 1000)
    return np.array([U.prop2abs(*U.abs2prop(b[0], b[1], b[2], b[3], img), grid) for b in boxes], np.float64).reshape(-1, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=500)
    ap.add_argument('--classes', type=int, default=10)
    ap.add_argument('--seeds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import coco_ref as R
    U = load_utils()
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    say('# tools/coco_grid_error.py: the CPU oracle (tests/coco_ref.py) on float pixel boxes and on the same boxes on the 1000 grid')
    say('# %d images of %d x %d, %d classes, thresholds 0.50:0.05:0.95; one table per seed' % (args.images, W, H, args.classes))
    worst = dict.fromkeys(R.SUMMARY_NAMES, 0.0)
    for seed in range(args.seeds):
        s = pixel_set(np.random.default_rng(100 + seed), args.images, args.classes)
        common = (s['det_conf'], s['det_cls'], s['det_sample'])
        gt = (s['gt_cls'], s['gt_sample'], s['gt_flags'], s['gt_area'])
        # float32 holds these pixel coordinates to 2^-14 px: the oracle's float32 detection boxes are float pixels still
        px = R.summarize(*R.evaluate(s['det_box'], *common, s['gt_box'], *gt, np.ones(args.images), s['ncls']))
        gr = R.summarize(*R.evaluate(on_grid(s['det_box'], U), *common, on_grid(s['gt_box'], U), *gt, np.full(args.images, W * H / 1e6), s['ncls']))
        say('# seed %d: %d detections, %d ground-truth boxes' % (100 + seed, len(s['det_conf']), len(s['gt_cls'])))
        say('  %-6s %12s %12s %12s' % ('', 'float pixels', '1000 grid', 'difference'))
        for name in R.SUMMARY_NAMES:
            say('  %-6s %12.6f %12.6f %+12.6f' % (name, px[name], gr[name], gr[name] - px[name]))
            worst[name] = max(worst[name], abs(gr[name] - px[name]))
    say('# largest |difference| over the seeds: ' + '  '.join('%s %.4f' % kv for kv in worst.items()))
    say('# largest of all: %.4f (%s)' % (max(worst.values()), max(worst, key=worst.get)))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
