#!/usr/bin/env python3
"""Effect of Soft-NMS on detection quality, on the only data this repository can make: the shapes detector,
trained ONCE here (one seed; the schedule of tools/eval_rate.py), decoded with --decode all under the hard rule, the linear rule
(iou 0.45) and the gaussian rule (sigma 0.5), min score = the confidence threshold.  Two held-out sets:
  standard   TrainingData('shapes')'s own held-out images: 1..3 rectangles that never overlap -- no difference is expected;
  crowded    built here (training_data.py is untouched): per image one seeded pair of same-class rectangles of equal size, the
             second shifted along one axis so that their boxes overlap by IoU 0.5 .. 0.7 and painted over the first.  The hard rule
             at 0.45 cannot report both boxes of such a pair.
Reported: VOC07 (11-point) and VOC12 (all-point) mAP at confidence thresholds 0.01 and 0.5, every figure, whichever way it
points; the margin is what ONE missed object per class changes in the 11-point mAP.  VOC / COCO AP on real data is not measurable
here: no such data set is available to this tool.

    python tools/soft_nms_accuracy.py [--epochs 40] [--checkpoint final.npz] [--out profiles/soft_nms_accuracy.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

RULES = (('hard', None), ('linear', 'linear'), ('gaussian', 'gaussian'))


def crowded_set(td, n_images=128, seed=38, size=300):
    """[(float32 BGR image [size, size, 3], [Box, Box])]: the textures of TrainingData._shapes_canvas (class = texture)"""
    from ssd_tensorflow_amd.utils import Box, Point, Size
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_images):
        img = rng.integers(104, 152, (size, size, 3), dtype=np.uint8)
        c = int(rng.integers(0, min(td.SHAPE_CLASSES, td.num_classes)))
        w, h = rng.uniform(0.25, 0.45, 2)
        t = rng.uniform(0.5, 0.7)                      # IoU of two equal boxes shifted by f of their side: (1 - f) / (1 + f)
        f = (1 - t) / (1 + t)
        along_x = bool(rng.integers(0, 2))
        dx, dy = (f * w, 0.0) if along_x else (0.0, f * h)
        cx = rng.uniform(w / 2, 1 - w / 2 - dx)
        cy = rng.uniform(h / 2, 1 - h / 2 - dy)
        boxes = []
        for k, (bx, by) in enumerate(((cx, cy), (cx + dx, cy + dy))):
            x0, x1 = int(round((bx - w / 2) * size)), int(round((bx + w / 2) * size))
            y0, y1 = int(round((by - h / 2) * size)), int(round((by + h / 2) * size))
            p = int(rng.integers(5, 12))
            yy, xx = np.mgrid[y0:y1, x0:x1]
            sgn = 1 if rng.integers(0, 2) else -1
            pat = [(yy // p) % 2, (xx // p) % 2, (yy // p + xx // p) % 2, ((yy + sgn * xx) // p) % 2][c].astype(bool)
            lo, hi = rng.integers(0, 64, 3), rng.integers(192, 256, 3)
            img[y0:y1, x0:x1] = np.where(pat[..., None], hi, lo).astype(np.uint8)
            boxes.append(Box(td.lid2name[c], c, Point(float(bx), float(by)), Size(float(w), float(h))))
        out.append((img.astype(np.float32), boxes))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--checkpoint', default='', help='evaluate this checkpoint instead of training one')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from fp8_accuracy import one_miss_allowance
    from ssd_tensorflow_amd import train
    from ssd_tensorflow_amd.average_precision import APCalculator, APs2mAP
    from ssd_tensorflow_amd.ssdutils import boxes_from_detection
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.training_data import TrainingData
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as tmp:
        ckpt = args.checkpoint
        if not ckpt:
            run = os.path.join(tmp, 'run')
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                rc = train.main(['--name', run, '--tensorboard-dir', os.path.join(tmp, 'tb'), '--data-dir', 'shapes', '--synthetic-train', '1024',
                                 '--synthetic-valid', '128', '--num-workers', '8', '--batch-size', '32', '--checkpoint-interval', '1000',
                                 '--lr-values', '0.0003;0.00075;0.0001', '--lr-boundaries', '96;768', '--epochs', str(args.epochs),
                                 '--dtype', 'bf16', '--augment', 'false'])
            assert rc == 0, 'training failed'
            ckpt = os.path.join(run, 'final.npz')
            say('# tools/soft_nms_accuracy.py: %s; shapes detector, vgg300, bf16, %d steps at batch 32, ONE run (one seed), trained in %.0f s'
                % (torch.cuda.get_device_name(0), args.epochs * 32, time.perf_counter() - t0))
        else:
            say('# tools/soft_nms_accuracy.py: %s; checkpoint %s' % (torch.cuda.get_device_name(0), os.path.basename(ckpt)))
        say('# --decode all, nms_top_k 400, keep_top_k 200; linear: iou 0.45; gaussian: sigma 0.5; min score = the confidence threshold')
        say('# VOC / COCO AP on real data is not measured: no such data set is available to this tool')
        td = TrainingData('shapes', 'vgg300', num_train=1024, num_valid=128, augment=False, device=0)
        standard = [(x.clone(), gts) for x, _, gts in td.valid_generator(32, 0)]
        crowd = crowded_set(td)
        crowded = [(torch.from_numpy(np.stack([im for im, _ in crowd[k:k + 32]])).cuda(), [g for _, g in crowd[k:k + 32]])
                   for k in range(0, len(crowd), 32)]
        with Session(0) as sess:
            net = SSDVGG(sess, 'vgg300')
            net.build_from_metagraph(None, ckpt, max_batch=32, dtype='bf16')
            for title, batches in (('standard held-out set (objects never overlap)', standard),
                                   ('crowded set (pairs of same-class rectangles, box IoU 0.5 .. 0.7)', crowded)):
                counts = {}
                for _, gts in batches:
                    for gt in gts:
                        for box in gt:
                            counts[box.label] = counts.get(box.label, 0) + 1
                allow = one_miss_allowance(counts)
                say('# ---- %s: %d images, objects per class %s; one missed object per class changes the 11-point mAP by %.4f'
                    % (title, sum(len(g) for _, g in batches), dict(sorted(counts.items())), allow))
                for thr in (0.01, 0.5):
                    res = {}
                    for name, kw in RULES:
                        calcs = {p: APCalculator(protocol=p) for p in ('voc07', 'voc12')}
                        ndet = 0
                        for x, gts in batches:
                            net.infer_dev(x)
                            for gt, det in zip(gts, net.detect_last_launch(len(gts), thr, decode='all', soft_nms=kw).get()):
                                boxes = boxes_from_detection(det, td.lid2name)
                                ndet += len(boxes)
                                for c in calcs.values():
                                    c.add_detections(gt, boxes)
                        res[name] = {p: APs2mAP(c.compute_aps()) for p, c in calcs.items()}
                        say('  threshold %.2f  %-9s VOC07 mAP %.4f   VOC12 mAP %.4f   (%d detections)' % (thr, name, res[name]['voc07'], res[name]['voc12'], ndet))
                    for name in ('linear', 'gaussian'):
                        d7, d12 = (res[name][p] - res['hard'][p] for p in ('voc07', 'voc12'))
                        verdict = 'inside the margin' if abs(d7) <= allow else ('better' if d7 > 0 else 'worse')
                        say('  threshold %.2f  %s - hard: VOC07 %+.4f (%s)   VOC12 %+.4f' % (thr, name, d7, verdict, d12))
            net.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
