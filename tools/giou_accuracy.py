#!/usr/bin/env python3
"""Does the GIoU localization loss train the shapes detector to tighter boxes than smooth-L1 does?  The detector is
trained with the product's own driver -- the same seed, schedule and data (those of tools/focal_accuracy.py), mining -- once with
--loc-loss smooth_l1 and once with --loc-loss giou at each of --loc-weight 1, 2, 5, 10, and every run's held-out AP is taken with
the device AP accumulator at IoU 0.5, at 0.75 and averaged over 0.5 ... 0.95 (confidence threshold 0.01).  Two settings: the
shapes set's default rectangles under the reference matching, and small ones (--size) under --match paper.  The yardstick is the
smooth-L1 run of the same invocation; the margin is the set's own granularity, 0.0909 (one missed object per class moves an
11-point AP by 1/11).  VOC / COCO AP is not measured: there is no such data set here.  A measurement, not a test.

    python tools/giou_accuracy.py [--epochs 40] [--size 0.04;0.10] [--out profiles/giou_accuracy.txt]
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

MARGIN = 1.0 / 11
RUNS = (('smooth_l1', 1.0), ('giou', 1.0), ('giou', 2.0), ('giou', 5.0), ('giou', 10.0))
IOUS = [0.5 + 0.05 * i for i in range(10)]
THRESHOLD = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--size', default='0.04;0.10', help='sides of the small rectangles of the second setting, fractions of the frame: lo;hi')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd import train
    from ssd_tensorflow_amd.average_precision import DeviceAPCalculator
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.training_data import TrainingData
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    say('# tools/giou_accuracy.py: %s; shapes detector, vgg300, bf16, mining, %d steps at batch 32 per run; held-out AP at confidence '
        'threshold %.2f, IoU 0.50 | 0.75 | mean over 0.50:0.95; margin %.4f' % (torch.cuda.get_device_name(0), args.epochs * 32, THRESHOLD, MARGIN))
    say('# VOC / COCO AP is not measured: no such data set is available to this tool')
    for size, match in (('0.2;0.5', 'reference'), (args.size, 'paper')):
        sz = [float(v) for v in size.split(';')]
        say('# ---- rectangles of %.2f .. %.2f of the frame, --match %s' % (sz[0], sz[1], match))
        td = TrainingData('shapes', 'vgg300', num_train=1024, num_valid=128, augment=False, device=0, shapes_size=sz, match=match)
        held = [(x.clone(), gts) for x, _, gts in td.valid_generator(32, 0)]
        maps = {}
        with tempfile.TemporaryDirectory() as tmp:
            secs, last = {}, {}
            for run in RUNS:
                tag = '%s_%g' % run
                t0 = time.perf_counter()
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    rc = train.main(['--name', os.path.join(tmp, tag), '--tensorboard-dir', os.path.join(tmp, 'tb'), '--data-dir', 'shapes',
                                     '--synthetic-train', '1024', '--synthetic-valid', '128', '--num-workers', '8', '--batch-size', '32',
                                     '--checkpoint-interval', '1000', '--lr-values', '0.0003;0.00075;0.0001', '--lr-boundaries', '96;768',
                                     '--epochs', str(args.epochs), '--dtype', 'bf16', '--augment', 'false', '--match', match,
                                     '--shapes-size', size, '--loc-loss', run[0], '--loc-weight', '%g' % run[1]])
                assert rc == 0, 'training failed'
                secs[run] = time.perf_counter() - t0
                last[run] = [l for l in buf.getvalue().splitlines() if l.startswith('[i] Valid')][-1]
            with Session(0) as sess:
                for run in RUNS:
                    net = SSDVGG(sess, 'vgg300')
                    net.build_from_metagraph(None, os.path.join(tmp, '%s_%g' % run, 'final.npz'), max_batch=32, dtype='bf16')
                    calc = DeviceAPCalculator(0, td.num_classes, minoverlap=IOUS)
                    for x, gts in held:
                        net.infer_dev(x)
                        calc.add_pass(net.detect_last_launch(len(gts), THRESHOLD, detections_cap=None, max_out=200), gts)
                    n = calc.num_detections()
                    aps = np.array([v for v in list(calc.compute_aps().values())[:td.SHAPE_CLASSES]], np.float64)      # [class][IoU]
                    m = aps.mean(0)
                    maps[run] = (float(m[0]), float(m[5]), float(m.mean()))
                    say('  --loc-loss %-9s weight %-4g AP50 %.4f  AP75 %.4f  AP50:95 %.4f   (%d detections; trained in %.0f s)   last epoch: %s'
                        % (run[0], run[1], maps[run][0], maps[run][1], maps[run][2], n, secs[run], last[run]))
                    calc.close()
                    net.close()
        base = maps[RUNS[0]]
        for run in RUNS[1:]:
            d = [a - b for a, b in zip(maps[run], base)]
            verdict = ['better' if v > MARGIN else 'worse' if v < -MARGIN else 'inside the margin' for v in d]
            say('  giou weight %-4g - smooth_l1: AP50 %+.4f (%s)  AP75 %+.4f (%s)  AP50:95 %+.4f (%s)'
                % (run[1], d[0], verdict[0], d[1], verdict[1], d[2], verdict[2]))
        td.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
