#!/usr/bin/env python3
"""Does the focal loss train the shapes detector as well as hard-negative mining does?  The detector is trained
twice with the product's own driver -- the same seed, schedule and data, once per loss (focal: gamma 2, alpha 0.25, prior 0.01) --
and both runs' mAP on the held-out images is taken with the device AP accumulator at confidence thresholds 0.5 and 0.01.  Two
settings: the shapes set's default rectangles under the reference matching, and small ones (--size) under --match paper.  The
yardstick is the mining run of the same invocation; the margin is the set's own granularity, 0.0909 (one missed object per
class moves an 11-point AP by 1/11).  VOC / COCO AP is not measured: there is no such data set here.  A measurement, not a test.

    python tools/focal_accuracy.py [--epochs 40] [--size 0.04;0.10] [--out profiles/focal_accuracy.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGIN = 1.0 / 11
LOSSES = ('mining', 'focal')
THRESHOLDS = (0.5, 0.01)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--size', default='0.04;0.10', help='sides of the small rectangles of the second setting, fractions of the frame: lo;hi')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd import train
    from ssd_tensorflow_amd.average_precision import DeviceAPCalculator, APs2mAP
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.training_data import TrainingData
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    say('# tools/focal_accuracy.py: %s; shapes detector, vgg300, bf16, %d steps at batch 32 per run; focal: gamma 2, alpha 0.25, prior 0.01; '
        'margin %.4f' % (torch.cuda.get_device_name(0), args.epochs * 32, MARGIN))
    say('# VOC / COCO AP is not measured: no such data set is available to this tool')
    for size, match in (('0.2;0.5', 'reference'), (args.size, 'paper')):
        sz = [float(v) for v in size.split(';')]
        say('# ---- rectangles of %.2f .. %.2f of the frame, --match %s' % (sz[0], sz[1], match))
        td = TrainingData('shapes', 'vgg300', num_train=1024, num_valid=128, augment=False, device=0, shapes_size=sz, match=match)
        held = [(x.clone(), gts) for x, _, gts in td.valid_generator(32, 0)]
        maps = {}
        with tempfile.TemporaryDirectory() as tmp:
            secs, last = {}, {}
            for loss in LOSSES:
                t0 = time.perf_counter()
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    rc = train.main(['--name', os.path.join(tmp, loss), '--tensorboard-dir', os.path.join(tmp, 'tb'), '--data-dir', 'shapes',
                                     '--synthetic-train', '1024', '--synthetic-valid', '128', '--num-workers', '8', '--batch-size', '32',
                                     '--checkpoint-interval', '1000', '--lr-values', '0.0003;0.00075;0.0001', '--lr-boundaries', '96;768',
                                     '--epochs', str(args.epochs), '--dtype', 'bf16', '--augment', 'false', '--match', match,
                                     '--shapes-size', size, '--loss', loss, '--focal-gamma', '2', '--focal-alpha', '0.25', '--focal-prior', '0.01'])
                assert rc == 0, 'training failed'
                secs[loss] = time.perf_counter() - t0
                last[loss] = [l for l in buf.getvalue().splitlines() if l.startswith('[i] Valid')][-1]
            with Session(0) as sess:
                for loss in LOSSES:
                    net = SSDVGG(sess, 'vgg300')
                    net.build_from_metagraph(None, os.path.join(tmp, loss, 'final.npz'), max_batch=32, dtype='bf16')
                    for thr in THRESHOLDS:
                        calc = DeviceAPCalculator(0, td.num_classes)
                        for x, gts in held:
                            net.infer_dev(x)
                            calc.add_pass(net.detect_last_launch(len(gts), thr, detections_cap=None, max_out=200), gts)
                        n = calc.num_detections()
                        aps = calc.compute_aps()
                        maps[loss, thr] = APs2mAP(aps)
                        say('  --loss %-7s threshold %.2f  held-out mAP %.4f   (%d detections; trained in %.0f s)   per class: %s'
                            % (loss, thr, maps[loss, thr], n, secs[loss], ' '.join('%.3f' % v for v in list(aps.values())[:td.SHAPE_CLASSES])))
                        calc.close()
                    say('  --loss %-7s last epoch: %s' % (loss, last[loss]))
                    net.close()
        for thr in THRESHOLDS:
            d = maps['focal', thr] - maps['mining', thr]
            verdict = 'better' if d > MARGIN else 'worse' if d < -MARGIN else 'not better, not worse: inside the margin'
            say('  threshold %.2f: focal - mining %+.4f: %s' % (thr, d, verdict))
        td.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
