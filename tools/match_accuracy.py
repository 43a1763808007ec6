#!/usr/bin/env python3
"""Does the 'paper' matching rule help on small objects?  The shapes detector is trained twice with the
product's own driver -- the same seed, schedule and data, once per rule -- on rectangles of --size of the frame (the
shapes set's default is 0.2;0.5: no box there is without an anchor above 0.5), then both runs' mAP on the held-out
images is taken with the device AP accumulator.  A measurement, not a test.

    python tools/match_accuracy.py [--epochs 40] [--size 0.04;0.10] [--out profiles/label_match_accuracy.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--size', default='0.04;0.10', help='sides of the rectangles, fractions of the frame: lo;hi')
    ap.add_argument('--threshold', type=float, default=0.01)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd import train, ssdutils as su
    from ssd_tensorflow_amd.average_precision import DeviceAPCalculator, APs2mAP
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.training_data import TrainingData, _gt_arrays
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    size = [float(v) for v in args.size.split(';')]
    say('# tools/match_accuracy.py: %s; shapes detector, vgg300, bf16, %d steps at batch 32 per run; rectangles of %.2f .. %.2f of the frame'
        % (torch.cuda.get_device_name(0), args.epochs * 32, size[0], size[1]))
    td = TrainingData('shapes', 'vgg300', num_train=1024, num_valid=128, augment=False, device=0, shapes_size=size)
    held = [(x.clone(), gts) for x, _, gts in td.valid_generator(32, 0)]
    # what the rules make of the held-out boxes themselves
    for rule in su.MATCH_RULES:
        none = total = 0
        for _, gts in held:
            bxs, cls = _gt_arrays(gts)
            _, mt = su.encode_labels_batch(td.preset, td.num_classes, bxs, cls, match=rule, return_match=True)
            for w, g in zip(mt, bxs):
                none += int((np.bincount(w[w >= 0], minlength=len(g)) == 0).sum())
                total += len(g)
        say('# %-9s: %d of the %d held-out boxes get no positive anchor' % (rule, none, total))
    with tempfile.TemporaryDirectory() as tmp:
        secs = {}
        for rule in su.MATCH_RULES:
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                rc = train.main(['--name', os.path.join(tmp, rule), '--tensorboard-dir', os.path.join(tmp, 'tb'), '--data-dir', 'shapes',
                                 '--synthetic-train', '1024', '--synthetic-valid', '128', '--num-workers', '8', '--batch-size', '32',
                                 '--checkpoint-interval', '1000', '--lr-values', '0.0003;0.00075;0.0001', '--lr-boundaries', '96;768',
                                 '--epochs', str(args.epochs), '--dtype', 'bf16', '--augment', 'false', '--match', rule, '--shapes-size', args.size])
            assert rc == 0, 'training failed'
            secs[rule] = time.perf_counter() - t0
        with Session(0) as sess:
            for rule in su.MATCH_RULES:
                net = SSDVGG(sess, 'vgg300')
                net.build_from_metagraph(None, os.path.join(tmp, rule, 'final.npz'), max_batch=32, dtype='bf16')
                calc = DeviceAPCalculator(0, td.num_classes)
                for x, gts in held:
                    net.infer_dev(x)
                    calc.add_pass(net.detect_last_launch(len(gts), args.threshold, detections_cap=None, max_out=200), gts)
                n = calc.num_detections()
                aps = calc.compute_aps()
                say('  --match %-9s held-out mAP %.4f   (%d detections at threshold %.2f; trained in %.0f s)   per class: %s'
                    % (rule, APs2mAP(aps), n, args.threshold, secs[rule], ' '.join('%.3f' % v for v in list(aps.values())[:td.SHAPE_CLASSES])))
                calc.close()
                net.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
