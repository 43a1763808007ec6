#!/usr/bin/env python3
"""What mosaic augmentation changes in detection accuracy.  Trains the shapes detector twice with the product's own
driver -- same seeds, schedule and flags (--augment true --match paper; the schedule of tools/tile_accuracy.py), one run with
--mosaic 0 and one with --mosaic 0.5 --mosaic-off-epochs 4 -- and evaluates VOC07 mAP at thresholds 0.5 and 0.01 (NMS, 200 boxes,
one f32 handle per arm) on

  (a) the held-out set (128 pictures through the validation recipe), and
  (b) the held-out pictures pasted 2 x 2 and resized to the preset in one piece: the same objects at half size.

ONE seed per arm: a difference below what one missed object per class changes in mAP says nothing.  No number is fixed in advance;
if neither arm learns under --augment true in this schedule the tool says so and tunes nothing.

    python tools/mosaic_accuracy.py [--epochs 40] [--out profiles/mosaic_accuracy.txt]
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

ARMS = [('--mosaic 0', []), ('--mosaic 0.5 --mosaic-off-epochs 4', ['--mosaic', '0.5', '--mosaic-off-epochs', '4'])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from fp8_accuracy import one_miss_allowance
    from ssd_tensorflow_amd import train
    from ssd_tensorflow_amd import transforms as T
    from ssd_tensorflow_amd.average_precision import APCalculator, APs2mAP
    from ssd_tensorflow_amd.ssdutils import boxes_from_detection
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.training_data import TrainingData
    from ssd_tensorflow_amd.utils import Box, Point, Size
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as tmp:
        ckpts = {}
        for k, (name, flags) in enumerate(ARMS):
            run = os.path.join(tmp, 'run%d' % k)
            t0 = time.perf_counter()
            log = io.StringIO()
            with contextlib.redirect_stdout(log):
                rc = train.main(['--name', run, '--tensorboard-dir', os.path.join(tmp, 'tb%d' % k), '--data-dir', 'shapes', '--synthetic-train', '1024',
                                 '--synthetic-valid', '128', '--num-workers', '8', '--batch-size', '32', '--checkpoint-interval', '1000',
                                 '--lr-values', '0.0003;0.00075;0.0001', '--lr-boundaries', '96;768', '--epochs', str(args.epochs),
                                 '--dtype', 'bf16', '--augment', 'true', '--match', 'paper'] + flags)
            assert rc == 0, 'training failed:\n' + log.getvalue()[-2000:]
            ckpts[name] = os.path.join(run, 'final.npz')
            say('# arm %-36s shapes detector, vgg300, bf16, --augment true --match paper, %d steps at batch 32, trained in %.0f s'
                % (name, args.epochs * 32, time.perf_counter() - t0))
            for ln in log.getvalue().splitlines():          # the feed of the first and the last epoch, the loss of the last
                words = ln.split()
                at = words[2] if len(words) > 2 else ''
                if ln.startswith('[i] Feed') and at in ('1/%d' % args.epochs, '%d/%d' % (args.epochs, args.epochs)):
                    say('#   ' + ln)
                if ln.startswith('[i] Train') and at == '%d/%d' % (args.epochs, args.epochs):
                    say('#   ' + ln)
        td = TrainingData('shapes', 'vgg300', num_train=1024, num_valid=128, augment=True, device=0, match='paper')
        xs, gts = [], []
        for x, _, g in td.valid_generator(32, 0):
            xs.append(x.clone()); gts += list(g)
        held = torch.cat(xs)
        pics = held.clamp(0, 255).round().to(torch.uint8).cpu().numpy()
        side = pics.shape[1]
        pasted, pgts, counts, pcounts = [], [], {}, {}
        for g in gts:
            for b in g:
                counts[b.label] = counts.get(b.label, 0) + 1
        for k in range(0, len(pics) - 3, 4):
            m = np.zeros((2 * side, 2 * side, 3), np.uint8)
            boxes = []
            for q in range(4):
                r, c = divmod(q, 2)
                m[r * side:(r + 1) * side, c * side:(c + 1) * side] = pics[k + q]
                for b in gts[k + q]:
                    boxes.append(Box(b.label, b.labelid, Point((c + b.center.x) / 2, (r + b.center.y) / 2), Size(b.size.w / 2, b.size.h / 2)))
                    pcounts[b.label] = pcounts.get(b.label, 0) + 1
            plan = T.ImagePlan(m)
            plan.resize = (side, side, T.INTER_LINEAR)
            pasted.append(plan); pgts.append(boxes)
        half = T.augment_batch(pasted, side, side, device=0)
        say('# (a) held-out set: %d pictures, objects per class %s' % (len(pics), dict(sorted(counts.items()))))
        say('# (b) the same pictures pasted 2 x 2 into %d pictures of %d x %d and resized to %d x %d (INTER_LINEAR): objects at half size'
            % (len(pasted), 2 * side, 2 * side, side, side))
        scores = {}
        for name, ckpt in ckpts.items():
            with Session(0) as sess:
                net = SSDVGG(sess, 'vgg300')
                net.build_from_metagraph(None, ckpt, max_batch=32, dtype='f32')
                for tag, x, truth in (('(a) held-out', held, gts), ('(b) pasted 2 x 2', half, pgts)):
                    for thr in (0.5, 0.01):
                        calc, ndet = APCalculator(), 0
                        for o in range(0, x.shape[0], 32):
                            part = x[o:o + 32].contiguous()
                            net.infer_dev(part)
                            for gt, det in zip(truth[o:o + 32], net.detect_last_launch(part.shape[0], thr, 200, None).get()):
                                boxes = boxes_from_detection(det, td.lid2name)
                                ndet += len(boxes)
                                calc.add_detections(gt, boxes)
                        aps = calc.compute_aps()
                        scores[name, tag, thr] = (APs2mAP(aps), aps, ndet)
                net.close()
        td.close()
        say('# VOC07 (11-point) mAP, f32 handle, NMS, at most 200 boxes per picture')
        for tag in ('(a) held-out', '(b) pasted 2 x 2'):
            for thr in (0.5, 0.01):
                for name, _ in ARMS:
                    r = scores[name, tag, thr]
                    say('  %-18s threshold %.2f  %-36s mAP %.4f   %s   (%d detections)' % (
                        tag, thr, name, r[0], '  '.join('%s %.4f' % (k, v) for k, v in sorted(r[1].items())), r[2]))
                say('  %-18s threshold %.2f  mosaic - plain = %+.4f' % (tag, thr, scores[ARMS[1][0], tag, thr][0] - scores[ARMS[0][0], tag, thr][0]))
        say('# one missed object per class changes mAP by %.4f on (a) and by %.4f on (b); ONE seed per arm' % (
            one_miss_allowance(counts), one_miss_allowance(pcounts)))
        if max(r[0] for r in scores.values()) < 0.05:
            say('# NEITHER arm learns under --augment true in this schedule (every mAP below 0.05): the comparison says nothing about mosaics')
        say('# real data is NOT measured: there is no data set here, only synthetic shapes')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
