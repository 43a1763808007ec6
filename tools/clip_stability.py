#!/usr/bin/env python3
"""Does clipping the gradient by its global norm hold the two documented unstable runs?  Both are rerun with the
product's own driver, first with --clip-norm inf -- bitwise the run without clipping, with the norm of every update on record -- then
with a threshold taken from that record, and every run's loss, mAP and norm trajectory is printed:
  A. DESIGN.md 7: the shapes detector in fp32 at a constant learning rate of 1e-3 (it collapsed near step 650: a loss spike, mAP
     back to ~0);
  B. DESIGN.md 31: small rectangles (--shapes-size 0.04;0.10) under --match paper with --loc-loss giou --loc-weight 1, bf16, the
     learning test's schedule (the confidence loss climbs from 5 to ~20 and the run does not train).
The threshold is MULTIPLE x the median norm of the healthy phase: the epochs after the first and before the first epoch whose
training loss rises by more than a quarter over the lowest so far (all epochs after the first if none does).  MULTIPLE = 2: the
typical update of the healthy phase passes untouched, and no update moves the weights more than twice as far as a typical one.
One seed per run: the evidence level of DESIGN.md 31's accuracy table.  A measurement, not a test.

    python tools/clip_stability.py [--epochs-a 56] [--epochs-b 40] [--out profiles/grad_clip_stability.txt]
"""
import argparse
import contextlib
import io
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MULTIPLE = 2.0
NUM = r'([-+\d.eE]+|nan|inf)'


def parse(text, epochs):
    """per epoch: training (total, localization, confidence), (training, validation) mAP from epoch 2 on, (median, max, clipped, skipped)"""
    tr = [tuple(map(float, m.groups())) for m in re.finditer(r'\[i\] Train +\d+/\d+ +total %s +localization %s +confidence %s' % (NUM, NUM, NUM), text)]
    maps = [tuple(map(float, m.groups())) for m in re.finditer(r'\[i\] mAP +\d+/\d+ +training %s +validation %s' % (NUM, NUM), text)]
    gn = [(float(m.group(1)), float(m.group(2)), int(m.group(3)), int(m.group(4)))
          for m in re.finditer(r'\[i\] Grad +\d+/\d+ +norm median %s +max %s +clipped (\d+) +skipped (\d+)' % (NUM, NUM), text)]
    assert len(tr) == epochs and len(maps) == epochs - 1 and len(gn) == epochs, text[-2000:]
    return dict(train=tr, maps=[(0.0, 0.0)] + maps, norms=gn)


def healthy_phase(train):
    """(first, last) epoch indices (0-based, inclusive) of the healthy phase, and the epoch that ends it (None: no rise)"""
    low = train[0][0]
    for e in range(1, len(train)):
        if train[e][0] > 1.25 * low:
            return (1, max(e - 1, 1)), e
        low = min(low, train[e][0])
    return (1, len(train) - 1), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs-a', type=int, default=56)
    ap.add_argument('--epochs-b', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd import train
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    def fmt(values, spec):
        return ' '.join(spec % v for v in values)

    say('# tools/clip_stability.py: %s; shapes detector, vgg300, 1024 training / 128 held-out pictures, batch 32 (32 updates per epoch), '
        'mining; mAP: the driver\'s, VOC07 11-point at confidence 0.5; ONE seed per run' % torch.cuda.get_device_name(0))
    settings = (
        ('A', 'DESIGN.md 7: fp32, constant learning rate 1e-3, rectangles 0.2 .. 0.5, --match reference, smooth_l1', args.epochs_a,
         ['--dtype', 'f32', '--lr-values', '0.001', '--lr-boundaries', '']),
        ('B', 'DESIGN.md 31: bf16, rectangles 0.04 .. 0.10, --match paper, --loc-loss giou --loc-weight 1, lr 3e-4 / 7.5e-4 / 1e-4 at 96 / 768',
         args.epochs_b, ['--dtype', 'bf16', '--lr-values', '0.0003;0.00075;0.0001', '--lr-boundaries', '96;768', '--match', 'paper',
                         '--shapes-size', '0.04;0.10', '--loc-loss', 'giou', '--loc-weight', '1']),
    )
    with tempfile.TemporaryDirectory() as tmp:
        def run(tag, epochs, extra, clip):
            buf = io.StringIO()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(buf):
                rc = train.main(['--name', os.path.join(tmp, tag), '--tensorboard-dir', os.path.join(tmp, 'tb'), '--data-dir', 'shapes',
                                 '--synthetic-train', '1024', '--synthetic-valid', '128', '--num-workers', '8', '--batch-size', '32',
                                 '--checkpoint-interval', '1000', '--epochs', str(epochs), '--augment', 'false', '--clip-norm', repr(float(clip))] + extra)
            assert rc == 0, buf.getvalue()[-2000:]
            r = parse(buf.getvalue(), epochs)
            r['secs'] = time.perf_counter() - t0
            return r

        def show(name, r):
            say('  %s  (%.0f s)' % (name, r['secs']))
            say('    training loss by epoch   ' + fmt([t[0] for t in r['train']], '%.2f'))
            say('    confidence loss          ' + fmt([t[2] for t in r['train']], '%.2f'))
            say('    training mAP             ' + fmt([m[0] for m in r['maps']], '%.2f'))
            say('    held-out mAP             ' + fmt([m[1] for m in r['maps']], '%.2f'))
            say('    norm, median of epoch    ' + fmt([g[0] for g in r['norms']], '%.3g'))
            say('    norm, maximum of epoch   ' + fmt([g[1] for g in r['norms']], '%.3g'))
            say('    clipped updates          ' + fmt([g[2] for g in r['norms']], '%d'))
            say('    skipped updates          ' + fmt([g[3] for g in r['norms']], '%d'))
            peak = int(np.argmax([m[0] for m in r['maps']]))
            say('    => clipped %d and skipped %d of %d updates; highest training loss after epoch 5: %.2f; training mAP peaks at %.3f (epoch %d), '
                'lowest after the peak %.3f; final mAP training %.4f, held-out %.4f'
                % (sum(g[2] for g in r['norms']), sum(g[3] for g in r['norms']), 32 * len(r['train']), max(t[0] for t in r['train'][5:]),
                   r['maps'][peak][0], peak + 1, min(m[0] for m in r['maps'][peak:]), r['maps'][-1][0], r['maps'][-1][1]))

        for key, title, epochs, extra in settings:
            say('# ---- %s. %s; %d epochs = %d updates' % (key, title, epochs, 32 * epochs))
            base = run(key + '_inf', epochs, extra, float('inf'))
            show('--clip-norm inf (the run without clipping, measured)', base)
            (lo, hi), end = healthy_phase(base['train'])
            med = float(np.median([g[0] for g in base['norms'][lo:hi + 1]]))
            thr = float(np.float32(MULTIPLE * med))
            say('  healthy phase: epochs %d .. %d (%s); median of their median norms %.4g; threshold = %g x that = %.4g'
                % (lo + 1, hi + 1, 'the training loss rises by more than a quarter in epoch %d' % (end + 1) if end is not None
                   else 'the training loss never rises by more than a quarter over its lowest', med, MULTIPLE, thr))
            clipped = run(key + '_clip', epochs, extra, thr)
            show('--clip-norm %.4g' % thr, clipped)
            d = clipped['maps'][-1][1] - base['maps'][-1][1]
            say('  %s: final held-out mAP %.4f without against %.4f with clipping (%+.4f); final training loss %.3f against %.3f'
                % (key, base['maps'][-1][1], clipped['maps'][-1][1], d, base['train'][-1][0], clipped['train'][-1][0]))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
