#!/usr/bin/env python3
"""Does AdamW train what the momentum rule does not, and does it cost anything where momentum works?  The product's
own driver on the shapes set, every run's loss and mAP trajectory printed:
  A. DESIGN.md 7's learnable set (rectangles 0.2 .. 0.5, --match reference, smooth_l1, fp32) under the learning test's schedule
     (3e-4 until update 96, 7.5e-4 until 768, 1e-4 after): momentum against adamw;
  B. DESIGN.md 31's small rectangles (--shapes-size 0.04;0.10, --match paper, --loc-loss giou --loc-weight 1, bf16), where momentum ends
     at mAP 0.00 and --clip-norm 100.4 at 0.68: momentum, momentum clipped, adamw and adamw clipped at 100.4.
AdamW's learning rate is not known in advance: three peaks are tried, 1e-4, 3e-4 and 1e-3, ALL reported, with the momentum schedule's
shape (0.4 x the peak until update 96 as warm-up, the peak until 768, 0.133 x after), --adam-decay 0.01, the L2 term at its adamw
default of 0.  ONE seed per run: the evidence level of DESIGN.md 31's accuracy table.  A measurement, not a test.

    python tools/adamw_stability.py [--epochs 40] [--out profiles/adamw_stability.txt]
"""
import argparse
import contextlib
import io
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NUM = r'([-+\d.eE]+|nan|inf)'
PEAKS = (1e-4, 3e-4, 1e-3)
CLIP_B = 100.4


def parse(text, epochs):
    tr = [tuple(map(float, m.groups())) for m in re.finditer(r'\[i\] Train +\d+/\d+ +total %s +localization %s +confidence %s' % (NUM, NUM, NUM), text)]
    maps = [tuple(map(float, m.groups())) for m in re.finditer(r'\[i\] mAP +\d+/\d+ +training %s +validation %s' % (NUM, NUM), text)]
    gn = [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r'\[i\] Grad +\d+/\d+ .* clipped (\d+) +skipped (\d+)', text)]
    assert len(tr) == epochs and len(maps) == epochs - 1, text[-2000:]
    return dict(train=tr, maps=[(0.0, 0.0)] + maps, clipped=sum(g[0] for g in gn), skipped=sum(g[1] for g in gn))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd import train
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)
        if args.out:      # as the runs go: a run takes a minute
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    def fmt(values, spec):
        return ' '.join(spec % v for v in values)

    E = args.epochs
    say('# tools/adamw_stability.py: %s; shapes detector, vgg300, 1024 training / 128 held-out pictures, batch 32 (32 updates per epoch), '
        'mining, %d epochs = %d updates; mAP: the driver\'s, VOC07 11-point at confidence 0.5; ONE seed per run' % (torch.cuda.get_device_name(0), E, 32 * E))
    momentum_lr = ['--lr-values', '0.0003;0.00075;0.0001', '--lr-boundaries', '96;768']

    def adamw_lr(peak):
        return ['--optimizer', 'adamw', '--adam-decay', '0.01', '--lr-values', '%g;%g;%g' % (0.4 * peak, peak, peak / 7.5), '--lr-boundaries', '96;768']

    settings = (
        ('A', 'DESIGN.md 7: fp32, rectangles 0.2 .. 0.5, --match reference, smooth_l1', ['--dtype', 'f32'], (0.0,)),
        ('B', 'DESIGN.md 31: bf16, rectangles 0.04 .. 0.10, --match paper, --loc-loss giou --loc-weight 1',
         ['--dtype', 'bf16', '--match', 'paper', '--shapes-size', '0.04;0.10', '--loc-loss', 'giou', '--loc-weight', '1'], (0.0, CLIP_B)),
    )
    summary = []
    with tempfile.TemporaryDirectory() as tmp:
        def run(tag, extra):
            buf = io.StringIO()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(buf):
                rc = train.main(['--name', os.path.join(tmp, tag), '--tensorboard-dir', os.path.join(tmp, 'tb'), '--data-dir', 'shapes',
                                 '--synthetic-train', '1024', '--synthetic-valid', '128', '--num-workers', '8', '--batch-size', '32',
                                 '--checkpoint-interval', '1000', '--epochs', str(E), '--augment', 'false'] + extra)
            assert rc == 0, buf.getvalue()[-2000:]
            r = parse(buf.getvalue(), E)
            r['secs'] = time.perf_counter() - t0
            return r

        def show(key, name, r):
            say('  %s  (%.0f s)' % (name, r['secs']))
            say('    training loss by epoch   ' + fmt([t[0] for t in r['train']], '%.2f'))
            say('    training mAP             ' + fmt([m[0] for m in r['maps']], '%.2f'))
            say('    held-out mAP             ' + fmt([m[1] for m in r['maps']], '%.2f'))
            first = next((e + 1 for e, m in enumerate(r['maps']) if m[1] >= 0.5), None)
            line = ('%s %-34s final loss %6.3f  highest loss after epoch 5 %6.2f  final mAP training %.4f held-out %.4f  held-out >= 0.5 from epoch %s  clipped %d skipped %d'
                    % (key, name, r['train'][-1][0], max(t[0] for t in r['train'][5:]), r['maps'][-1][0], r['maps'][-1][1], first, r['clipped'], r['skipped']))
            say('    => ' + line)
            summary.append(line)

        for key, title, extra, clips in settings:
            say('# ---- %s. %s' % (key, title))
            for clip in clips:
                c = ['--clip-norm', repr(clip)] if clip else []
                ctag = ' --clip-norm %g' % clip if clip else ''
                show(key, 'momentum 3e-4/7.5e-4/1e-4' + ctag, run('%s_m_%g' % (key, clip), extra + momentum_lr + c))
                for peak in PEAKS:
                    show(key, 'adamw peak %g' % peak + ctag, run('%s_a_%g_%g' % (key, peak, clip), extra + adamw_lr(peak) + c))
    say('# ---- summary, one line per run')
    for line in summary:
        say(line)


if __name__ == '__main__':
    main()
