#!/usr/bin/env python3
"""How many ground-truth boxes get no positive anchor, and how many positives a box gets, under the two matching rules of
the label encoder, per preset and band of box sizes.  Seeded uniform boxes (tests/match_ref.random_boxes:
40 images of 1..8 boxes, default_rng(7) per band).  On the CPU the numpy oracle of tests/match_ref.py does the matching;
with --gpu the library does (encode_labels_batch(..., return_match=True)) -- the two print the same table.

    python tools/match_stats.py [--gpu] [--out profiles/label_match_stats.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

BANDS = [(0.02, 0.08), (0.05, 0.20), (0.10, 0.60)]
C = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpu', action='store_true', help='match on the GPU (the library) instead of the numpy oracle')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import match_ref as mr
    from oracle import boxes as ob
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    say('# tools/match_stats.py%s: boxes without a positive anchor and positives per box, rules reference / paper' % (' --gpu' if args.gpu else ''))
    say('# 40 images of 1..8 boxes per band, centres uniform in the image, sides uniform in the band (fractions of the image side), default_rng(7)')
    say('%-7s %-12s %6s | %10s %10s | %12s %12s | %14s' % ('preset', 'box side', 'boxes', 'none (ref)', 'none (pap)', 'pos/box ref', 'pos/box pap',
                                                             'median pos r/p'))
    for pname in ('vgg300', 'vgg512'):
        preset = ob.get_preset(pname)
        anch, aabs = mr.tables(preset)
        for lo, hi in BANDS:
            sets = mr.random_boxes(np.random.default_rng(7), lo, hi, num_classes=C)
            gts, cls = [s[0] for s in sets], [s[1] for s in sets]
            wins = {}
            for rule in mr.RULES:
                if args.gpu:
                    from ssd_tensorflow_amd import ssdutils as su
                    wins[rule] = su.encode_labels_batch(su.get_preset_by_name(pname), C, gts, cls, match=rule, return_match=True)[1]
                else:
                    wins[rule] = [mr.match_anchors(mr.iou_matrix(g, aabs), rule) for g in gts]
            per = {rule: np.concatenate([np.bincount(w[w >= 0], minlength=len(g)) for w, g in zip(wins[rule], gts)]) for rule in mr.RULES}
            n = len(per['paper'])
            say('%-7s %4.2f - %4.2f %6d | %10d %10d | %12.2f %12.2f | %8d / %-5d' % (
                pname, lo, hi, n, int((per['reference'] == 0).sum()), int((per['paper'] == 0).sum()), per['reference'].mean(),
                per['paper'].mean(), int(np.median(per['reference'])), int(np.median(per['paper']))))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
