#!/usr/bin/env python3
"""GPU time of the label encode under the two matching rules: ssd_encode_labels_resident_ex with everything
in HBM, HIP events around the call's kernels alone, ONE process, interleaved rounds.  vgg300, 20 classes:
  (a) batch 32, 1..8 boxes per image (a training batch);
  (b) batch 32, 100 boxes per image (a crowded COCO batch: most boxes live in the workspace, not in LDS);
  (c) one image of 100 identical boxes: every round of the bipartite stage sends all remaining boxes back to the
      anchor table (the rescan worst case).
The `reference` column runs the kernels of the encoder as it was before the rule existed; it is the yardstick.

    python tools/match_rate.py [--rounds 7] [--reps 20] [--out profiles/label_match_rate.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_MS = (32 / 4899 * 1e3, 32 / 4775 * 1e3)      # README: bf16, vgg300 batch 32, 4775 - 4899 images/s by box
C = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20, help="timed calls per leg and round (their median is the round's figure)")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd import ssdutils as su
    from ssd_tensorflow_amd._lib import lib, check
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    rng = np.random.default_rng(3)

    def uniform_boxes(n, lo, hi):
        w, h = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
        return np.stack([rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2), w, h], 1)

    cases = [
        ('(a) batch 32, 1..8 boxes per image, sides 0.02..0.6', [uniform_boxes(int(rng.integers(1, 9)), 0.02, 0.6) for _ in range(32)]),
        ('(b) batch 32, 100 boxes per image, sides 0.02..0.3', [uniform_boxes(100, 0.02, 0.3) for _ in range(32)]),
        ('(c) one image, 100 identical boxes', [np.tile(np.array([[0.5, 0.5, 0.3, 0.3]]), (100, 1))]),
    ]
    dev = torch.device('cuda', 0)
    preset = su.get_preset_by_name('vgg300')
    A = preset.num_anchors
    say('# tools/match_rate.py: %s; ssd_encode_labels_resident_ex, vgg300, %d classes; HIP events around the call, %d interleaved rounds '
        'of %d calls per rule: median of the rounds\' medians (min ... max)' % (torch.cuda.get_device_name(0), C, args.rounds, args.reps))
    say('# beside it: one bf16 training step of vgg300 at batch 32 takes %.2f - %.2f ms (README, bench.py)' % STEP_MS)
    worst = 0.0
    for title, gts in cases:
        cls = [rng.integers(0, C, len(g)).astype(np.int32) for g in gts]
        gt, gcls, offs = su._pack_gt(gts, cls)
        b, ntot = len(gts), int(gcls.shape[0])
        d_gt, d_cls, d_off = (torch.from_numpy(a).to(dev) for a in (gt, gcls, offs))
        vec = torch.empty((b, A, C + 5), dtype=torch.float32, device=dev)
        ws = torch.empty((max(lib.ssd_encode_labels_ws_bytes_ex(ntot, b, m) for m in (0, 1)),), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def call(m):
            check(lib.ssd_encode_labels_resident_ex(b'vgg300', C, 0, d_gt.data_ptr(), d_cls.data_ptr(), d_off.data_ptr(), b, ntot,
                                                    vec.data_ptr(), ws.data_ptr(), stream, m, None))

        def timed(m):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(m)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        positives = {}
        for name, m in su.MATCH_RULES.items():
            for _ in range(3):
                timed(m)
            positives[name] = int((vec[:, :, C] == 0).sum())
        per = {name: [] for name in su.MATCH_RULES}
        for _ in range(args.rounds):
            for name, m in su.MATCH_RULES.items():
                per[name].append(float(np.median([timed(m) for _ in range(args.reps)])))
        say('# ---- %s: %d boxes' % (title, ntot))
        med = {}
        for name in su.MATCH_RULES:
            t = per[name]
            med[name] = float(np.median(t))
            say('  %-10s %9.4f ms  (%.4f ... %.4f)   %7d positive anchors' % (name, med[name], min(t), max(t), positives[name]))
        say('  paper / reference %.2f   paper / bf16 step %.4f' % (med['paper'] / med['reference'], med['paper'] / STEP_MS[0]))
        worst = max(worst, med['paper'])
    say('# The encode runs on the feeder\'s stream beside the step.  Slowest paper encode above: %.4f ms = %.1f %% of the shortest bf16 step: it %s.'
        % (worst, 100 * worst / STEP_MS[0], 'still hides behind a step' if worst < STEP_MS[0] else 'does NOT hide behind a step'))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
