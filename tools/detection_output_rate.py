#!/usr/bin/env python3
"""Cost of DetectionOutput beside the reference decode and beside the network: detect_last_launch(decode='argmax')
and detect_last_launch(decode='all') on RESIDENT results of one bf16 handle, HIP events around the decode pass alone, in ONE
process, interleaved rounds; the network pass of the same handle and batch (bf16) is timed the same way.  vgg300 at batches 32 and
128, threshold 0.01:
  (a) Xavier weights with 20 and 80 classes: nearly every (anchor, class) pair is a candidate, every class takes the select path;
  (b) the trained shapes detector (trained here with the product's own driver, the schedule of tools/eval_rate.py): few candidates.
Then the shapes detector's held-out mAP at threshold 0.01 under both decodes.

    python tools/detection_output_rate.py [--epochs 40] [--checkpoint final.npz] [--rounds 5] [--reps 20] [--out profiles/detection_output_rate.txt]
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
    ap.add_argument('--checkpoint', default='', help='use this shapes checkpoint instead of training one')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20, help='timed passes per leg and round (their median is the round\'s figure)')
    ap.add_argument('--threshold', type=float, default=0.01)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd import train
    from ssd_tensorflow_amd.average_precision import DeviceAPCalculator, APs2mAP
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.training_data import TrainingData
    lines = []
    thr = args.threshold

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        """GPU time of what fn enqueues on the handle's stream (the default stream), ms"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(net, x, title):
        b = x.shape[0]
        net.infer_dev(x)
        torch.cuda.synchronize()
        legs = [('decode argmax', lambda: net.detect_last_launch(b, thr, None, 200)),
                ('decode all', lambda: net.detect_last_launch(b, thr, decode='all')),
                ('network pass', lambda: net.infer_dev(x))]       # (last: it rewrites the result with the same values)
        for _, f in legs:
            for _ in range(3):
                timed(f)
        per = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, f in legs:
                per[name].append(float(np.median([timed(f) for _ in range(args.reps)])))
        n_arg = sum(len(d['conf']) for d in net.detect_last(b, thr, None, 200))
        n_all = sum(len(d['conf']) for d in net.detect_last(b, thr, decode='all'))
        say('# ---- %s, batch %d: %d detections (argmax), %d (all)' % (title, b, n_arg, n_all))
        for name, _ in legs:
            t = per[name]
            say('  %-14s %9.4f ms  (%.4f ... %.4f)   %.5f ms per image' % (name, float(np.median(t)), min(t), max(t), float(np.median(t)) / b))
        m = {name: float(np.median(per[name])) for name, _ in legs}
        say('  all / argmax %.2f   all / network pass %.3f   argmax / network pass %.4f' % (m['decode all'] / m['decode argmax'],
                                                                                           m['decode all'] / m['network pass'],
                                                                                           m['decode argmax'] / m['network pass']))

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
            say('# tools/detection_output_rate.py: %s; shapes detector, vgg300, bf16, %d steps at batch 32, trained in %.0f s'
                % (torch.cuda.get_device_name(0), args.epochs * 32, time.perf_counter() - t0))
        else:
            say('# tools/detection_output_rate.py: %s; checkpoint %s' % (torch.cuda.get_device_name(0), os.path.basename(ckpt)))
        say('# HIP events around the pass alone, results resident; threshold %.2f, nms_top_k 400, keep_top_k 200; %d interleaved rounds of %d '
            'passes per leg: median of the rounds\' medians (min ... max)' % (thr, args.rounds, args.reps))
        td = TrainingData('shapes', 'vgg300', num_train=1024, num_valid=128, augment=False, device=0)
        held = [(x.clone(), gts) for x, _, gts in td.valid_generator(32, 0)]
        rng = np.random.default_rng(5)
        with Session(0) as sess:
            for ncls in (20, 80):
                net = SSDVGG(sess, 'vgg300')
                net.build_from_vgg(None, ncls, max_batch=128, training=False, dtype='bf16')
                for b in (32, 128):
                    x = torch.from_numpy(rng.integers(0, 256, (b, 300, 300, 3)).astype(np.float32)).cuda()
                    measure(net, x, '(a) Xavier weights (seed 42), %d classes' % ncls)
                net.close()
            trained = SSDVGG(sess, 'vgg300')
            trained.build_from_metagraph(None, ckpt, max_batch=128, dtype='bf16')
            images = torch.cat([x for x, _ in held], 0)
            for b in (32, 128):
                measure(trained, images[:b].contiguous(), '(b) the trained shapes detector, %d classes' % td.num_classes)
            # ---- the detector's held-out mAP under both decodes (the device accumulator) ----
            say('# mAP of the shapes detector on its %d held-out images, threshold %.2f' % (sum(len(g) for _, g in held), thr))
            for name, kw in (('decode argmax', dict(detections_cap=None, max_out=200)), ('decode all', dict(decode='all'))):
                calc = DeviceAPCalculator(0, td.num_classes)
                for x, gts in held:
                    trained.infer_dev(x)
                    calc.add_pass(trained.detect_last_launch(len(gts), thr, **kw), gts)
                n = calc.num_detections()
                say('  %-14s mAP %.4f   (%d detections)' % (name, APs2mAP(calc.compute_aps()), n))
                calc.close()
            trained.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
