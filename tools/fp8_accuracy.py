#!/usr/bin/env python3
"""Detection accuracy of the fp8 handle.  Trains the shapes detector once with the product's own driver (bf16,
the schedule of tests/test_gpu_learning.py: 40 epochs of 1024 images at batch 32), calibrates an fp8 handle on 32 training
images and evaluates VOC07 mAP (threshold 0.5, NMS, 200 boxes: what train.py's validation does) on the 128 held-out images with
an fp32, a bf16 and an fp8 handle built from the same checkpoint.  Next to the result: what ONE missed object per class changes
in mAP, from the held-out set's object counts -- the allowance for fp8 against bf16.

    python tools/fp8_accuracy.py [--epochs 40] [--checkpoint final.npz] [--out profiles/fp8_accuracy.txt]

--a-trous false trains and evaluates the fc graph; the fp8 handle is then built twice, under SSD_FP8_BIGK=0 (the 7x7
fc6 on the bf16 kernel) and under SSD_FP8_BIGK=1 (fc6 on e4m3), and the allowance is applied to the second.

    python tools/fp8_accuracy.py --a-trous false --out profiles/fp8_fc_accuracy.txt

--mxfp8 adds a fourth row (a-trous graph): the mxfp8 handle, which is not calibrated; the allowance is applied to it.

    python tools/fp8_accuracy.py --mxfp8 --out profiles/mxfp8_accuracy.txt

--a-trous false --mxfp8: the fc graph with the mxfp8 handle under SSD_MXFP8_BIGK=0 and, last, under SSD_MXFP8_BIGK=1 (fc6 on MX
operands); the allowance is applied to the last.

    python tools/fp8_accuracy.py --a-trous false --mxfp8 --out profiles/mxfp8_fc_accuracy.txt

--mxfp6 (a-trous graph): rows for fp32, bf16, fp8, mxfp8 and mxfp6, the allowance applied to mxfp6, and the distance of
every handle's result to the fp32 handle's on the fixture of DESIGN.md 18 (synthetic alive weights, two synthetic images).

    python tools/fp8_accuracy.py --mxfp6 --out profiles/mxfp6_accuracy.txt
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


def one_miss_allowance(counts):
    """11-point AP of a class with n objects, all found at precision 1, is 1; with one object missed the recall stops at
    (n - 1) / n and the points t > (n - 1) / n of {0, 0.1, ..., 1} fall to 0.  mAP changes by the mean over the classes."""
    drops = []
    for n in counts.values():
        top = (n - 1) / n
        drops.append(sum(1 for t in np.arange(0, 1.1, 0.1) if t > top + 1e-9) / 11.0)
    return float(np.mean(drops))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--checkpoint', default='', help='evaluate this checkpoint instead of training one')
    ap.add_argument('--calibrate-images', type=int, default=32)
    ap.add_argument('--a-trous', default='true', choices=['true', 'false'], help='false: the fc graph, fp8 under SSD_FP8_BIGK 0 and 1')
    ap.add_argument('--mxfp8', action='store_true', help='further rows: the mxfp8 handle (no calibration); fc graph: under SSD_MXFP8_BIGK 0 and 1')
    ap.add_argument('--mxfp6', action='store_true', help='a-trous graph: rows for fp8, mxfp8 and mxfp6, and the distance to fp32 on the synthetic fixture')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.mxfp6:
        if args.a_trous == 'false':
            ap.error('--mxfp6 evaluates the a-trous graph')
        args.mxfp8 = True
    fc = args.a_trous == 'false'
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
                                 '--dtype', 'bf16', '--augment', 'false', '--a-trous', args.a_trous])
            assert rc == 0, 'training failed'
            ckpt = os.path.join(run, 'final.npz')
            say('# tools/fp8_accuracy.py: shapes detector, vgg300%s, bf16, %d steps at batch 32, trained in %.0f s'
                % (' fc graph' if fc else '', args.epochs * 32, time.perf_counter() - t0))
        else:
            say('# tools/fp8_accuracy.py: checkpoint %s' % os.path.basename(ckpt))
        td = TrainingData('shapes', 'vgg300', num_train=1024, num_valid=128, augment=False, device=0)
        calib = next(iter(td.train_generator(args.calibrate_images, 0)))[0].clone()
        held = [(x.clone(), gts) for x, _, gts in td.valid_generator(32, 0)]
        counts = {}
        for _, gts in held:
            for gt in gts:
                for box in gt:
                    counts[box.label] = counts.get(box.label, 0) + 1
        say('# held-out set: %d images, objects per class %s' % (sum(len(g) for _, g in held), dict(sorted(counts.items()))))
        results = {}
        with Session(0) as sess:
            # (handle name, dtype, the switch set while the handle is created, its value)
            F8, MX = 'SSD_FP8_BIGK', 'SSD_MXFP8_BIGK'
            handles = [('f32', 'f32', None, None), ('bf16', 'bf16', None, None)]
            if fc and args.mxfp8:
                handles += [('fp8', 'fp8', F8, '1'), ('mxfp8/bigk0', 'mxfp8', MX, '0'), ('mxfp8/bigk1', 'mxfp8', MX, '1')]
            elif fc:
                handles += [('fp8/bigk0', 'fp8', F8, '0'), ('fp8/bigk1', 'fp8', F8, '1')]
            else:
                handles += [('fp8', 'fp8', None, None)] + ([('mxfp8', 'mxfp8', None, None)] if args.mxfp8 else []) + ([('mxfp6', 'mxfp6', None, None)] if args.mxfp6 else [])
            for name, dt, switch, bigk in handles:
                saved = os.environ.get(switch) if switch else None
                if switch:
                    os.environ[switch] = bigk
                try:
                    net = SSDVGG(sess, 'vgg300')
                    net.build_from_metagraph(None, ckpt, max_batch=32, dtype=dt)
                finally:
                    if switch:
                        os.environ.pop(switch)
                        if saved is not None:
                            os.environ[switch] = saved
                assert net.a_trous == (not fc)
                if dt == 'fp8':
                    net.calibrate_fp8(calib)
                    if fc:
                        say('# %s: e4m3 tensors %s' % (name, ' '.join(net.fp8_scales)))
                calc = APCalculator()
                ndet = 0
                for x, gts in held:
                    net.infer_dev(x)
                    for gt, det in zip(gts, net.detect_last_launch(len(gts), 0.5, 200, None).get()):
                        boxes = boxes_from_detection(det, td.lid2name)
                        ndet += len(boxes)
                        calc.add_detections(gt, boxes)
                aps = calc.compute_aps()
                results[name] = (APs2mAP(aps), aps, ndet)
                net.close()
        say('# VOC07 (11-point) AP on the held-out images, detections above 0.5 after NMS')
        for dt, (m, aps, ndet) in results.items():
            say(('  %-11s' if fc else '  %-5s') % dt + ' mAP %.4f   %s   (%d detections)' % (m, '  '.join('%s %.4f' % (k, v) for k, v in sorted(aps.items())), ndet))
        allow = one_miss_allowance(counts)
        last = handles[-1][0]
        diff = results['bf16'][0] - results[last][0]
        say('# one missed object per class changes mAP by %.4f; bf16 - %s = %+.4f: %s' % (allow, last, diff, 'within it' if diff <= allow else 'BELOW it'))
        if args.mxfp8:
            say('# bf16 - fp8 = %+.4f' % (results['bf16'][0] - results['fp8'][0]))
        if args.mxfp6:
            say('# bf16 - mxfp8 = %+.4f' % (results['bf16'][0] - results['mxfp8'][0]))
            # the fixture of DESIGN.md 18: weights init_params(seed 42, alive), images synth_images(default_rng(99), 2)
            from oracle import boxes as ob, ssdvgg_ref as ref
            preset = ob.get_preset('vgg300')
            w = ref.init_params(preset, 20, seed=42, alive=True)
            x = ref.synth_images(np.random.default_rng(99), 2, preset)
            res = {}
            with Session(0) as sess:
                for dt in ('f32', 'bf16', 'fp8', 'mxfp8', 'mxfp6'):
                    net = SSDVGG(sess, 'vgg300')
                    net.build_from_vgg(None, 20, max_batch=2, training=False, weights=w, dtype=dt)
                    if dt == 'fp8':
                        net.calibrate_fp8(x)
                    res[dt] = net.infer(x).astype(np.float64)
            dist = lambda a: float(np.linalg.norm(a - res['f32']) / np.linalg.norm(res['f32']))
            say('# synthetic fixture (alive weights seed 42, 2 images): |result - result fp32| / |result fp32|: '
                + ', '.join('%s %.4e' % (dt, dist(res[dt])) for dt in ('bf16', 'fp8', 'mxfp8', 'mxfp6')))
        say('# fp8 activation scales calibrated on the first %d training images' % args.calibrate_images + ('; mxfp8: nothing to calibrate' if args.mxfp8 else ''))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
