#!/usr/bin/env python3
"""Cost of the evaluation loop around the network: the same detection passes evaluated with the detections in host
lists (--ap-on host: ticket.get(), boxes_from_detection, APCalculator.add_detections) and in the device accumulator (--ap-on gpu:
DeviceAPCalculator.add_pass), in ONE process, interleaved rounds, wall clock.  Trains the shapes detector once with the product's
own driver (the schedule of tools/fp8_accuracy.py), then evaluates its held-out images at threshold 0.01 on two bf16 handles: one
with random weights, which gives many detections per image (the cap is 200), and the trained detector, whose detections are few.  Per round and leg: wall time per image from the first launch to the collected AP state
(host: the last add_detections has returned; gpu: num_detections() has waited for the last append), and the time of
compute_aps().  `net only` is the same loop without any AP bookkeeping (launch, then wait for the GPU).  Then the detector's mAP
under the three protocols, without flags and with the small objects flagged as difficult.

    python tools/eval_rate.py [--epochs 40] [--checkpoint final.npz] [--rounds 5] [--repeat 4] [--out profiles/eval_rate.txt]
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
    ap.add_argument('--checkpoint', default='', help='evaluate this checkpoint instead of training one')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--repeat', type=int, default=4, help='the held-out set is evaluated this many times per timed interval')
    ap.add_argument('--threshold', type=float, default=0.01)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd import train
    from ssd_tensorflow_amd.average_precision import APCalculator, DeviceAPCalculator, APs2mAP
    from ssd_tensorflow_amd.ssdutils import boxes_from_detection
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.training_data import TrainingData
    from ssd_tensorflow_amd.utils import FlaggedBox
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
                                 '--dtype', 'bf16', '--augment', 'false'])
            assert rc == 0, 'training failed'
            ckpt = os.path.join(run, 'final.npz')
            say('# tools/eval_rate.py: %s; shapes detector, vgg300, bf16, %d steps at batch 32, trained in %.0f s'
                % (torch.cuda.get_device_name(0), args.epochs * 32, time.perf_counter() - t0))
        else:
            say('# tools/eval_rate.py: %s; checkpoint %s' % (torch.cuda.get_device_name(0), os.path.basename(ckpt)))
        td = TrainingData('shapes', 'vgg300', num_train=1024, num_valid=128, augment=False, device=0)
        held = [(x.clone(), gts) for x, _, gts in td.valid_generator(32, 0)]
        n_img = sum(len(g) for _, g in held) * args.repeat
        thr = args.threshold
        with Session(0) as sess:
            trained = SSDVGG(sess, 'vgg300')
            trained.build_from_metagraph(None, ckpt, max_batch=32, dtype='bf16')
            ncls = td.num_classes
            random_net = SSDVGG(sess, 'vgg300')
            random_net.build_from_vgg(None, ncls, max_batch=32, training=False, dtype='bf16')
            net = trained

            def passes():
                for _ in range(args.repeat):
                    yield from held

            def leg_net():
                t0 = time.perf_counter()
                for x, gts in passes():
                    net.infer_dev(x)
                    net.detect_last_launch(len(gts), thr, 200, None)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, 0.0, None, 0

            def leg_host(protocol='reference', flag=None):
                calc = APCalculator(protocol=protocol)
                n = 0

                def collect(p):
                    nonlocal n
                    for gt, det in zip(p[1], p[0].get()):
                        boxes = boxes_from_detection(det, td.lid2name)
                        n += len(boxes)
                        calc.add_detections(flag(gt) if flag else gt, boxes)
                t0 = time.perf_counter()
                pending = None
                for x, gts in passes():
                    net.infer_dev(x)
                    ticket = net.detect_last_launch(len(gts), thr, 200, None)
                    if pending:
                        collect(pending)
                    pending = (ticket, gts)
                collect(pending)
                t1 = time.perf_counter()
                aps = calc.compute_aps()
                return t1 - t0, time.perf_counter() - t1, aps, n

            def leg_gpu(protocol='reference', flag=None):
                calc = DeviceAPCalculator(0, ncls, protocol)
                t0 = time.perf_counter()
                for x, gts in passes():
                    net.infer_dev(x)
                    ticket = net.detect_last_launch(len(gts), thr, 200, None)
                    calc.add_pass(ticket, [flag(gt) for gt in gts] if flag else gts)
                n = calc.num_detections()
                t1 = time.perf_counter()
                aps = calc.compute_aps()
                t2 = time.perf_counter()
                calc.close()
                return t1 - t0, t2 - t1, aps, n

            legs = [('net only', leg_net), ('--ap-on host', leg_host), ('--ap-on gpu', leg_gpu)]
            for net, title in ((random_net, 'random weights (Xavier, seed 42): many low-confidence detections per image (the cap is 200)'),
                               (trained, 'the trained shapes detector: few, confident detections')):
                say('# ---- %s' % title)
                for _, f in legs:       # warm-up: buffers, slots, the first launches
                    f()
                loop = {name: [] for name, _ in legs}
                comp = {name: [] for name, _ in legs}
                res = {}
                for _ in range(args.rounds):
                    for name, f in legs:
                        a, b, aps, n = f()
                        loop[name].append(a * 1e3 / n_img)
                        comp[name].append(b * 1e3)
                        res[name] = (aps, n)
                same = list(res['--ap-on host'][0].items()) == list(res['--ap-on gpu'][0].items()) and res['--ap-on host'][1] == res['--ap-on gpu'][1]
                say('# %d images per interval (%d held-out images x %d) at batch 32, threshold %.2f, %d detections (%.1f per image); wall clock, '
                    '%d interleaved rounds: median (min ... max)' % (n_img, n_img // args.repeat, args.repeat, thr, res['--ap-on host'][1],
                                                                   res['--ap-on host'][1] / n_img, args.rounds))
                say('# launch to collected AP state, ms per image')
                for name, _ in legs:
                    t = loop[name]
                    say('  %-14s %8.4f  (%.4f ... %.4f)' % (name, float(np.median(t)), min(t), max(t)))
                say('# compute_aps(), ms per call (%d detections, %d samples)' % (res['--ap-on host'][1], n_img))
                for name, _ in legs[1:]:
                    t = comp[name]
                    say('  %-14s %8.3f  (%.3f ... %.3f)' % (name, float(np.median(t)), min(t), max(t)))
                h, g = loop['--ap-on host'], loop['--ap-on gpu']
                say('# the two dicts and detection totals are %s; every round separates the two loops: %s (slowest gpu round %.4f, fastest host round %.4f)'
                    % ('identical' if same else 'DIFFERENT', 'yes, gpu below host' if max(g) < min(h) else ('yes, host below gpu' if max(h) < min(g) else 'no'), max(g), min(h)))
                net_t = float(np.median(loop['net only']))
                say('# bookkeeping beside the network: host %.4f ms per image, gpu %.4f ms per image' % (float(np.median(h)) - net_t, float(np.median(g)) - net_t))

            net = trained
            # ---- what the protocols do to the detector's mAP (one evaluation of the held-out set each, on the GPU path) ----
            args.repeat = 1
            sizes = sorted(b.size.w * b.size.h for _, gts in held for gt in gts for b in gt)
            small = sizes[len(sizes) // 5]       # the smallest fifth of the objects

            def flag_small(gt):
                return [FlaggedBox(*b, difficult=b.size.w * b.size.h < small) for b in gt]
            n_flag = sum(1 for v in sizes if v < small)
            say('# mAP of the shapes detector on the held-out images, threshold %.2f (host lists = accumulator for every row)' % thr)
            for title, flag in (('no flagged objects', None), ('the %d smallest of %d objects flagged difficult' % (n_flag, len(sizes)), flag_small)):
                row = []
                for protocol in ('reference', 'voc07', 'voc12'):
                    _, _, aps_h, _ = leg_host(protocol, flag)
                    _, _, aps_g, _ = leg_gpu(protocol, flag)
                    assert list(aps_h.items()) == list(aps_g.items()), (title, protocol)
                    row.append('%s %.4f' % (protocol, APs2mAP(aps_g)))
                say('  %-52s %s' % (title, '   '.join(row)))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
