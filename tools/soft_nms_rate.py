#!/usr/bin/env python3
"""Cost of Soft-NMS in the DetectionOutput decode beside the hard rule: detect_last_launch(decode='all') with
soft_nms = None / 'linear' / 'gaussian' on RESIDENT results of one bf16 handle, HIP events around the pass alone, ONE process,
the three rules interleaved inside every round.  The yardstick is the hard pass of the same process.  The legs are those of
tools/detection_output_rate.py (vgg300, threshold 0.01, nms_top_k 400, keep_top_k 200):
  (a) Xavier weights with 20 and 80 classes at batches 32 and 128: nearly every (anchor, class) pair is a candidate;
  (b) the trained shapes detector (trained here, the schedule of tools/eval_rate.py): few candidates;
  (c) the tiled merge alone (ssd_detout_tiles_merge(_soft)_dev) of 8 pictures x 20 windows, 20 classes, on a workspace the tile
      stage filled from seeded softmax rows.

    python tools/soft_nms_rate.py [--epochs 40] [--checkpoint final.npz] [--rounds 5] [--reps 20] [--out profiles/soft_nms_rate.txt]
"""
import argparse
import contextlib
import ctypes as C
import io
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RULES = (('hard', None), ('linear', 'linear'), ('gaussian', 'gaussian'))


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
    from ssd_tensorflow_amd import train, tiling
    from ssd_tensorflow_amd import ssdutils as su
    from ssd_tensorflow_amd._lib import lib, check
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.training_data import TrainingData
    lines = []
    thr = args.threshold

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds(legs):
        """legs [(name, fn)] -> {name: [the median of every round]}, the legs interleaved inside a round"""
        for _, f in legs:
            for _ in range(3):
                timed(f)
        per = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, f in legs:
                per[name].append(float(np.median([timed(f) for _ in range(args.reps)])))
        return per

    def report(per, unit_count, unit):
        hard = per['hard']
        for name, _ in RULES:
            t = per[name]
            say('  %-9s %9.4f ms  (%.4f ... %.4f)   %.5f ms per %s' % (name, float(np.median(t)), min(t), max(t), float(np.median(t)) / unit_count, unit))
        for name in ('linear', 'gaussian'):
            t = per[name]
            apart = min(t) > max(hard) or max(t) < min(hard)
            say('  %s / hard %.2f   (the rounds %s: %s %.4f ... %.4f against hard %.4f ... %.4f)'
                % (name, float(np.median(t)) / float(np.median(hard)), 'separate them' if apart else 'do NOT separate them', name, min(t), max(t),
                   min(hard), max(hard)))

    def measure(net, x, title):
        b = x.shape[0]
        net.infer_dev(x)
        torch.cuda.synchronize()
        per = rounds([(name, (lambda kw=kw: net.detect_last_launch(b, thr, decode='all', soft_nms=kw))) for name, kw in RULES])
        counts = [sum(len(d['conf']) for d in net.detect_last(b, thr, decode='all', soft_nms=kw)) for _, kw in RULES]
        say('# ---- %s, batch %d: %d / %d / %d detections (hard / linear / gaussian)' % ((title, b) + tuple(counts)))
        report(per, b, 'image')

    def measure_tiled(n_pictures=8, n_windows=20, ncls=20, k=400, keep=200):
        pname = b'vgg300'
        A = 8732
        size = (1600, 1280)
        tiles = []
        for img in range(n_pictures):      # 5 x 4 windows of 400 with every inner edge interior
            for j in range(4):
                for i in range(5):
                    interior = (1 if i > 0 else 0) | (2 if i < 4 else 0) | (4 if j > 0 else 0) | (8 if j < 3 else 0)
                    tiles.append((img, tiling.Tile(300 * i, 293 * j, 400, 400, interior), size))
        n_tiles = len(tiles)
        assert n_tiles == n_pictures * n_windows
        dev = torch.device('cuda', 0)
        anc = torch.empty((A, 4), dtype=torch.float64, device=dev)
        check(lib.ssd_anchors_dev(pname, anc.data_ptr(), None, None))
        wsb = int(lib.ssd_detout_tiles_ws_bytes(pname, ncls, n_tiles, n_pictures, k))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        structs = C.cast(tiling.tile_structs(tiles), C.c_void_p)
        gen = torch.Generator(device=dev)
        gen.manual_seed(38)
        for first in range(0, n_tiles, 32):      # the tile stage, once: softmax rows, offsets N(0, 1)
            b = min(32, n_tiles - first)
            pred = torch.empty((b, A, ncls + 5), dtype=torch.float32, device=dev)
            pred[..., :ncls + 1] = torch.softmax(torch.randn((b, A, ncls + 1), generator=gen, device=dev), -1)
            pred[..., ncls + 1:] = torch.randn((b, A, 4), generator=gen, device=dev)
            check(lib.ssd_detout_tiles_add_dev(pname, ncls, anc.data_ptr(), pred.data_ptr(), structs, n_tiles, first, b, thr, k, 2, ws.data_ptr(), wsb,
                                               None))
        torch.cuda.synchronize()
        o = [torch.zeros(n_pictures, dtype=torch.int32, device=dev), torch.zeros((n_pictures, keep), dtype=torch.float32, device=dev)]
        o += [torch.zeros((n_pictures, keep), dtype=torch.int32, device=dev) for _ in range(3)]
        o.append(torch.zeros((n_pictures, keep, 4), dtype=torch.int32, device=dev))
        ptrs = [t.data_ptr() for t in o]

        def merge(kw):
            if kw is None:
                check(lib.ssd_detout_tiles_merge_dev(ncls, structs, n_tiles, n_pictures, k, keep, keep, *ptrs, ws.data_ptr(), wsb, None))
            else:
                nms = su.soft_nms_params(kw, thr=thr)
                check(lib.ssd_detout_tiles_merge_soft_dev(ncls, structs, n_tiles, n_pictures, k, keep, keep, *ptrs, ws.data_ptr(), wsb,
                                                          C.cast(C.pointer(nms), C.c_void_p), None))

        per = rounds([(name, (lambda kw=kw: merge(kw))) for name, kw in RULES])
        say('# ---- (c) the tiled merge alone: %d pictures x %d windows, %d classes, seeded softmax rows' % (n_pictures, n_windows, ncls))
        report(per, n_pictures, 'picture')

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
            say('# tools/soft_nms_rate.py: %s; shapes detector, vgg300, bf16, %d steps at batch 32, trained in %.0f s'
                % (torch.cuda.get_device_name(0), args.epochs * 32, time.perf_counter() - t0))
        else:
            say('# tools/soft_nms_rate.py: %s; checkpoint %s' % (torch.cuda.get_device_name(0), os.path.basename(ckpt)))
        say('# HIP events around the DetectionOutput pass alone, results resident; threshold %.2f, nms_top_k 400, keep_top_k 200, soft nms iou '
            '0.45, sigma 0.5, min score = the threshold; %d rounds, the three rules interleaved inside a round, %d passes per rule and round: '
            'median of the rounds\' medians (min ... max)' % (thr, args.rounds, args.reps))
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
            trained.close()
            measure_tiled()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
