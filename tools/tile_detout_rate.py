#!/usr/bin/env python3
"""Cost of tiled detection with the DetectionOutput decode beside the argmax tile path, the untiled DetectionOutput
and the network, in ONE process with HIP events, interleaved rounds.  8 pictures x 20 tiles (1500 x 1200 at tile 400, overlap 0.25,
no whole view) = 160 network inputs of one bf16 handle, whose RESIDENT result every leg decodes; threshold 0.01:
  (a) the new path: ssd_detout_tiles_add_dev (the tile stage) + ssd_detout_tiles_merge_dev (class merge + picture merge), also
      timed apart;
  (b) the parent's path, the yardstick: ssd_decode_nms_dev(nms = 0, tile_cap 200) + ssd_merge_tiles_dev;
  (c) the untiled ssd_detection_output_dev on the same 160 inputs;
  the network pass of those inputs (bf16).
Weights: Xavier with 20 and 80 classes (nearly every (anchor, class) pair is a candidate), and the trained shapes detector (trained
here with the product's own driver, the schedule of tools/eval_rate.py; its held-out pictures are the tiles: few candidates).

    python tools/tile_detout_rate.py [--epochs 40] [--checkpoint final.npz] [--rounds 5] [--reps 10] [--out profiles/tile_detout_rate.txt]
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

PICTURES, CAP, K, KEEP, MARGIN = 8, 200, 400, 200, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--checkpoint', default='', help='use this shapes checkpoint instead of training one')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10, help='timed passes per leg and round (their median is the round\'s figure)')
    ap.add_argument('--threshold', type=float, default=0.01)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd import tiling, train
    from ssd_tensorflow_amd._lib import lib, check
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.training_data import TrainingData
    lines = []
    thr = args.threshold
    dev = torch.device('cuda', 0)
    windows = tiling.plan_tiles(1500, 1200, 400, 0.25, whole=False)
    tiles = [(i, t, (1500, 1200)) for i in range(PICTURES) for t in windows]
    n = len(tiles)
    assert n == 160
    structs = tiling.tile_structs(tiles)
    sp = C.cast(structs, C.c_void_p)
    A = 8732
    anchors = torch.empty((A, 4), dtype=torch.float64, device=dev)
    check(lib.ssd_anchors_dev(b'vgg300', anchors.data_ptr(), None, None))
    i32 = dict(dtype=torch.int32, device=dev)

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

    def measure(net, x, title):
        ncls = net.num_vars - 5
        net.infer_dev(x)
        result = C.c_void_p()
        check(lib.ssd_result_dev(net._h, C.byref(result)))
        torch.cuda.synchronize()
        wsb = int(lib.ssd_detout_tiles_ws_bytes(b'vgg300', ncls, n, PICTURES, K))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        dws = torch.empty(int(lib.ssd_decode_nms_ws_bytes(b'vgg300', n)), dtype=torch.uint8, device=dev)
        mws = torch.empty(int(lib.ssd_merge_tiles_ws_bytes(n, CAP)), dtype=torch.uint8, device=dev)
        uwb = int(lib.ssd_detection_output_ws_bytes(b'vgg300', ncls, n, K))
        uws = torch.empty(uwb, dtype=torch.uint8, device=dev)
        L = dict(count=torch.zeros(n, **i32), conf=torch.zeros((n, CAP), device=dev), cls=torch.zeros((n, CAP), **i32),
                 idx=torch.zeros((n, CAP), **i32), box=torch.zeros((n, CAP, 4), **i32))
        U = dict(count=torch.zeros(n, **i32), conf=torch.zeros((n, KEEP), device=dev), cls=torch.zeros((n, KEEP), **i32),
                 idx=torch.zeros((n, KEEP), **i32), box=torch.zeros((n, KEEP, 4), **i32))

        def outputs():
            return dict(count=torch.zeros(PICTURES, **i32), conf=torch.zeros((PICTURES, KEEP), device=dev), cls=torch.zeros((PICTURES, KEEP), **i32),
                        idx=torch.zeros((PICTURES, KEEP), **i32), tile=torch.zeros((PICTURES, KEEP), **i32),
                        box=torch.zeros((PICTURES, KEEP, 4), **i32))
        Ma, Mb = outputs(), outputs()

        def add():
            check(lib.ssd_detout_tiles_add_dev(b'vgg300', ncls, anchors.data_ptr(), result.value, sp, n, 0, n, thr, K, MARGIN, ws.data_ptr(), wsb,
                                               None))

        def merge_all():
            check(lib.ssd_detout_tiles_merge_dev(ncls, sp, n, PICTURES, K, KEEP, KEEP, Ma['count'].data_ptr(), Ma['conf'].data_ptr(),
                                                 Ma['cls'].data_ptr(), Ma['idx'].data_ptr(), Ma['tile'].data_ptr(), Ma['box'].data_ptr(),
                                                 ws.data_ptr(), wsb, None))

        def decode_argmax():
            check(lib.ssd_decode_nms_dev(b'vgg300', ncls, anchors.data_ptr(), result.value, n, thr, CAP, -1, CAP, 0, L['count'].data_ptr(),
                                         L['conf'].data_ptr(), L['cls'].data_ptr(), L['idx'].data_ptr(), L['box'].data_ptr(), dws.data_ptr(), None))

        def merge_argmax():
            check(lib.ssd_merge_tiles_dev(sp, n, PICTURES, CAP, L['count'].data_ptr(), L['conf'].data_ptr(), L['cls'].data_ptr(),
                                          L['idx'].data_ptr(), L['box'].data_ptr(), MARGIN, KEEP, KEEP, Mb['count'].data_ptr(), Mb['conf'].data_ptr(),
                                          Mb['cls'].data_ptr(), Mb['idx'].data_ptr(), Mb['tile'].data_ptr(), Mb['box'].data_ptr(), mws.data_ptr(),
                                          None))

        def untiled():
            check(lib.ssd_detection_output_dev(b'vgg300', ncls, anchors.data_ptr(), result.value, n, thr, K, KEEP, KEEP, U['count'].data_ptr(),
                                               U['conf'].data_ptr(), U['cls'].data_ptr(), U['idx'].data_ptr(), U['box'].data_ptr(), uws.data_ptr(),
                                               uwb, None))

        legs = [('(a) tile stage (add_dev)', add),
                ('(a) class + picture merge (merge_dev)', merge_all),
                ('(a) tile stage + merge', lambda: (add(), merge_all())),
                ('(b) argmax: decode(nms=0) + merge_tiles', lambda: (decode_argmax(), merge_argmax())),
                ('(c) untiled DetectionOutput, 160 inputs', untiled),
                ('network pass, 160 inputs (bf16)', lambda: net.infer_dev(x))]      # (last: it rewrites the result with the same values)
        for _, f in legs:
            for _ in range(2):
                timed(f)
        per = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, f in legs:
                per[name].append(float(np.median([timed(f) for _ in range(args.reps)])))
        torch.cuda.synchronize()
        say('# ---- %s: merged detections per picture %s (all), %s (argmax); tile-stage records %d of %d slots'
            % (title, ' '.join(str(int(v)) for v in Ma['count'].cpu()), ' '.join(str(int(v)) for v in Mb['count'].cpu()),
               int(ws[_count_off(n, PICTURES):_count_off(n, PICTURES) + 4 * n * ncls].view(torch.int32).clamp(0, K).sum()), n * ncls * K))
        med = {name: float(np.median(per[name])) for name, _ in legs}
        net_ms = med[legs[-1][0]]
        for name, _ in legs:
            t = per[name]
            say('  %-42s %9.4f ms  (%.4f ... %.4f)   %.3f of the network pass' % (name, med[name], min(t), max(t), med[name] / net_ms))
        a, b = per[legs[2][0]], per[legs[3][0]]
        apart = min(a) > max(b) or max(a) < min(b)
        say('  (a) / (b) = %.2f; the rounds %s (a) from (b); workspace %.1f MB' % (med[legs[2][0]] / med[legs[3][0]],
                                                                               'separate' if apart else 'do NOT separate', wsb / 1e6))

    def _count_off(n_tiles, n_images):
        return (4 * (8 * n_tiles + n_images + 1) + 255) // 256 * 256

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
            say('# tools/tile_detout_rate.py: %s; shapes detector, vgg300, bf16, %d steps at batch 32, trained in %.0f s'
                % (torch.cuda.get_device_name(0), args.epochs * 32, time.perf_counter() - t0))
        else:
            say('# tools/tile_detout_rate.py: %s; checkpoint %s' % (torch.cuda.get_device_name(0), os.path.basename(ckpt)))
        say('# HIP events around each leg alone, the 160 results resident; threshold %.2f, nms_top_k %d, keep_top_k %d, tile_cap %d, edge margin %d; '
            '%d interleaved rounds of %d passes per leg: median of the rounds\' medians (min ... max)' % (thr, K, KEEP, CAP, MARGIN, args.rounds, args.reps))
        td = TrainingData('shapes', 'vgg300', num_train=1024, num_valid=128, augment=False, device=0)
        held = torch.cat([x.clone() for x, _, _ in td.valid_generator(32, 0)], 0)
        rng = np.random.default_rng(5)
        with Session(0) as sess:
            x = torch.from_numpy(rng.integers(0, 256, (n, 300, 300, 3)).astype(np.float32)).cuda()
            for ncls in (20, 80):
                net = SSDVGG(sess, 'vgg300')
                net.build_from_vgg(None, ncls, max_batch=n, training=False, dtype='bf16')
                measure(net, x, 'Xavier weights (seed 42), %d classes' % ncls)
                net.close()
            trained = SSDVGG(sess, 'vgg300')
            trained.build_from_metagraph(None, ckpt, max_batch=n, dtype='bf16')
            measure(trained, torch.cat([held, held[:n - held.shape[0]]], 0).contiguous(), 'the trained shapes detector, %d classes' % td.num_classes)
            trained.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
