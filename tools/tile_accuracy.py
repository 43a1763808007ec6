#!/usr/bin/env python3
"""Detection accuracy of tiled detection.  Trains the shapes detector once with the product's own driver (the
schedule of tools/fp8_accuracy.py), pastes the 128 held-out 300 x 300 pictures into 4 x 4 mosaics of 1200 x 1200 (ground truth
shifted and scaled) and evaluates VOC07 mAP (threshold 0.5, NMS, 200 boxes) of the untiled pass -- the mosaic shrunk to 300 x 300
in one piece -- and of --tile 400 --tile-overlap 0.25 with and without the edge drop, on one f32 handle.  Next to the result:
what ONE missed object per class changes in mAP.  No number is fixed in advance.
--tile-decodes evaluates --tile under both tile decodes instead -- argmax (tile_cap 200, 200 boxes) and all (nms_top_k
400, keep_top_k 200) -- at thresholds 0.5 and 0.01, edge drop 2, with the whole view.

    python tools/tile_accuracy.py [--epochs 40] [--checkpoint final.npz] [--out profiles/tile_accuracy.txt]
    python tools/tile_accuracy.py --tile-decodes [--out profiles/tile_detout_accuracy.txt]
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

GRID = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--checkpoint', default='', help='evaluate this checkpoint instead of training one')
    ap.add_argument('--tile', type=int, default=400)
    ap.add_argument('--tile-overlap', type=float, default=0.25)
    ap.add_argument('--tile-decodes', action='store_true', help='compare the two tile decodes at thresholds 0.5 and 0.01')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from fp8_accuracy import one_miss_allowance
    from ssd_tensorflow_amd import train, tiling
    from ssd_tensorflow_amd import transforms as T
    from ssd_tensorflow_amd.annotate import pack_offsets
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
            say('# tools/tile_accuracy.py: shapes detector, vgg300, bf16, %d steps at batch 32, trained in %.0f s'
                % (args.epochs * 32, time.perf_counter() - t0))
        else:
            say('# tools/tile_accuracy.py: checkpoint %s' % os.path.basename(ckpt))
        td = TrainingData('shapes', 'vgg300', num_train=1024, num_valid=128, augment=False, device=0)
        pics, gts = [], []
        for x, _, g in td.valid_generator(32, 0):
            pics += list(x.clamp(0, 255).round().to(torch.uint8).cpu().numpy())
            gts += list(g)
        per = GRID * GRID
        side = pics[0].shape[0]
        mosaics, mgts, counts = [], [], {}
        for k in range(0, len(pics) - per + 1, per):
            m = np.zeros((GRID * side, GRID * side, 3), np.uint8)
            boxes = []
            for q in range(per):
                r, c = divmod(q, GRID)
                m[r * side:(r + 1) * side, c * side:(c + 1) * side] = pics[k + q]
                for b in gts[k + q]:
                    boxes.append(Box(b.label, b.labelid, Point((c + b.center.x) / GRID, (r + b.center.y) / GRID),
                                     Size(b.size.w / GRID, b.size.h / GRID)))
                    counts[b.label] = counts.get(b.label, 0) + 1
            mosaics.append(m); mgts.append(boxes)
        say('# held-out set: %d pictures of %d x %d pasted into %d mosaics of %d x %d, objects per class %s'
            % (len(mosaics) * per, side, side, len(mosaics), GRID * side, GRID * side, dict(sorted(counts.items()))))
        shapes = [(m.shape[0], m.shape[1]) for m in mosaics]
        offs, total = pack_offsets(shapes, 1)
        host = np.zeros(total, np.uint8)
        for o, m in zip(offs, mosaics):
            host[o:o + m.size] = m.reshape(-1)
        results = {}
        with Session(0) as sess:
            net = SSDVGG(sess, 'vgg300')
            net.build_from_metagraph(None, ckpt, max_batch=32, dtype='f32')
            packed = torch.from_numpy(host).to(torch.device('cuda', sess.device))

            def score(dets):
                calc, ndet = APCalculator(), 0
                for gt, det in zip(mgts, dets):
                    boxes = boxes_from_detection(det, td.lid2name)
                    ndet += len(boxes)
                    calc.add_detections(gt, boxes)
                aps = calc.compute_aps()
                return APs2mAP(aps), aps, ndet

            plans = []
            for o, s in zip(offs, shapes):
                plan = T.ImagePlan((packed, o, s))
                plan.resize = (side, side, T.INTER_LINEAR)
                plans.append(plan)
            net.infer_dev(T.augment_batch(plans, side, side, device=sess.device))
            results['untiled'] = score(net.detect_last_launch(len(plans), 0.5, 200, None).get())
            decodes = {}
            for thr in (0.5, 0.01) if args.tile_decodes else ():
                for decode in ('argmax', 'all'):
                    det = tiling.TiledDetector(net, args.tile, args.tile_overlap, True, 2, thr, 200, 200, decode=decode)
                    ticket = det.launch(packed, offs, shapes)
                    decodes['tile %d, threshold %.2f, tile decode %s' % (args.tile, thr, decode)] = score(ticket.get()) + (len(ticket.tiles) // len(mosaics),)
            for name, margin, whole in () if args.tile_decodes else (
                    ('tile %d, edge drop 2' % args.tile, 2, True), ('tile %d, no edge drop' % args.tile, -1, True),
                    ('tile %d, edge drop 2, no whole view' % args.tile, 2, False)):
                det = tiling.TiledDetector(net, args.tile, args.tile_overlap, whole, margin, 0.5, 200, 200)
                ticket = det.launch(packed, offs, shapes)
                results[name] = score(ticket.get()) + (len(ticket.tiles) // len(mosaics),)
            net.close()
        say('# VOC07 (11-point) AP on the mosaics, f32 handle, detections above 0.5 after NMS; --tile-overlap %.2f' % args.tile_overlap)
        for name, r in results.items():
            say('  %-36s mAP %.4f   %s   (%d detections%s)' % (name, r[0], '  '.join('%s %.4f' % (k, v) for k, v in sorted(r[1].items())), r[2],
                                                             ', %d tiles per mosaic' % r[3] if len(r) > 3 else ''))
        if decodes:
            say('# the two tile decodes (DESIGN.md 28): argmax = tile_cap 200, 200 boxes; all = nms_top_k 400, keep_top_k 200; edge drop 2, whole view')
            for name, r in decodes.items():
                say('  %-44s mAP %.4f   %s   (%d detections, %d tiles per mosaic)'
                    % (name, r[0], '  '.join('%s %.4f' % (k, v) for k, v in sorted(r[1].items())), r[2], r[3]))
            for thr in ('0.50', '0.01'):
                a, b = (decodes['tile %d, threshold %s, tile decode %s' % (args.tile, thr, d)][0] for d in ('all', 'argmax'))
                say('# threshold %s: all - argmax = %+.4f' % (thr, a - b))
            say('# VOC / COCO AP under the two tile decodes is NOT measured: there is no such data set here, only these mosaics of synthetic shapes')
        allow = one_miss_allowance(counts)
        base = results['untiled'][0]
        for name, r in results.items():
            if name != 'untiled':
                say('# %s - untiled = %+.4f' % (name, r[0] - base))
        say('# one missed object per class changes mAP by %.4f' % allow)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
