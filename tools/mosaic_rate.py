#!/usr/bin/env python3
"""What the cells entry of the augmentation costs.  HIP events around `--calls` back-to-back calls per leg, the legs
interleaved in `--rounds` rounds of one process, vgg300 at batch 32, on the source pictures of tools/feeder_rate.py (the 500 x 375
fixture picture, shifted by a different offset each), already in HBM:

  (a) ssd_augment_batch_dev                                  32 pictures through the train recipe: the yardstick
  (b) ssd_augment_cells_dev, 32 whole-sample cells           the same 32 parameter structs: the same work through the other entry
  (c) ssd_augment_cells_dev, 128 cells, four per sample      32 mosaics: 128 pictures through the cell recipe into quarter-ish cells

A leg "separates" from (a) when its rounds' range and (a)'s do not overlap.

    python tools/mosaic_rate.py [--rounds 5] [--calls 50] [--out profiles/mosaic_rate.txt]
"""
import argparse
import ctypes as C
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, W, H = 32, 300, 300


def sources(n):
    from ssd_tensorflow_amd import jpeg
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'j1_jpeg.npz')) as g:
        bgr = jpeg.decode(g['voc_000232_jpg'].tobytes())
    big = np.pad(bgr, ((0, 32), (0, 32), (0, 0)), mode='reflect')
    return [np.ascontiguousarray(big[(i // 32) % 32:(i // 32) % 32 + 375, i % 32:i % 32 + 500]) for i in range(n)]


def record(i):
    from ssd_tensorflow_amd.utils import Box, Point, Size, Sample
    x0, y0 = 20 + i % 60, 30 + i % 40
    boxes = [Box('dog', 11, Point((x0 + 110) / 500, (y0 + 130) / 375), Size(220 / 500, 260 / 375)),
             Box('person', 14, Point(380 / 500, 185 / 375), Size(160 / 500, 290 / 375))]
    return Sample('im', boxes, Size(500, 375))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mosaic_rate.txt'))
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd import transforms as T
    from ssd_tensorflow_amd._lib import lib, check
    from ssd_tensorflow_amd.ssdutils import get_preset_by_name
    preset = get_preset_by_name('vgg300')
    pics = sources(4 * B)
    tfs = [t for t in T.build_train_transforms(preset, 20, 50, 0.5) if not isinstance(t, T.LabelCreatorTransform)]
    cell_tfs, resize = T.mosaic_cell_transforms(tfs)

    def run(tf_list, i, seed):
        tf_list[0].images = {'im': pics[i]}
        random.seed(seed)
        args_ = (None, None, record(i))
        for t in tf_list:
            args_ = t(*args_)
        return args_

    whole = [run(tfs, i, 100 + i)[0] for i in range(B)]
    quads, cells, fell = [], [], 0
    for s in range(B):
        _, centre = T.mosaic_draw(1000 + s, 1.0, 4 * B, W, H)
        for c, cell in enumerate(T.mosaic_layout(centre[0], centre[1], W, H)):
            a = run(cell_tfs, 4 * s + c, 5000 + 4 * s + c)
            data, _, _, f = T.mosaic_cell_resize(resize, a[0], a[1], a[2], cell[2], cell[3])
            quads.append(data); cells.append((s,) + cell); fell += f
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    legs = {}

    def leg(name, plans, cell_rows):
        cnp = None if cell_rows is None else np.ascontiguousarray(np.array(cell_rows, np.int32))
        arr, packed = T.plan_params(plans, W, H, cells=cnp)
        images = torch.from_numpy(packed).to(dev)
        n = len(plans)
        ws = torch.empty((lib.ssd_augment_ws_bytes(n, W, H) if cnp is None else lib.ssd_augment_cells_ws_bytes(n, W, H),), dtype=torch.uint8, device=dev)
        if cnp is None:
            call = lambda: check(lib.ssd_augment_batch_dev(images.data_ptr(), C.cast(arr, C.c_void_p), n, W, H, out.data_ptr(), ws.data_ptr(), stream))
        else:
            call = lambda: check(lib.ssd_augment_cells_dev(images.data_ptr(), C.cast(arr, C.c_void_p), C.c_void_p(cnp.ctypes.data), n, B, W, H,
                                                           out.data_ptr(), ws.data_ptr(), stream))
        legs[name] = (call, (arr, images, ws, cnp), int(packed.nbytes))

    leg('(a) ssd_augment_batch_dev, 32 pictures', whole, None)
    leg('(b) ssd_augment_cells_dev, 32 whole-sample cells', whole, [(i, 0, 0, W, H) for i in range(B)])
    leg('(c) ssd_augment_cells_dev, 128 cells', quads, cells)
    results = {}
    for name, (call, _, _) in legs.items():          # the same work must give the same batch, and everything is warm afterwards
        call(); call()
        torch.cuda.synchronize()
        results[name] = out.clone()
    names = list(legs)
    same = bool(torch.equal(results[names[0]], results[names[1]]))
    times = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, (call, _, _) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                call()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.calls * 1e3)
    lines = ['augmentation entries: one batch of %d samples of %d x %d from 500 x 375 sources in HBM, %s, torch %s' % (
                 B, W, H, torch.cuda.get_device_name(0), torch.__version__),
             'HIP events around %d back-to-back calls (parameter copies, taps, photometric pre-pass, gather), %d interleaved rounds in one process' % (
                 args.calls, args.rounds),
             'us per call: median (min .. max); output %.1f MB per call' % (B * W * H * 12 / 1e6), '']
    base = times[names[0]]
    for name in names:
        t = times[name]
        note = ''
        if name != names[0]:
            apart = max(t) < min(base) or min(t) > max(base)
            note = '   %.3f x (a); the rounds %s from (a)' % (statistics.median(t) / statistics.median(base), 'separate' if apart else 'do NOT separate')
        lines.append('%-52s %8.1f (%.1f .. %.1f)   %6.1f MB of sources%s' % (name, statistics.median(t), min(t), max(t), legs[name][2] / 1e6, note))
    lines += ['', '(b) writes the batch of (a) bit for bit: %s' % same,
              '(c): %d of 128 cells drew INTER_AREA onto a cell more than 14x smaller than their frame and run INTER_LINEAR' % fell]
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
