#!/usr/bin/env python3
"""Time of the cross-tile merge pass beside the existing untiled detect pass, in one process, with HIP events: five
interleaved rounds, medians with min ... max.  160 network inputs either way: 8 pictures x 20 tiles (1500 x 1200 at tile 400,
overlap 0.25, no whole view) at tile_cap 200 and threshold 0.01 -- the per-tile decode (ssd_decode_nms_dev, nms = 0) and the merge
(ssd_merge_tiles_dev) -- against ssd_decode_nms_dev with NMS on the same 160 predictions.  The predictions are synthetic: every
anchor speaks for one random class at confidence u^16 (u uniform: a quarter of the anchors pass 0.01), offsets N(0, 1).

    python tools/tile_rate.py [--out profiles/tile_detect_rate.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10, help='calls per timed interval')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd import tiling
    from ssd_tensorflow_amd._lib import lib, check
    dev = torch.device('cuda', 0)
    A, ncls, cap, thr, pictures = 8732, 20, 200, 0.01, 8
    windows = tiling.plan_tiles(1500, 1200, 400, 0.25, whole=False)
    tiles = [(i, t, (1500, 1200)) for i in range(pictures) for t in windows]
    n = len(tiles)
    assert n == 160
    g = torch.Generator(device=dev); g.manual_seed(7)
    pred = torch.zeros((n, A, ncls + 5), device=dev)
    conf = torch.rand((n, A), device=dev, generator=g) ** 16
    cls = torch.randint(0, ncls, (n, A), device=dev, generator=g)
    pred.scatter_(2, cls[:, :, None], conf[:, :, None])
    pred[:, :, ncls] = 1 - conf
    pred[:, :, ncls + 1:] = torch.randn((n, A, 4), device=dev, generator=g)
    anchors = torch.empty((A, 4), dtype=torch.float64, device=dev)
    check(lib.ssd_anchors_dev(b'vgg300', anchors.data_ptr(), None, None))
    dws = torch.empty(int(lib.ssd_decode_nms_ws_bytes(b'vgg300', n)), dtype=torch.uint8, device=dev)
    mws = torch.empty(int(lib.ssd_merge_tiles_ws_bytes(n, cap)), dtype=torch.uint8, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    L = dict(count=torch.zeros(n, **i32), conf=torch.zeros((n, cap), device=dev), cls=torch.zeros((n, cap), **i32),
             idx=torch.zeros((n, cap), **i32), box=torch.zeros((n, cap, 4), **i32))
    U = {k: torch.zeros_like(v) for k, v in L.items()}
    M = dict(count=torch.zeros(pictures, **i32), conf=torch.zeros((pictures, cap), device=dev), cls=torch.zeros((pictures, cap), **i32),
             idx=torch.zeros((pictures, cap), **i32), tile=torch.zeros((pictures, cap), **i32), box=torch.zeros((pictures, cap, 4), **i32))
    structs = tiling.tile_structs(tiles)

    def decode(out, nms):
        check(lib.ssd_decode_nms_dev(b'vgg300', ncls, anchors.data_ptr(), pred.data_ptr(), n, thr, cap, 200 if nms else -1, cap, nms,
                                     out['count'].data_ptr(), out['conf'].data_ptr(), out['cls'].data_ptr(), out['idx'].data_ptr(),
                                     out['box'].data_ptr(), dws.data_ptr(), None))

    def merge():
        check(lib.ssd_merge_tiles_dev(C.cast(structs, C.c_void_p), n, pictures, cap, L['count'].data_ptr(), L['conf'].data_ptr(),
                                      L['cls'].data_ptr(), L['idx'].data_ptr(), L['box'].data_ptr(), 2, 200, cap, M['count'].data_ptr(),
                                      M['conf'].data_ptr(), M['cls'].data_ptr(), M['idx'].data_ptr(), M['tile'].data_ptr(),
                                      M['box'].data_ptr(), mws.data_ptr(), None))

    legs = [('untiled detect (decode + NMS), 160 inputs', lambda: decode(U, 1)),
            ('tile decode (nms = 0), 160 tiles', lambda: decode(L, 0)),
            ('merge, 8 pictures x 20 tiles', merge)]
    for _, f in legs:
        f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, f in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000.0 / args.reps)
    lines = ['# tools/tile_rate.py: %s, HIP events, %d interleaved rounds of %d calls, us per call: median (min ... max)'
             % (torch.cuda.get_device_name(0), args.rounds, args.reps),
             '# vgg300, 20 classes, threshold %.2f, tile_cap %d; candidates per input: mean %.0f; records per tile after the cap: mean %.0f; '
             'merged detections per picture: %s' % (thr, cap, float((conf >= thr).sum()) / n, float(L['count'].clamp(max=cap).float().mean()),
                                                    ' '.join(str(int(v)) for v in M['count'].cpu()))]
    for name, _ in legs:
        t = times[name]
        lines.append('  %-44s %9.1f  (%.1f ... %.1f)' % (name, float(np.median(t)), min(t), max(t)))
    tiled = float(np.median(times[legs[1][0]])) + float(np.median(times[legs[2][0]]))
    lines.append('# tile decode + merge = %.1f us against %.1f us of the untiled pass on as many inputs' % (tiled, float(np.median(times[legs[0][0]]))))
    print('\n'.join(lines))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
