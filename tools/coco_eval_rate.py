#!/usr/bin/env python3
"""Cost of the COCO box evaluation on the GPU at val2017's scale: a seeded synthetic set -- 5 000 samples, 80
classes, 100 detections per image, about 7 ground-truth boxes per image, 1 % of them crowd -- in ONE accumulator, ONE process:

  (a) ssd_ap_compute_coco, ten thresholds: 60 (threshold, area, maxDet) combinations per class, one walk per class;
  (b) ssd_ap_compute, protocol voc12, the same ten thresholds: 10 walks per class, one per wave -- what the library could do
      before, and the yardstick;
  (c) the numpy oracle of tests/coco_ref.py on the host, once; (a)'s arrays must equal it.

(a) and (b) alternate over `--rounds` rounds behind a warm-up of each: wall clock around the call (it ends in a stream
synchronise and includes the ground truth's upload, the count pass's read-back and the allocations) and the count / sort / walk
stage times from HIP events (ssd_ap_kernel_times).  Reported: median (min ... max), and (a) / (b) per round.

    python tools/coco_eval_rate.py [--samples 5000] [--rounds 5] [--no-oracle] [--out profiles/coco_eval_rate.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def synthetic_set(rng, n_samples, ncls, dets_per_image, gts_per_image, crowd_rate):
    """arrays as ssd_coco_eval takes them; detections arrive image by image"""
    sizes = np.array([(640, 480), (480, 640), (640, 427), (500, 375), (640, 640)], np.float64)[rng.integers(0, 5, n_samples)]
    scale = sizes[:, 0] * sizes[:, 1] / 1e6
    n_gt_img = rng.poisson(gts_per_image, n_samples)
    gs = np.repeat(np.arange(n_samples), n_gt_img)
    ng = len(gs)
    area = 10.0 ** rng.uniform(1.5, 5.2, ng)                          # px^2, COCO-like: many small
    side = np.sqrt(area / scale[gs])
    w = np.clip((side * rng.uniform(0.6, 1.6, ng)).astype(np.int64), 2, 900)
    h = np.clip((side * side / w).astype(np.int64), 2, 900)
    x0 = (rng.random(ng) * (1000 - w)).astype(np.int64); y0 = (rng.random(ng) * (1000 - h)).astype(np.int64)
    gb = np.stack([x0, x0 + w, y0, y0 + h], 1).astype(np.float64)
    # a few classes per image, as in COCO: the classes of an image's boxes come from a small pool of its own
    pool = rng.integers(0, ncls, (n_samples, 3))
    gk = pool[gs, rng.integers(0, 3, ng)].astype(np.int32)
    crowd = rng.random(ng) < crowd_rate
    gf = np.where(crowd, 3, 0).astype(np.uint8)
    ga = (w * h * scale[gs] * rng.uniform(0.5, 1.0, ng)).astype(np.float64)
    first = np.concatenate(([0], np.cumsum(n_gt_img)))
    nd = n_samples * dets_per_image
    ds = np.repeat(np.arange(n_samples), dets_per_image).astype(np.int32)
    db = np.zeros((nd, 4), np.float64); dk = np.zeros(nd, np.int32)
    near = (rng.random(nd) < 0.5) & (n_gt_img[ds] > 0)
    pick = first[ds] + (rng.random(nd) * np.maximum(n_gt_img[ds], 1)).astype(np.int64)
    pick = np.minimum(pick, max(ng - 1, 0))
    jit = rng.integers(-1, 2, (nd, 4)) * (rng.random((nd, 4)) * 0.2 * (gb[pick, 1] - gb[pick, 0])[:, None]).astype(np.int64)
    db[near] = (gb[pick] + jit)[near]
    dk[near] = np.where(rng.random(nd) < 0.85, gk[pick], rng.integers(0, ncls, nd))[near]
    far = ~near
    fw = rng.integers(5, 400, nd); fh = rng.integers(5, 400, nd); fx = rng.integers(0, 600, nd); fy = rng.integers(0, 600, nd)
    db[far] = np.stack([fx, fx + fw, fy, fy + fh], 1)[far]
    dk[far] = rng.integers(0, ncls, nd)[far]
    conf = (rng.integers(1, 1000, nd) / 1000.0).astype(np.float32)
    return dict(det_box=np.ascontiguousarray(db, np.float32), det_conf=conf, det_cls=dk, det_sample=ds, gt_box=gb, gt_cls=gk,
                gt_sample=gs.astype(np.int32), gt_flags=gf, gt_area=ga, sample_scale=scale, ncls=ncls)


def spread(values, fmt='{:9.3f}'):
    v = sorted(values)
    return (fmt + '  (' + fmt.strip() + ' ... ' + fmt.strip() + ')').format(v[len(v) // 2], v[0], v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=5000)
    ap.add_argument('--classes', type=int, default=80)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--gts', type=float, default=7.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-oracle', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    import coco_ref as R
    from ssd_tensorflow_amd._lib import lib, check, np_ptr
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    s = synthetic_set(np.random.default_rng(2017), args.samples, args.classes, args.dets, args.gts, 0.01)
    ncls, thr = args.classes, np.ascontiguousarray(R.DEFAULT_THRESHOLDS)
    say('# tools/coco_eval_rate.py: %s; %d samples, %d classes, %d detections (%d per image), %d ground-truth boxes (%.2f per image), '
        '%d crowd; 10 thresholds' % (torch.cuda.get_device_name(0), args.samples, ncls, len(s['det_conf']), args.dets, len(s['gt_cls']),
                                     len(s['gt_cls']) / args.samples, int((s['gt_flags'] == 3).sum())))
    acc = C.c_void_p()
    check(lib.ssd_ap_create(0, ncls, C.byref(acc)))
    check(lib.ssd_ap_add_host_coco(acc, len(s['det_conf']), np_ptr(s['det_box']), np_ptr(s['det_conf']), np_ptr(s['det_cls']), np_ptr(s['det_sample']),
                                   args.samples, len(s['gt_cls']), np_ptr(s['gt_box']), np_ptr(s['gt_cls']), np_ptr(s['gt_sample']),
                                   np_ptr(s['gt_flags']), np_ptr(s['gt_area']), np_ptr(s['sample_scale'])))
    cap = np.full((4, 10, ncls), 7.0); car = np.full((6, 10, ncls), 7.0); cpresent = np.zeros((4, ncls), np.int32)
    vap = np.zeros((10, ncls)); vpresent = np.zeros(ncls, np.int32)
    n = C.c_longlong(); dropped = C.c_longlong()
    stages = np.zeros(3)

    def run_coco():
        check(lib.ssd_ap_compute_coco(acc, 10, np_ptr(thr), np_ptr(cap), np_ptr(car), np_ptr(cpresent), C.byref(n), C.byref(dropped)))

    def run_voc():
        check(lib.ssd_ap_compute(acc, 2, 10, np_ptr(thr), np_ptr(vap), np_ptr(vpresent), C.byref(n), C.byref(dropped)))

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        check(lib.ssd_ap_kernel_times(1, np_ptr(stages)))
        return [wall] + stages.tolist()

    check(lib.ssd_ap_kernel_times(1, None))
    run_coco(); run_voc()                                              # warm-up: code objects, allocator
    rows = {'coco': [], 'voc12': []}
    for _ in range(args.rounds):
        rows['coco'].append(timed(run_coco))
        rows['voc12'].append(timed(run_voc))
    check(lib.ssd_ap_kernel_times(0, None))
    assert n.value == len(s['det_conf']) and dropped.value == 0
    say('# %d interleaved rounds behind one warm-up of each; ms per call: median (min ... max)' % args.rounds)
    for name, label in (('coco', '(a) ssd_ap_compute_coco, 60 combinations per class'), ('voc12', '(b) ssd_ap_compute voc12, 10 walks per class')):
        r = np.array(rows[name])
        say('  ' + label)
        for i, what in enumerate(('wall clock around the call', 'count kernels (HIP events)', 'sort kernel  (HIP events)', 'walk kernel  (HIP events)')):
            say('    %-28s %s' % (what, spread(r[:, i].tolist())))
    ratio_wall = [a[0] / b[0] for a, b in zip(rows['coco'], rows['voc12'])]
    ratio_walk = [a[3] / b[3] for a, b in zip(rows['coco'], rows['voc12'])]
    say('# (a) / (b) per round, wall clock:  ' + '  '.join('%.2f' % v for v in ratio_wall))
    say('# (a) / (b) per round, walk kernel: ' + '  '.join('%.2f' % v for v in ratio_walk))
    say('# (a) evaluates 6 x the combinations of (b); (a) above 6 x (b) in every round: wall clock %s, walk kernel %s'
        % ('yes' if min(ratio_wall) > 6 else 'no', 'yes' if min(ratio_walk) > 6 else 'no'))
    if not args.no_oracle:
        t0 = time.perf_counter()
        want = R.evaluate_set(s, thr)
        wall = time.perf_counter() - t0
        same = all(np.array_equal(g, w) for g, w in zip((cap, car, cpresent), want))
        say('# (c) the numpy oracle on the host, once: %.1f s; (a) equals it bit for bit: %s' % (wall, 'yes' if same else 'NO'))
        summary = R.summarize(*want, thr)
        say('# the twelve numbers of the set: ' + '  '.join('%s %.4f' % kv for kv in summary.items()))
    else:
        say('# (c) the numpy oracle: not run')
    check(lib.ssd_ap_destroy(acc))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
