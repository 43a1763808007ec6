#!/usr/bin/env python3
"""GPU time of the two localization losses: smooth-L1, the default, against GIoU.  HIP events, ONE process,
interleaved rounds; the yardstick is the smooth-L1 path of the same process, not a number chosen in advance.
  op level, on resident head buffers (ssd_op_multibox_loss_ex2 / _grad_ex2): forward (the head kernel + the per-sample kernel) and
      gradient of both localization losses under mining and under focal, at vgg300 batch 32 and vgg512 batch 16, 20 and 80
      classes, fp32 gradient buffers, 30 positives per image;
  through the handle: ssd_train_step_dev at vgg300 batch 32, bf16 and fp32, mining, under both (learning rate 0: the weights stay).
A measurement, not a test.

    python tools/giou_rate.py [--rounds 5] [--reps 20] [--out profiles/giou_loss_rate.txt]
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
    ap.add_argument('--reps', type=int, default=20, help="timed calls per leg and round (their median is the round's figure)")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd import ssdutils as su
    from ssd_tensorflow_amd._lib import lib, check
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session, loss_config, loc_loss_config
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(7)
    confs = {'mining': loss_config('mining'), 'focal': loss_config('focal', 2.0, 0.25)}
    locs = {'smooth_l1': loc_loss_config('smooth_l1'), 'giou': loc_loss_config('giou', 1.0)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds_of(legs):
        """{name: [per-round medians]} of the legs run in turn, args.rounds times"""
        for fn in legs.values():
            for _ in range(3):
                timed(fn)
        per = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                per[k].append(float(np.median([timed(fn) for _ in range(args.reps)])))
        return per

    def row(name, t, extra=''):
        say('  %-32s %8.4f ms  (%.4f ... %.4f)%s' % (name, float(np.median(t)), min(t), max(t), extra))

    def separated(a, b):
        """do the rounds of two legs separate, and which way"""
        if max(a) < min(b):
            return 'every round of the first is below every round of the second'
        if max(b) < min(a):
            return 'every round of the second is below every round of the first'
        return 'the rounds overlap: not separated'

    say('# tools/giou_rate.py: %s; HIP events, one process, %d interleaved rounds of %d calls per leg: median of the rounds\' medians '
        '(min ... max); giou: weight 1; focal: gamma 2, alpha 0.25' % (torch.cuda.get_device_name(0), args.rounds, args.reps))
    say('# ---- op level, resident heads, fp32 gradient buffers, 30 positives per image')
    for pname, B in (('vgg300', 32), ('vgg512', 16)):
        preset = su.get_preset_by_name(pname)
        hw = [m.size[0] * m.size[1] for m in preset.maps]
        nj = [2 + len(m.aspect_ratios) for m in preset.maps]
        A = sum(h * j for h, j in zip(hw, nj))
        assert A == preset.num_anchors
        for nclass in (20, 80):
            nv, nc = nclass + 5, nclass + 1
            ld = [(j * nv + 7) // 8 * 8 for j in nj]
            hw_, nj_ = (C.c_int * len(hw))(*hw), (C.c_int * len(nj))(*nj)
            offs = (C.c_size_t * 6)()
            nbytes = lib.ssd_op_multibox_loss_ws_bytes(len(hw), hw_, nj_, B, offs, None)
            ws = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
            heads = [torch.randn((B * h, l), device=dev) * 3 for h, l in zip(hw, ld)]
            grads = [torch.zeros_like(h) for h in heads]
            y = np.zeros((B, A, nv), np.float32)
            y[:, :, nc - 1] = 1
            for b in range(B):
                idx = rng.choice(A, 30, replace=False)
                y[b, idx, nc - 1] = 0
                y[b, idx, rng.integers(0, nclass, 30)] = 1
                y[b, idx, nc:] = rng.normal(0, 1, (30, 4))
            labels = torch.from_numpy(y).to(dev)
            result = torch.empty_like(labels)
            hp = (C.c_void_p * len(heads))(*[t.data_ptr() for t in heads])
            gp = (C.c_void_p * len(grads))(*[t.data_ptr() for t in grads])

            def fwd(cfg, loc):
                check(lib.ssd_op_multibox_loss_ex2(len(hw), hw_, nj_, nclass, hp, labels.data_ptr(), result.data_ptr(), ws.data_ptr(), B, 0, B,
                                                   0.0, None, 0, 0.0, C.byref(cfg), C.byref(loc), None))

            def bwd(cfg, loc):
                check(lib.ssd_op_multibox_loss_grad_ex2(len(hw), hw_, nj_, nclass, gp, 0, labels.data_ptr(), result.data_ptr(), ws.data_ptr(),
                                                        B, 0, B, C.byref(cfg), C.byref(loc), None))

            say('# %s batch %d, %d classes: %d anchors' % (pname, B, nclass, A))
            for conf, cfg in confs.items():
                # a gradient call reads what ITS forward left: each forward leg is followed by its own gradient leg
                legs = {}
                for lname, loc in locs.items():
                    legs['%s %s forward' % (conf, lname)] = lambda cfg=cfg, loc=loc: fwd(cfg, loc)
                    legs['%s %s gradient' % (conf, lname)] = lambda cfg=cfg, loc=loc: bwd(cfg, loc)
                per = rounds_of(legs)
                for k in per:
                    row(k, per[k])
                for part in ('forward', 'gradient'):
                    a, g = per['%s smooth_l1 %s' % (conf, part)], per['%s giou %s' % (conf, part)]
                    say('  %s %-8s smooth_l1 | giou: %s (giou - smooth_l1 %+.4f ms)' % (conf, part, separated(a, g), float(np.median(g) - np.median(a))))

    say('# ---- through the handle: ssd_train_step_dev, vgg300 batch 32, 20 classes, mining, learning rate 0')
    B = 32
    preset = su.get_preset_by_name('vgg300')
    boxes, classes = [], []
    for _ in range(B):
        n = int(rng.integers(1, 9))
        w, h = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
        boxes.append(np.stack([rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2), w, h], 1))
        classes.append(rng.integers(0, 20, n).astype(np.int32))
    yt = torch.from_numpy(np.ascontiguousarray(su.encode_labels_batch(preset, 20, boxes, classes), np.float32)).to(dev)
    xt = torch.rand((B, 300, 300, 3), device=dev) * 255
    with Session(0) as sess:
        for dtype in ('bf16', 'f32'):
            net = SSDVGG(sess, 'vgg300')
            net.build_from_vgg(None, 20, max_batch=B, dtype=dtype)
            net.build_optimizer(learning_rate=0.0)

            def step(kind):
                net.set_loc_loss(kind, 1.0)
                net.train_step_dev(xt, yt)

            per = rounds_of({'smooth_l1': lambda: step('smooth_l1'), 'giou': lambda: step('giou')})
            say('# %s step' % dtype)
            for k in per:
                row(k, per[k], '   %.0f images/s' % (B / (np.median(per[k]) * 1e-3)))
            d = float(np.median(per['giou']) - np.median(per['smooth_l1']))
            say('  giou - smooth_l1 %+.4f ms (%+.2f %% of the smooth_l1 step); smooth_l1 | giou: %s'
                % (d, 100 * d / float(np.median(per['smooth_l1'])), separated(per['smooth_l1'], per['giou'])))
            net.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
