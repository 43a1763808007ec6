#!/usr/bin/env python3
"""GPU time of the two losses: hard-negative mining, the default, against the focal loss.  HIP events, ONE process,
interleaved rounds; the yardstick is the mining path of the same process, not a number chosen in advance.
  op level, on resident head buffers (ssd_op_multibox_loss_ex / _grad_ex): forward (heads_kernel<true> + the per-sample kernel) and
      gradient of both losses at vgg300 batch 32 and vgg512 batch 16, 20 and 80 classes, fp32 gradient buffers; for the dense
      focal gradient kernel also the bytes it moves over its time, beside the same figure of the forward call, whose
      heads_kernel<true> moves the same bytes (the forward's figure includes its per-sample kernel: a lower bound for the head
      kernel alone);
  through the handle: ssd_train_step_dev at vgg300 batch 32, bf16 and fp32, under both losses (learning rate 0: the weights stay).
A measurement, not a test.

    python tools/focal_rate.py [--rounds 5] [--reps 20] [--out profiles/focal_loss_rate.txt]
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
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session, loss_config
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(7)
    cfgs = {'mining': loss_config('mining'), 'focal': loss_config('focal', 2.0, 0.25)}

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
        say('  %-28s %8.4f ms  (%.4f ... %.4f)%s' % (name, float(np.median(t)), min(t), max(t), extra))

    def separated(a, b):
        """do the rounds of two legs separate, and which way"""
        if max(a) < min(b):
            return 'every round of the first is below every round of the second'
        if max(b) < min(a):
            return 'every round of the second is below every round of the first'
        return 'the rounds overlap: not separated'

    say('# tools/focal_rate.py: %s; HIP events, one process, %d interleaved rounds of %d calls per leg: median of the rounds\' medians '
        '(min ... max); focal: gamma 2, alpha 0.25' % (torch.cuda.get_device_name(0), args.rounds, args.reps))
    say('# ---- op level, resident heads, fp32 gradient buffers')
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

            def fwd(cfg):
                check(lib.ssd_op_multibox_loss_ex(len(hw), hw_, nj_, nclass, hp, labels.data_ptr(), result.data_ptr(), ws.data_ptr(), B, 0, B,
                                                  0.0, None, 0, 0.0, C.byref(cfg), None))

            def bwd(cfg):
                check(lib.ssd_op_multibox_loss_grad_ex(len(hw), hw_, nj_, nclass, gp, 0, labels.data_ptr(), result.data_ptr(), ws.data_ptr(),
                                                       B, 0, B, C.byref(cfg), None))

            # a gradient call reads what ITS forward left (sel): each forward leg is followed by its own gradient leg
            per = rounds_of({'mining forward': lambda: fwd(cfgs['mining']), 'mining gradient': lambda: bwd(cfgs['mining']),
                             'focal forward': lambda: fwd(cfgs['focal']), 'focal gradient': lambda: bwd(cfgs['focal'])})
            head_bytes = 4.0 * B * sum(h * l for h, l in zip(hw, ld))
            rec_bytes = 4.0 * B * A * nv
            moved = head_bytes + 2 * rec_bytes          # heads in, labels in, result out == result in, labels in, gradient out
            say('# %s batch %d, %d classes: %d anchors; heads %.1f MB, one [A][nvars] record array %.1f MB' % (pname, B, nclass, A, head_bytes / 1e6, rec_bytes / 1e6))
            for k in per:
                extra = ''
                if k in ('focal gradient', 'focal forward', 'mining forward'):
                    extra = '   %.1f MB moved: %.2f TB/s' % (moved / 1e6, moved / (np.median(per[k]) * 1e-3) / 1e12)
                row(k, per[k], extra)
            say('  forward  mining | focal: %s' % separated(per['mining forward'], per['focal forward']))
            say('  gradient mining | focal: %s' % separated(per['mining gradient'], per['focal gradient']))
            tot = {k: np.median(per[k + ' forward']) + np.median(per[k + ' gradient']) for k in cfgs}
            say('  forward + gradient: mining %.4f ms, focal %.4f ms (focal - mining %+.4f ms)' % (tot['mining'], tot['focal'], tot['focal'] - tot['mining']))

    say('# ---- through the handle: ssd_train_step_dev, vgg300 batch 32, 20 classes, learning rate 0')
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
                net.set_loss(kind, 2.0, 0.25)
                net.train_step_dev(xt, yt)

            per = rounds_of({'mining': lambda: step('mining'), 'focal': lambda: step('focal')})
            say('# %s step' % dtype)
            for k in per:
                row(k, per[k], '   %.0f images/s' % (B / (np.median(per[k]) * 1e-3)))
            d = float(np.median(per['focal']) - np.median(per['mining']))
            say('  focal - mining %+.4f ms (%+.2f %% of the mining step); mining | focal: %s'
                % (d, 100 * d / float(np.median(per['mining'])), separated(per['mining'], per['focal'])))
            net.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
