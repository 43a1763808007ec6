#!/usr/bin/env python3
"""GPU time of gradient clipping by global norm.  HIP events, ONE process, interleaved rounds; the yardstick is the
step with clipping off -- the step of the commit before the switch existed -- in the same process, not a number chosen in advance.
  op level, on resident buffers of the vgg300 arena's size (ssd_op_momentum_update_clipped): the plain update (max_norm 0), the
      measured one (inf) and a clipped one; the norm pass's own time is the measured update minus the plain one, its bandwidth
      4 bytes per parameter over that time;
  through the handle: ssd_train_step_dev at vgg300 batch 32, bf16 and fp32, learning rate 0 (the weights stay), clipping off, inf,
      and a threshold of half the measured norm, which clips every step.
A measurement, not a test.

    python tools/clip_rate.py [--rounds 5] [--reps 20] [--out profiles/grad_clip_rate.txt]
"""
import argparse
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
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(7)

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

    def verdict(off, on, what):
        """do the rounds separate, and is the difference beyond the off leg's own min ... max range"""
        d = float(np.median(on) - np.median(off))
        spread = max(off) - min(off)
        if max(off) < min(on):
            sep = 'every round of off is below every round of %s' % what
        elif max(on) < min(off):
            sep = 'every round of %s is below every round of off' % what
        else:
            sep = 'the rounds overlap: not separated'
        say('  %s - off %+.4f ms (%+.2f %% of off; off\'s own min ... max range %.4f ms): %s%s'
            % (what, d, 100 * d / float(np.median(off)), spread, sep,
               '; slower by more than that range' if d > spread and max(off) < min(on) else ''))

    say('# tools/clip_rate.py: %s; HIP events, one process, %d interleaved rounds of %d calls per leg: median of the rounds\' medians '
        '(min ... max)' % (torch.cuda.get_device_name(0), args.rounds, args.reps))
    n = int(lib.ssd_arena_floats(b'vgg300', 20))
    say('# ---- op level: ssd_op_momentum_update_clipped on resident buffers, %d parameters (the vgg300 / 20 classes arena: %.1f MB per buffer), '
        'learning rate 0, momentum 0.9' % (n, 4e-6 * n))
    w = torch.randn(n, device=dev)
    acc = torch.zeros(n, device=dev)
    g = torch.randn(n, device=dev) * 1e-3
    ws = torch.zeros(int(lib.ssd_op_grad_norm_ws_bytes(n)), dtype=torch.uint8, device=dev)
    rep = torch.zeros(2, device=dev)
    true_norm = float(g.double().norm())

    def update(max_norm):
        check(lib.ssd_op_momentum_update_clipped(w.data_ptr(), acc.data_ptr(), g.data_ptr(), n, 0.0, 0.9, 1.0, max_norm, ws.data_ptr(), rep.data_ptr(), None))

    per = rounds_of({'off (max_norm 0)': lambda: update(0.0), 'inf': lambda: update(float('inf')), 'clipping': lambda: update(0.5 * true_norm)})
    for k in per:
        row(k, per[k], '   %.2f TB/s of %d bytes per parameter' % ((20 if k.startswith('off') else 24) * n / (np.median(per[k]) * 1e-3) * 1e-12,
                                                                 20 if k.startswith('off') else 24))
    torch.cuda.synchronize()
    say('  reported norm %r, factor %r (norm of the buffer in float64: %r)' % (float(rep[0]), float(rep[1]), true_norm))
    dn = float(np.median(per['inf']) - np.median(per['off (max_norm 0)']))
    say('  the norm pass and its finish (inf - off): %.4f ms = %.1f us; %.2f TB/s of the arena\'s %.1f MB read once'
        % (dn, 1e3 * dn, 4 * n / (dn * 1e-3) * 1e-12 if dn > 0 else float('nan'), 4e-6 * n))
    verdict(per['off (max_norm 0)'], per['inf'], 'inf')
    verdict(per['off (max_norm 0)'], per['clipping'], 'clipping')
    del w, acc, g, ws

    say('# ---- through the handle: ssd_train_step_dev, vgg300 batch 32, 20 classes, mining, learning rate 0')
    B = 32
    preset = su.get_preset_by_name('vgg300')
    boxes, classes = [], []
    for _ in range(B):
        k = int(rng.integers(1, 9))
        bw, bh = rng.uniform(0.05, 0.6, k), rng.uniform(0.05, 0.6, k)
        boxes.append(np.stack([rng.uniform(bw / 2, 1 - bw / 2), rng.uniform(bh / 2, 1 - bh / 2), bw, bh], 1))
        classes.append(rng.integers(0, 20, k).astype(np.int32))
    yt = torch.from_numpy(np.ascontiguousarray(su.encode_labels_batch(preset, 20, boxes, classes), np.float32)).to(dev)
    xt = torch.rand((B, 300, 300, 3), device=dev) * 255
    with Session(0) as sess:
        for dtype in ('bf16', 'f32'):
            net = SSDVGG(sess, 'vgg300')
            net.build_from_vgg(None, 20, max_batch=B, dtype=dtype)
            net.build_optimizer(learning_rate=0.0, clip_norm=float('inf'))
            net.train_step_dev(xt, yt)
            norm = net.get_grad_norm_step()[0]
            half = 0.5 * norm

            def step(clip_norm):
                net.set_grad_clip(clip_norm)
                net.train_step_dev(xt, yt)

            per = rounds_of({'off': lambda: step(0.0), 'inf': lambda: step(float('inf')), 'clipping': lambda: step(half)})
            say('# %s step (gradient norm of the first step %.6g; clipping: threshold %.6g, last factor %r)'
                % (dtype, norm, half, net.get_grad_norm_step()[1]))
            for k in per:
                row(k, per[k], '   %.0f images/s' % (B / (np.median(per[k]) * 1e-3)))
            verdict(per['off'], per['inf'], 'inf')
            verdict(per['off'], per['clipping'], 'clipping')
            net.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
