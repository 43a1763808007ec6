#!/usr/bin/env python3
"""GPU time of the AdamW update.  HIP events, ONE process, interleaved rounds; the yardstick is the momentum update
measured in the same process, not a number chosen in advance.
  op level, on resident buffers of the vgg300 arena's size: the momentum update (ssd_op_momentum_update_clipped, max_norm 0; 20
      bytes per parameter), the AdamW update (ssd_op_adamw_update; 28) and the AdamW update with clipping (32: the norm pass reads
      the gradient once more), in us and TB/s; at the momentum update's bytes per second the 28 bytes would take 1.4 x its time;
      both back to back and with the last-level cache emptied in front of every call;
  through the handle: ssd_train_step_dev at vgg300 batch 32, bf16 and fp32, learning rate 0 (the weights stay), one handle per rule
      and a second momentum handle as the control for what two handles differ by on their own.
A measurement, not a test.

    python tools/adamw_rate.py [--rounds 5] [--reps 20] [--out profiles/adamw_rate.txt]
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

    def timed(fn, pre=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if pre:
            pre()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds_of(legs, pre=None):
        """{name: [per-round medians]} of the legs run in turn, args.rounds times; pre runs in front of every timed call, untimed"""
        for fn in legs.values():
            for _ in range(3):
                timed(fn, pre)
        per = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                per[k].append(float(np.median([timed(fn, pre) for _ in range(args.reps)])))
        return per

    def row(name, t, extra=''):
        say('  %-32s %8.4f ms  (%.4f ... %.4f)%s' % (name, float(np.median(t)), min(t), max(t), extra))

    def verdict(base, other, base_name, what):
        d = float(np.median(other) - np.median(base))
        spread = max(base) - min(base)
        if max(base) < min(other):
            sep = 'every round of %s is below every round of %s' % (base_name, what)
        elif max(other) < min(base):
            sep = 'every round of %s is below every round of %s' % (what, base_name)
        else:
            sep = 'the rounds overlap: not separated'
        say('  %s - %s %+.4f ms (%+.2f %% of %s; its own min ... max range %.4f ms): %s'
            % (what, base_name, d, 100 * d / float(np.median(base)), base_name, spread, sep))

    say('# tools/adamw_rate.py: %s; HIP events, one process, %d interleaved rounds of %d calls per leg: median of the rounds\' medians '
        '(min ... max)' % (torch.cuda.get_device_name(0), args.rounds, args.reps))
    n = int(lib.ssd_arena_floats(b'vgg300', 20))
    nd = n // 8 * 7
    say('# ---- op level on resident buffers, %d parameters (the vgg300 / 20 classes arena: %.1f MB per buffer), learning rate 0' % (n, 4e-6 * n))
    w = torch.randn(n, device=dev)
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    g = torch.randn(n, device=dev) * 1e-3
    ws = torch.zeros(int(lib.ssd_op_grad_norm_ws_bytes(n)), dtype=torch.uint8, device=dev)
    rep = torch.zeros(2, device=dev)
    true_norm = float(g.double().norm())
    acc = torch.zeros(n, device=dev)

    def momentum():
        check(lib.ssd_op_momentum_update_clipped(w.data_ptr(), acc.data_ptr(), g.data_ptr(), n, 0.0, 0.9, 1.0, 0.0, None, None, None))

    def adamw(max_norm):
        check(lib.ssd_op_adamw_update(w.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), n, nd, 0.0, 0.9, 0.999, 1e-8, 0.01, 10, 1.0,
                                      max_norm, ws.data_ptr(), rep.data_ptr(), None))

    legs = {'momentum': (momentum, 20), 'adamw': (lambda: adamw(0.0), 28), 'adamw + clipping': (lambda: adamw(0.5 * true_norm), 32)}
    # Back to back the same buffers come round again every call, and the chip's 256 MiB last-level cache keeps part of them: more of
    # the momentum update's three buffers (316 MB) than of AdamW's four (422 MB).  In a training step the arenas are cold -- the step
    # moves gigabytes between two updates -- so the second table reads 1 GiB of another buffer in front of every timed call.
    flush = torch.zeros(1 << 28, dtype=torch.float32, device=dev)
    for title, pre in (('back to back (the buffers partly in the last-level cache)', None),
                       ('cold: 1 GiB of another buffer read in front of every call, untimed', lambda: flush.sum())):
        say('  -- ' + title)
        per = rounds_of({k: f for k, (f, _) in legs.items()}, pre)
        for k, (_, nbytes) in legs.items():
            row(k, per[k], '   %7.1f us  %.2f TB/s of %d bytes per parameter' % (1e3 * np.median(per[k]), nbytes * n / (np.median(per[k]) * 1e-3) * 1e-12, nbytes))
        torch.cuda.synchronize()
        say('  adamw / momentum = %.3f (the bytes alone: 28 / 20 = 1.4); adamw + clipping / momentum = %.3f (32 / 20 = 1.6)'
            % (float(np.median(per['adamw']) / np.median(per['momentum'])), float(np.median(per['adamw + clipping']) / np.median(per['momentum']))))
        verdict(per['momentum'], per['adamw'], 'momentum', 'adamw')
    say('  last reported norm %r, factor %r (norm of the buffer in float64: %r)' % (float(rep[0]), float(rep[1]), true_norm))
    del w, m, v, g, ws, acc, flush

    say('# ---- through the handle: ssd_train_step_dev, vgg300 batch 32, 20 classes, mining, learning rate 0, one handle per rule')
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
            nets = {}
            # two handles are two placements of every buffer: the third, a second momentum handle, shows what that alone is worth
            for name in ('momentum', 'adamw', 'momentum (a second handle)'):
                nets[name] = SSDVGG(sess, 'vgg300')
                nets[name].build_from_vgg(None, 20, max_batch=B, dtype=dtype)
                nets[name].build_optimizer(learning_rate=0.0, optimizer=name.split()[0])
            per = rounds_of({rule: (lambda net=net: net.train_step_dev(xt, yt)) for rule, net in nets.items()})
            say('# %s step' % dtype)
            for k in per:
                row(k, per[k], '   %.0f images/s' % (B / (np.median(per[k]) * 1e-3)))
            verdict(per['momentum'], per['adamw'], 'momentum', 'adamw')
            verdict(per['momentum'], per['momentum (a second handle)'], 'momentum', 'momentum (a second handle)')
            for net in nets.values():
                net.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
