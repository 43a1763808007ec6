#!/usr/bin/env python3
"""GPU time of the weight EMA.  HIP events, ONE process, interleaved rounds; the yardstick is the momentum update
measured in the same process, not a number chosen in advance.
  op level, on resident buffers of the vgg300 arena's size: the momentum update (ssd_op_momentum_update_clipped, max_norm 0; 20
      bytes per parameter), the EMA update (ssd_op_ema_update; 12) and the swap (ssd_op_ema_swap; 16), in us and TB/s, with the
      ratio of the EMA kernel's bytes per second to the momentum update's; both back to back and with the last-level cache emptied
      in front of every call (a training step leaves the arenas cold: the second table is the one that counts);
  through the handle: ssd_train_step_dev at vgg300 batch 32, bf16 and fp32, learning rate 0 (the weights stay), a handle without
      and one with the EMA, and a second handle without it as the control for what two handles differ by on their own.
A measurement, not a test.

    python tools/ema_rate.py [--rounds 5] [--reps 20] [--out profiles/ema_rate.txt]
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

    say('# tools/ema_rate.py: %s; HIP events, one process, %d interleaved rounds of %d calls per leg: median of the rounds\' medians '
        '(min ... max)' % (torch.cuda.get_device_name(0), args.rounds, args.reps))
    n = int(lib.ssd_arena_floats(b'vgg300', 20))
    say('# ---- op level on resident buffers, %d parameters (the vgg300 / 20 classes arena: %.1f MB per buffer), learning rate 0' % (n, 4e-6 * n))
    w = torch.randn(n, device=dev)
    e = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev) * 1e-3
    acc = torch.zeros(n, device=dev)

    def momentum():
        check(lib.ssd_op_momentum_update_clipped(w.data_ptr(), acc.data_ptr(), g.data_ptr(), n, 0.0, 0.9, 1.0, 0.0, None, None, None))

    def ema():
        check(lib.ssd_op_ema_update(e.data_ptr(), w.data_ptr(), n, 0.999, 10 ** 6, None))

    def swap():
        check(lib.ssd_op_ema_swap(e.data_ptr(), w.data_ptr(), n, None))

    legs = {'momentum': (momentum, 20), 'ema': (ema, 12), 'swap': (swap, 16)}
    # Back to back the same buffers come round again every call, and the chip's 256 MiB last-level cache keeps part of them: all of
    # the EMA's two buffers (211 MB) and less of the momentum update's three (316 MB).  In a training step the arenas are cold -- the
    # step moves gigabytes between two updates -- so the second table reads 1 GiB of another buffer in front of every timed call.
    flush = torch.zeros(1 << 28, dtype=torch.float32, device=dev)
    for title, pre in (('back to back (the buffers partly in the last-level cache)', None),
                       ('cold: 1 GiB of another buffer read in front of every call, untimed', lambda: flush.sum())):
        say('  -- ' + title)
        per = rounds_of({k: f for k, (f, _) in legs.items()}, pre)
        rate = {}
        for k, (_, nbytes) in legs.items():
            rate[k] = nbytes * n / (np.median(per[k]) * 1e-3) * 1e-12
            row(k, per[k], '   %7.1f us  %.2f TB/s of %d bytes per parameter' % (1e3 * np.median(per[k]), rate[k], nbytes))
        torch.cuda.synchronize()
        say('  ema / momentum: time %.3f (the bytes alone: 12 / 20 = 0.6); bytes per second %.3f; swap / momentum: time %.3f (16 / 20 = 0.8); '
            'bytes per second %.3f' % (float(np.median(per['ema']) / np.median(per['momentum'])), rate['ema'] / rate['momentum'],
                                       float(np.median(per['swap']) / np.median(per['momentum'])), rate['swap'] / rate['momentum']))
    del w, e, g, acc, flush

    say('# ---- through the handle: ssd_train_step_dev, vgg300 batch 32, 20 classes, mining, momentum, learning rate 0, one handle per leg')
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
            # two handles are two placements of every buffer: the third, a second handle without the EMA, shows what that alone is worth
            for name, decay in (('no ema', 0.0), ('ema 0.999', 0.999), ('no ema (a second handle)', 0.0)):
                nets[name] = SSDVGG(sess, 'vgg300')
                nets[name].build_from_vgg(None, 20, max_batch=B, dtype=dtype)
                nets[name].build_optimizer(learning_rate=0.0, ema_decay=decay)
            per = rounds_of({name: (lambda net=net: net.train_step_dev(xt, yt)) for name, net in nets.items()})
            say('# %s step' % dtype)
            for k in per:
                row(k, per[k], '   %.0f images/s' % (B / (np.median(per[k]) * 1e-3)))
            verdict(per['no ema'], per['ema 0.999'], 'no ema', 'ema 0.999')
            verdict(per['no ema'], per['no ema (a second handle)'], 'no ema', 'no ema (a second handle)')
            if dtype == 'f32':
                net = nets['ema 0.999']
                sw = rounds_of({'swap in + swap out': lambda: (net.swap_ema(), net.swap_ema())})
                row('averaged_weights(): two swaps', sw['swap in + swap out'])
            for net in nets.values():
                net.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
