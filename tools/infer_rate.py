#!/usr/bin/env python3
"""Inference rate of the bf16 and the fp8 handle: vgg300, batch 128, input resident in HBM, one process, the
two handles built from the same weights and run in interleaved rounds (bf16, fp8, bf16, fp8, ...), so that both see the same
clocks and the same neighbours.  Per handle: ms per batch and per image, median and min..max over the rounds; the ratio per
round.  Then per-layer kernel times of both handles from the library's own per-launch events, on ONE stream (ssd_set_overlap 0:
no second lane, no side stream, so an event interval is one kernel's duration), again interleaved; a layer counts as faster in
fp8 only if the rounds separate: max(fp8) < min(bf16).

    python tools/infer_rate.py [--batch 128] [--rounds 5] [--passes 20] [--out profiles/fp8_infer_rate.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_passes(net, x, passes):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(passes):
        net.infer_dev(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / passes


def layer_times(net, x, passes):
    """{layer: ms per pass} from the handle's per-launch events (labels 'kernel:layer')"""
    from ssd_tensorflow_amd._lib import lib, check
    check(lib.ssd_profile_enable(net._h, 2))
    for _ in range(passes):
        net.infer_dev(x)
    buf = C.create_string_buffer(1 << 18)
    check(lib.ssd_profile_report(net._h, buf, len(buf)))
    check(lib.ssd_profile_enable(net._h, 0))
    out = {}
    for line in buf.value.decode().strip().split('\n'):
        if line:
            label, cnt, ms, fl, by = line.split('\t')
            layer = label.split(':', 1)[1] if ':' in label else label
            out[layer] = out.get(layer, 0.0) + float(ms) / passes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--preset', default='vgg300')
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--passes', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from oracle import boxes as ob, ssdvgg_ref as ref
    from ssd_tensorflow_amd._lib import lib, check
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    preset = ob.get_preset(args.preset)
    w = ref.init_params(preset, 20, seed=42, alive=True)
    x = torch.from_numpy(ref.synth_images(np.random.default_rng(5), args.batch, preset)).cuda()
    with Session(0) as sess:
        nets = {}
        for dt in ('bf16', 'fp8'):
            nets[dt] = SSDVGG(sess, args.preset)
            nets[dt].build_from_vgg(None, 20, max_batch=args.batch, training=False, weights=w, dtype=dt)
        nets['fp8'].calibrate_fp8(x[:32])
        for dt in nets:                       # warm-up: code objects, clocks
            timed_passes(nets[dt], x, 5)
        say('# tools/infer_rate.py: %s, batch %d, resident input, %d interleaved rounds of %d passes per handle, %s'
            % (args.preset, args.batch, args.rounds, args.passes, torch.cuda.get_device_name(0)))
        ms = {dt: [] for dt in nets}
        for r in range(args.rounds):
            for dt in nets:
                ms[dt].append(timed_passes(nets[dt], x, args.passes))
        say('# %-6s %14s %26s %12s' % ('handle', 'ms/batch', '(min..max over rounds)', 'ms/image'))
        for dt in nets:
            v = ms[dt]
            say('  %-6s %14.3f %15.3f..%.3f %14.4f' % (dt, statistics.median(v), min(v), max(v), statistics.median(v) / args.batch))
        ratios = [a / b for a, b in zip(ms['bf16'], ms['fp8'])]
        sep = max(ms['fp8']) < min(ms['bf16']) or max(ms['bf16']) < min(ms['fp8'])
        say('# bf16 time / fp8 time: median %.3f, per round %s; the rounds %s' % (statistics.median(ratios), ' '.join('%.3f' % q for q in ratios),
                                                                                'separate the two handles' if sep else 'do NOT separate the two handles'))
        # ---- per layer, one stream
        for dt in nets:
            check(lib.ssd_set_overlap(nets[dt]._h, 0))
            layer_times(nets[dt], x, 2)
        per = {dt: [] for dt in nets}
        for r in range(args.rounds):
            for dt in nets:
                per[dt].append(layer_times(nets[dt], x, max(args.passes // 4, 2)))
        layers = [k for k in per['bf16'][0] if k in per['fp8'][0]]
        say('# per layer on one stream (kernel events, ms per batch): median (min..max); fp8 includes the layer\'s e4m3 outputs')
        say('# %-18s %28s %28s %8s  %s' % ('layer', 'bf16', 'fp8', 'ratio', 'verdict'))
        tot = {dt: 0.0 for dt in nets}
        for k in layers:
            a = [p[k] for p in per['bf16']]
            f = [p[k] for p in per['fp8']]
            tot['bf16'] += statistics.median(a); tot['fp8'] += statistics.median(f)
            verdict = 'fp8 faster' if max(f) < min(a) else ('fp8 SLOWER' if max(a) < min(f) else 'not separated')
            say('  %-18s %10.4f (%.4f..%.4f) %10.4f (%.4f..%.4f) %8.3f  %s' % (k, statistics.median(a), min(a), max(a), statistics.median(f),
                                                                               min(f), max(f), statistics.median(a) / max(statistics.median(f), 1e-9), verdict))
        only8 = [k for k in per['fp8'][0] if k not in per['bf16'][0]]
        for k in only8:
            f = [p[k] for p in per['fp8']]
            tot['fp8'] += statistics.median(f)
            say('  %-18s %28s %10.4f (%.4f..%.4f)' % (k, '-', statistics.median(f), min(f), max(f)))
        say('# sum of the kernels per batch, one stream: bf16 %.3f ms, fp8 %.3f ms' % (tot['bf16'], tot['fp8']))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
