#!/usr/bin/env python3
"""Inference rate of the bf16 and the fp8 handle: vgg300, batch 128, input resident in HBM, one process, the
two handles built from the same weights and run in interleaved rounds (bf16, fp8, bf16, fp8, ...), so that both see the same
clocks and the same neighbours.  Per handle: ms per batch and per image, median and min..max over the rounds; the ratio per
round.  Then per-layer kernel times of both handles from the library's own per-launch events, on ONE stream (ssd_set_overlap 0:
no second lane, no side stream, so an event interval is one kernel's duration), again interleaved; a layer counts as faster in
fp8 only if the rounds separate: max(fp8) < min(bf16).

    python tools/infer_rate.py [--batch 128] [--rounds 5] [--passes 20] [--out profiles/fp8_infer_rate.txt]

--a-trous false measures the fc graph with three handles from the same tests/fc_ref.py weights: bf16, fp8 created
under SSD_FP8_BIGK=0 (the 7x7 fc6 on conv_bigk_fwd_bf16 with a quantise pass behind it) and fp8 under SSD_FP8_BIGK=1 (fc6 on
e4m3), the same tables with one column per handle, then the kernels of mod_pool5, mod_conv6, mod_conv7 and the filter images one
by one, with fc6's rate from its executed FLOPs.

    python tools/infer_rate.py --a-trous false --out profiles/fp8_fc_infer_rate.txt

--mxfp8 adds the mxfp8 handle as the handle under test beside bf16 and fp8 (a-trous graph): the ratios and verdicts
are then mxfp8 against each of the two, and the per-layer table has its pools and quantise passes.

    python tools/infer_rate.py --mxfp8 --out profiles/mxfp8_infer_rate.txt

--a-trous false --mxfp8 measures the fc graph's mxfp8 handle with its 7x7 fc6 on MX operands: four handles from the
same weights -- bf16, fp8 (SSD_FP8_BIGK=1, calibrated), mxfp8 under SSD_MXFP8_BIGK=0 (fc6 on conv_bigk_fwd_bf16 with a quantise pass
behind it) and, the handle under test, mxfp8 under SSD_MXFP8_BIGK=1.

    python tools/infer_rate.py --a-trous false --mxfp8 --out profiles/mxfp8_fc_infer_rate.txt

--mxfp6 (a-trous graph) measures four handles from the same weights -- bf16, fp8, mxfp8 and, the handle under test, mxfp6 (DESIGN.md
24): the ratios and verdicts are mxfp6 against each of the others, and the convolution kernels of conv4_2 and mod_conv6 are listed
with their TF/s for every handle.

    python tools/infer_rate.py --mxfp6 --out profiles/mxfp6_infer_rate.txt
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


def layer_times(net, x, passes, by_label=None):
    """{layer: ms per pass} from the handle's per-launch events (labels 'kernel:layer'); by_label (a dict) gets {label: ms}"""
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
            if by_label is not None:
                by_label[label] = by_label.get(label, 0.0) + float(ms) / passes
    return out


def mmm(v):
    return '%10.4f (%.4f..%.4f)' % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--preset', default='vgg300')
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--passes', type=int, default=20)
    ap.add_argument('--a-trous', default='true', choices=['true', 'false'], help="false: the fc graph, three handles (SSD_FP8_BIGK 0 / 1)"
                    "; with --mxfp8 four (SSD_MXFP8_BIGK 0 / 1)")
    ap.add_argument('--mxfp8', action='store_true', help='a further handle, mxfp8, as the handle under test (fc graph: under SSD_MXFP8_BIGK=1)')
    ap.add_argument('--mxfp6', action='store_true', help='a-trous graph: bf16, fp8, mxfp8 and mxfp6 handles, mxfp6 as the handle under test')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.mxfp6:
        if args.a_trous == 'false':
            ap.error('--mxfp6 measures the a-trous graph: the fc graph has no mxfp6 kernel for its 7x7 fc6')
        args.mxfp8 = True
    import torch
    from oracle import boxes as ob, ssdvgg_ref as ref
    from ssd_tensorflow_amd._lib import lib, check
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    fc = args.a_trous == 'false'
    preset = ob.get_preset(args.preset)
    if fc:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import fc_ref
        w = fc_ref.init_params(preset, 20, seed=42)
        # (name, dtype, the switch read when the handle is created, its value)
        if args.mxfp8:
            handles = [('bf16', 'bf16', None, None), ('fp8', 'fp8', 'SSD_FP8_BIGK', '1'), ('mxfp8/bigk0', 'mxfp8', 'SSD_MXFP8_BIGK', '0'),
                       ('mxfp8/bigk1', 'mxfp8', 'SSD_MXFP8_BIGK', '1')]
        else:
            handles = [('bf16', 'bf16', None, None), ('fp8/bigk0', 'fp8', 'SSD_FP8_BIGK', '0'), ('fp8/bigk1', 'fp8', 'SSD_FP8_BIGK', '1')]
    else:
        w = ref.init_params(preset, 20, seed=42, alive=True)
        handles = [('bf16', 'bf16', None, None), ('fp8', 'fp8', None, None)] + ([('mxfp8', 'mxfp8', None, None)] if args.mxfp8 else []) + ([('mxfp6', 'mxfp6', None, None)] if args.mxfp6 else [])
    x = torch.from_numpy(ref.synth_images(np.random.default_rng(5), args.batch, preset)).cuda()
    with Session(0) as sess:
        nets = {}
        for name, dt, switch, bigk in handles:
            saved = os.environ.get(switch) if switch else None
            if switch:
                os.environ[switch] = bigk      # read when the handle is created
            try:
                nets[name] = SSDVGG(sess, args.preset)
                nets[name].build_from_vgg(None, 20, a_trous=not fc, max_batch=args.batch, training=False, weights=w, dtype=dt)
            finally:
                if switch:
                    os.environ.pop(switch)
                    if saved is not None:
                        os.environ[switch] = saved
            if dt == 'fp8':
                nets[name].calibrate_fp8(x[:32])
        last = handles[-1][0]                 # the handle under test: every comparison is this one against another
        for dt in nets:                       # warm-up: code objects, clocks
            timed_passes(nets[dt], x, 5)
        say('# tools/infer_rate.py: %s%s, batch %d, resident input, %d interleaved rounds of %d passes per handle, %s'
            % (args.preset, ' fc graph' if fc else '', args.batch, args.rounds, args.passes, torch.cuda.get_device_name(0)))
        if fc:
            for name in nets:
                if nets[name].dtype == 'fp8':
                    say('# %s scales: %s' % (name, ' '.join(nets[name].fp8_scales)))
        ms = {dt: [] for dt in nets}
        for r in range(args.rounds):
            for dt in nets:
                ms[dt].append(timed_passes(nets[dt], x, args.passes))
        say('# %-11s %14s %26s %12s' % ('handle', 'ms/batch', '(min..max over rounds)', 'ms/image') if fc else
            '# %-6s %14s %26s %12s' % ('handle', 'ms/batch', '(min..max over rounds)', 'ms/image'))
        for dt in nets:
            v = ms[dt]
            say(('  %-11s %14.3f %15.3f..%.3f %14.4f' if fc else '  %-6s %14.3f %15.3f..%.3f %14.4f')
                % (dt, statistics.median(v), min(v), max(v), statistics.median(v) / args.batch))
        for other in [h[0] for h in handles[:-1]]:
            ratios = [a / b for a, b in zip(ms[other], ms[last])]
            sep = max(ms[last]) < min(ms[other]) or max(ms[other]) < min(ms[last])
            say('# %s time / %s time: median %.3f, per round %s; the rounds %s'
                % (other, last, statistics.median(ratios), ' '.join('%.3f' % q for q in ratios),
                   'separate the two handles' if sep else 'do NOT separate the two handles'))
        # ---- per layer, one stream
        for dt in nets:
            check(lib.ssd_set_overlap(nets[dt]._h, 0))
            layer_times(nets[dt], x, 2)
        per = {dt: [] for dt in nets}
        lab = {dt: [] for dt in nets}
        for r in range(args.rounds):
            for dt in nets:
                lab[dt].append({})
                per[dt].append(layer_times(nets[dt], x, max(args.passes // 4, 2), lab[dt][-1]))
        layers = [k for k in per['bf16'][0] if all(k in per[dt][0] for dt in nets)]
        say('# per layer on one stream (kernel events, ms per batch): median (min..max); fp8 includes the layer\'s e4m3 outputs')
        if fc or args.mxfp8:
            say('# verdict: %s against bf16; a quantise pass behind a bf16 layer counts with that layer' % last)
        say('# %-18s ' % 'layer' + ' '.join('%28s' % dt for dt in nets) + ' %8s  %s' % ('ratio', 'verdict'))
        tot = {dt: 0.0 for dt in nets}
        for k in layers:
            cols = {dt: [p[k] for p in per[dt]] for dt in nets}
            for dt in nets:
                tot[dt] += statistics.median(cols[dt])
            a, f = cols['bf16'], cols[last]
            tag = 'mxfp6' if args.mxfp6 else 'mxfp8' if args.mxfp8 else 'fp8'
            verdict = tag + ' faster' if max(f) < min(a) else (tag + ' SLOWER' if max(a) < min(f) else 'not separated')
            for other in (['fp8'] + (['mxfp8/bigk0'] if fc else []) + (['mxfp8'] if args.mxfp6 else []) if args.mxfp8 else []):      # ... and against these handles' rows
                g = cols[other]
                verdict += '; against %s %.3f %s' % (other, statistics.median(g) / max(statistics.median(f), 1e-9),
                                                     'faster' if max(f) < min(g) else ('SLOWER' if max(g) < min(f) else 'not separated'))
            say('  %-18s ' % k + ' '.join(mmm(cols[dt]) for dt in nets) + ' %8.3f  %s' % (statistics.median(a) / max(statistics.median(f), 1e-9), verdict))
        for dt in nets:
            for k in per[dt][0]:
                if k not in layers:
                    f = [p.get(k, 0.0) for p in per[dt]]
                    tot[dt] += statistics.median(f)
                    say('  %-18s only in %s: %s' % (k, dt, mmm(f)) if fc or args.mxfp8 else '  %-18s %28s %s' % (k, '-', mmm(f)))
        say('# sum of the kernels per batch, one stream: ' + ', '.join('%s %.3f ms' % (dt, tot[dt]) for dt in nets))
        if args.mxfp6:
            # ---- the convolution kernels of conv4_2 and mod_conv6, with their rates from the executed FLOPs 2 * pixels * Ci * Co * 9
            f38, f19 = preset['maps'][0][0], preset['maps'][1][0]
            flops = {'conv4_2': 2.0 * args.batch * f38 * f38 * 512 * 512 * 9, 'mod_conv6': 2.0 * args.batch * f19 * f19 * 512 * 1024 * 9}
            say('# convolution kernels of conv4_2 (%.1f GFLOP) and mod_conv6 (%.1f GFLOP), ms per batch and TF/s'
                % (flops['conv4_2'] / 1e9, flops['mod_conv6'] / 1e9))
            for dt in nets:
                for label in lab[dt][0]:
                    kern, _, layer = label.partition(':')
                    if layer in flops and kern.startswith('conv'):
                        v = [p.get(label, 0.0) for p in lab[dt]]
                        say('  %-6s %-40s %s  %.0f TF/s' % (dt, label, mmm(v), flops[layer] / (statistics.median(v) * 1e-3) / 1e12))
        if fc:
            # ---- the kernels around fc6 one by one; fc6's rate from its executed FLOPs 2 * pixels * Ci * Co * taps
            fmap = preset['maps'][1][0]
            flops6 = 2.0 * args.batch * fmap * fmap * 512 * 4096 * 49
            say('# kernels of mod_pool5, mod_conv6, mod_conv7 and the filter images (ms per batch); mod_conv6: TF/s from 2*pixels*Ci*Co*49 = %.1f GFLOP' % (flops6 / 1e9))
            for dt in nets:
                for label in lab[dt][0]:
                    layer = label.split(':', 1)[1] if ':' in label else label
                    if layer in ('mod_pool5', 'mod_conv6', 'mod_conv7', 'filters'):
                        v = [p.get(label, 0.0) for p in lab[dt]]
                        rate = '  %.0f TF/s' % (flops6 / (statistics.median(v) * 1e-3) / 1e12) if layer == 'mod_conv6' and 'conv' in label.split(':')[0] else ''
                        say('  %-11s %-44s %s%s' % (dt, label, mmm(v), rate))
            n0, n1 = handles[-2][0], handles[-1][0]      # the same dtype with the switch 0 and 1
            k0, k1 = [p['mod_conv6'] for p in per[n0]], [p['mod_conv6'] for p in per[n1]]
            a = [p['mod_conv6'] for p in per['bf16']]
            say('# rule (DESIGN.md 18): mod_conv6 row max(%s) %.4f %s min(bf16) %.4f; whole handle max(bigk1) %.3f %s min(bigk0) %.3f'
                % (n1, max(k1), '<' if max(k1) < min(a) else '>=', min(a), max(ms[n1]), '<' if max(ms[n1]) < min(ms[n0]) else '>=', min(ms[n0])))
            if args.mxfp8:
                say('# mod_conv6 row (a quantise pass behind a bf16 layer counts with it): max(%s) %.4f %s min(%s) %.4f'
                    % (n1, max(k1), '<' if max(k1) < min(k0) else '>=', n0, min(k0)))
            say('# %s: not measured' % ('vgg512' if args.preset == 'vgg300' else 'vgg300'))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
