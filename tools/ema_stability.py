#!/usr/bin/env python3
"""Does the weight EMA evaluate better than the last iterate where the repository's own runs misbehave, and does it
cost anything where they do not?  The driver's loop (train.StepLoop) on the shapes set, with BOTH sets of weights of the SAME run
evaluated on the held-out pictures after every epoch: the raw weights, then the average inside averaged_weights():
  a. DESIGN.md 34's fp32 run at a constant learning rate of 1e-3 without clipping, which loses its detector in one epoch
     (profiles/grad_clip_stability.txt: held-out mAP 0.51 -> 0.00 in epoch 19) -- 56 epochs = 1792 updates;
  b. DESIGN.md 7's learnable set on its own schedule (3e-4 until update 96, 7.5e-4 until 768, 1e-4 after) -- 40 epochs = 1280 updates.
The runs are 1280 .. 1792 updates long, so the decays tried are 0.99 (a horizon of 100 updates, three epochs) and 0.999 (1000 updates:
most of the run); BOTH are reported.  Under d = min(decay, (1 + t) / (10 + t)) the decay 0.99 holds from update 891 on and 0.999 from
update 8991 on: in runs this short 0.999 IS the warm-up from the first update to the last, and the two differ only after update 891.  ONE seed per run: the evidence level of DESIGN.md 31's accuracy table.  The training itself
does not depend on the decay (the average feeds nothing back), so the raw rows of the two decays of a setting repeat each other up to
the run-to-run differences of the training kernels.  VOC / COCO is not measured: no data set is here.  A measurement, not a test.

    python tools/ema_stability.py [--epochs-a 56] [--epochs-b 40] [--out profiles/ema_stability.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DECAYS = (0.99, 0.999)
B = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs-a', type=int, default=56)
    ap.add_argument('--epochs-b', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd.average_precision import APCalculator, APs2mAP
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session, LearningRate
    from ssd_tensorflow_amd.train import StepLoop
    from ssd_tensorflow_amd.training_data import TrainingData
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)
        if args.out:      # as the runs go: a run takes a minute
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    def fmt(values):
        return ' '.join('%.2f' % v for v in values)

    def first_at(values, level):
        return next((e + 1 for e, v in enumerate(values) if v >= level), None)

    say('# tools/ema_stability.py: %s; shapes detector (rectangles 0.2 .. 0.5, --match reference, smooth_l1, mining), vgg300, fp32, 1024 '
        'training / 128 held-out pictures, batch 32 (32 updates per epoch), momentum 0.9; mAP: the driver\'s, 11-point at confidence 0.5, '
        'of the raw and of the averaged weights of the SAME run after every epoch; ONE seed per run' % torch.cuda.get_device_name(0))

    def crossover(decay):
        """the first update (counted from 0) at which the warm-up (1 + t) / (10 + t) is no longer below the float32 decay"""
        import numpy as np
        d, t = float(np.float32(decay)), 0
        while (1.0 + t) / (10.0 + t) < d:
            t += 1
        return t

    say('# d = min(decay, (1 + t) / (10 + t)): ' + '; '.join('decay %g holds from update %d on (epoch %d)' % (d, crossover(d), crossover(d) // 32 + 1)
                                                           for d in DECAYS)
        + ' -- before that, and so for the whole of a run shorter than that, the average runs under the warm-up whatever the decay')

    def run(lr, epochs, decay):
        td = TrainingData('shapes', 'vgg300', 1024, 128, augment=False, device=0, shapes_size=[0.2, 0.5])
        raw, avg, steps = [], [], 0
        t0 = time.perf_counter()
        with Session(0) as sess:
            net = SSDVGG(sess, td.preset)
            net.build_from_vgg('vgg_graph', td.num_classes, max_batch=B, dtype='f32')
            net.build_optimizer(learning_rate=lr, weight_decay=0.0005, momentum=0.9, ema_decay=decay)
            net.set_stream(torch.cuda.current_stream().cuda_stream)
            loop = StepLoop(net, sess, td, B, 8)
            for e in range(epochs):
                td.epoch = e
                loop.run_epoch(td.train_generator, True, None, None, False)
                for out, ctx in ((raw, None), (avg, net.averaged_weights())):
                    calc = APCalculator()
                    if ctx is None:
                        loop.run_epoch(td.valid_generator, False, None, calc, True)
                    else:
                        with ctx:
                            loop.run_epoch(td.valid_generator, False, None, calc, True)
                    out.append(APs2mAP(calc.compute_aps()))
            steps = net.get_ema()[1]
        td.close()
        return raw, avg, steps, time.perf_counter() - t0

    summary = []
    settings = (('a', 'DESIGN.md 34: constant learning rate 1e-3, no clipping', LearningRate([0.001], []), args.epochs_a),
                ('b', 'DESIGN.md 7: lr 3e-4 / 7.5e-4 / 1e-4 at 96 / 768', LearningRate([0.0003, 0.00075, 0.0001], [96, 768]), args.epochs_b))
    for key, title, lr, epochs in settings:
        say('# ---- %s. %s; %d epochs = %d updates' % (key, title, epochs, 32 * epochs))
        for decay in DECAYS:
            raw, avg, steps, secs = run(lr, epochs, decay)
            say('  --ema-decay %g  (%d EMA updates, %.0f s)' % (decay, steps, secs))
            say('    held-out mAP, raw weights        ' + fmt(raw))
            say('    held-out mAP, averaged weights   ' + fmt(avg))
            worst = lambda v: min(v[e] - max(v[:e + 1]) for e in range(len(v)))      # the deepest fall below the best so far
            line = ('%s --ema-decay %-6g raw: >= 0.5 from epoch %s, >= 1.0 from %s, final %.4f, deepest fall below its best so far %.2f | '
                    'averaged: >= 0.5 from %s, >= 1.0 from %s, final %.4f, deepest fall %.2f'
                    % (key, decay, first_at(raw, 0.5), first_at(raw, 0.9995), raw[-1], worst(raw), first_at(avg, 0.5), first_at(avg, 0.9995),
                       avg[-1], worst(avg)))
            say('    => ' + line)
            summary.append(line)
    say('# ---- summary, one line per run (epochs count from 1; 1.0 means >= 0.9995)')
    for line in summary:
        say(line)


if __name__ == '__main__':
    main()
