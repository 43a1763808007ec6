#!/usr/bin/env python3
"""Training driver: the counterpart of the reference's train.py loop (train.py:247-343) over
the HIP library.  Same flags (train.py:55-80) plus --preset / --synthetic-train / --synthetic-valid /
--augment / --mosaic / --decoder / --cache-gb / --dtype / --ema-decay / --allreduce-bucket-mb / --allreduce-dtype.  Scalar summaries go to <tensorboard-dir>/<name>/scalars.jsonl
(summaries.py), the annotated image summaries as PNG files; TensorBoard event files are out of scope.

    python -m ssd_tensorflow_amd.train --name run1 --epochs 2 --batch-size 8
    python -m torch.distributed.run --nproc-per-node 8 -m ssd_tensorflow_amd.train ...   # data parallel

A batch never leaves the GPU: the feeder hands out device tensors, the step runs on them, decode + NMS
for the AP bookkeeping runs on the result where it lies (the reference fetches `result` to the host for
decode_boxes, train.py:262-277).  --num-workers N means what the reference's means: N forked processes
prepare the next batches beside the step (training_data.py).  The loop (StepLoop) never waits for the step
it has just launched: losses are read one step late, detections one pass late.  Data parallel: one process
per GPU, rank-sharded batches, bucketed all-reduce of the gradient arena overlapped with backward
(parallel.train_step_dp); losses are summed and detections gathered over ranks for the epoch summaries."""
import argparse
import math
import os
import sys

import numpy as np

from . import _lib, parallel
from .average_precision import APCalculator, DeviceAPCalculator, APs2mAP, add_ap_arguments
from .coco_eval import COCOEvaluator, DeviceCOCOEvaluator, aps_of, format_summary, summarize
from .ssdutils import boxes_from_detection
from .ssdvgg import SSDVGG, Session, LearningRate
from .summaries import SummaryWriter, LossSummary, PrecisionSummary, ImageSummary, GradNormSummary
from .training_data import TrainingData
from .utils import str2bool


def compute_lr(lr_values, lr_boundaries):
    """train.py:43-47"""
    return LearningRate(lr_values, lr_boundaries)


class StepLoop:
    """The body of the reference's epoch loops (train.py:254-281 training, 286-306 validation) over the HIP library,
    shared by main() below and by bench.py's end-to-end block.  The host never waits for the step it has just launched:
    the losses of step k are read after step k + 1 is in flight (ssd_get_losses_step), the detections of step k are
    collected after step k + 1's decode has been launched, and with num_workers > 0 batch k + 1 is already in HBM
    (training_data.py)."""

    def __init__(self, net, sess, td, batch_size, num_workers=0, world=1, rank=0, bucket=0, allreduce_dtype='f32'):
        self.net, self.sess, self.td = net, sess, td
        self.batch_size, self.num_workers = batch_size, num_workers
        self.world, self.rank, self.bucket = world, rank, bucket
        self.allreduce_dtype = allreduce_dtype
        self.steps = 0
        self.grad_norms = None      # a summaries.GradNormSummary when the handle clips or measures (--clip-norm): booked like the losses

    def booked(self, loss_batch, count):
        """(values, weight) for LossSummary.add.  One GPU: the batch's losses, weighted by its samples
        (train.py:271).  Data parallel: a rank's data terms are normalised by count / world, so summed over ranks
        with weight count / world they are count x the global-batch value; the l2 term is the same number on every
        rank that ran a step and absent on a rank whose shard was empty, so rank 0 (never empty) books it, once."""
        world = self.world
        if world <= 1:
            return loss_batch, count
        data = loss_batch['localization'] + loss_batch['confidence']
        l2 = loss_batch['l2'] * world if self.rank == 0 else 0.0
        return dict(total=data + l2, localization=loss_batch['localization'], confidence=loss_batch['confidence'], l2=l2), count / world

    def book(self, loss_batch, count, loss_summary):
        if math.isnan(loss_batch['confidence']):
            print('[!] Confidence loss is NaN.')                                     # train.py:268-269
        if loss_summary is not None:
            loss_summary.add(*self.booked(loss_batch, count))

    def collect(self, dets, gt_boxes, drawn, calc, image_samples=None):
        if dets is None:
            return
        if drawn is not None:
            image_samples.add(drawn.get())
        if isinstance(calc, (DeviceAPCalculator, DeviceCOCOEvaluator)):      # (run_epoch has handed it the pass where it launched the decode)
            return
        for gt, det in zip(gt_boxes, dets.get()):
            if isinstance(calc, COCOEvaluator):
                calc.add_detections(self.coco_gt([gt])[0], boxes_from_detection(det, self.td.lid2name), self.net.preset.image_size)
            else:
                calc.add_detections(gt, boxes_from_detection(det, self.td.lid2name))

    @staticmethod
    def coco_gt(gt_boxes):
        """--ap-protocol coco: the epochs are evaluated on the resized network input, so every image has the network's size and a
        box's area is its own w*h there, not the annotation's (which is in the source picture's pixels)"""
        return [[b._replace(area=None) if getattr(b, 'area', None) is not None else b for b in gt] for gt in gt_boxes]

    def annotate_launch(self, x, n, image_samples):
        """train.py:273-281, 298-306: the first three samples of the epoch that have a decode, drawn on the GPU behind that
        decode: cv2.resize(512, 512) -> draw_box per detection -> clamp -> uint8 RGB (summaries.ImageSummary)."""
        if image_samples is None or self.rank != 0 or image_samples.room() <= 0:
            return None
        import torch
        if not (hasattr(x, 'is_cuda') and x.is_cuda):
            x = torch.from_numpy(x).to(torch.device('cuda', self.net.device))
        k = min(image_samples.room(), n)
        h, w = int(x.shape[1]), int(x.shape[2])
        size = image_samples.SIZE
        drawn = self.net.annotate_last_launch(x.contiguous(), [i * h * w * 12 for i in range(k)], [(h, w)] * k, image_samples.style(self.net.device),
                                              dst_shapes=[(size, size)] * k, rgb_out=True)
        image_samples.reserve(k)
        return drawn

    def run_epoch(self, generator, train, loss_summary, ap_calc, with_ap, image_samples=None):
        net, sess, td, world = self.net, self.sess, self.td, self.world
        pending_det = None
        pending_loss = None                     # sample count of the launched step whose losses are not booked yet
        pending_norm = False                    # the launched step ends in an update whose norm is not booked yet
        for x, y, gt_boxes in generator(self.batch_size, self.num_workers):
            n = len(gt_boxes)
            count = td.global_count if world > 1 else n
            ran = True
            if train and world > 1:
                parallel.train_step_dp(net, x, y, world, self.bucket, td.global_count, allreduce_dtype=self.allreduce_dtype)       # an empty shard still steps
            elif n == 0:
                ran = False
            elif train:
                sess.run(net.optimizer, feed_dict={net.image_input: x, net.labels: y})
            else:
                if world > 1:
                    net.set_loss_normalizer(td.global_count / world)
                sess.run(net.eval_op, feed_dict={net.image_input: x, net.labels: y})
                if world > 1:
                    net.set_loss_normalizer(0.0)
            self.steps += int(ran)
            if pending_loss is not None:
                self.book(net.get_losses_step(1 if ran else 0), pending_loss, loss_summary)
            pending_loss = count if ran else None
            if train and self.grad_norms is not None:
                if pending_norm:
                    self.grad_norms.add(*net.get_grad_norm_step(1 if ran else 0))
                pending_norm = ran
            if not with_ap or n == 0:
                continue
            # decode + NMS of the batch just computed, on the GPU (train.py:275-277)
            launched = net.detect_last_launch(n, 0.5, 200, None)
            if isinstance(ap_calc, DeviceAPCalculator):
                ap_calc.add_pass(launched, gt_boxes)
            elif isinstance(ap_calc, DeviceCOCOEvaluator):
                ap_calc.add_pass(launched, self.coco_gt(gt_boxes), [net.preset.image_size] * n)
            drawn = self.annotate_launch(x, n, image_samples)
            if pending_det:
                self.collect(*pending_det, ap_calc, image_samples)
            pending_det = (launched, gt_boxes, drawn)
        if pending_loss is not None:
            self.book(net.get_losses_step(0), pending_loss, loss_summary)
        if pending_norm:
            self.grad_norms.add(*net.get_grad_norm_step(0))
        if pending_det:
            self.collect(*pending_det, ap_calc, image_samples)


def checkpoint_match(path):
    """The matching rule a checkpoint's run encoded its labels with (checkpoints from before the option: 'reference')."""
    with np.load(path, allow_pickle=False) as ck:
        return str(ck['__match__']) if '__match__' in ck.files else 'reference'


def checkpoint_loss(path):
    """(loss, gamma, alpha) a checkpoint's run trained with (checkpoints from before the option: 'mining')."""
    from .ssdvgg import checkpoint_loss as of
    with np.load(path, allow_pickle=False) as ck:
        return of(ck)


def checkpoint_loc_loss(path):
    """(localization loss, weight) a checkpoint's run trained with (checkpoints from before the option: 'smooth_l1')."""
    from .ssdvgg import checkpoint_loc_loss as of
    with np.load(path, allow_pickle=False) as ck:
        return of(ck)


def checkpoint_clip_norm(path):
    """--clip-norm of a checkpoint's run (checkpoints from before the option: 0, off)."""
    from .ssdvgg import checkpoint_clip_norm as of
    with np.load(path, allow_pickle=False) as ck:
        return of(ck)


def checkpoint_update_rule(path):
    """(--optimizer, beta1, beta2, eps, decay) of a checkpoint's run (a file without __optimizer__: a momentum run's)."""
    from .ssdvgg import checkpoint_update_rule as of
    with np.load(path, allow_pickle=False) as ck:
        return of(ck)


def checkpoint_ema(path):
    """--ema-decay of a checkpoint's run (a file without __ema_decay__: 0, no average)."""
    from .ssdvgg import checkpoint_ema as of
    with np.load(path, allow_pickle=False) as ck:
        return of(ck)


def resolved_weight_decay(weight_decay, optimizer):
    """--weight-decay as the run uses it: the value given, else the reference's 0.0005 under momentum and 0 under adamw, whose
    decay is the decoupled --adam-decay"""
    if weight_decay is not None:
        return weight_decay
    return 0.0005 if optimizer == 'momentum' else 0.0


def main(argv=None):
    parser = argparse.ArgumentParser(description='Train the SSD')
    parser.add_argument('--name', default='test', help='project name')
    parser.add_argument('--data-dir', default='synthetic', help='data directory')
    parser.add_argument('--vgg-dir', default='vgg_graph', help='directory for the VGG-16 model')
    parser.add_argument('--epochs', type=int, default=200, help='number of training epochs')
    parser.add_argument('--batch-size', type=int, default=8, help='batch size (per GPU)')
    parser.add_argument('--tensorboard-dir', default='tb', help='name of the summary data directory')
    parser.add_argument('--checkpoint-interval', type=int, default=5, help='checkpoint interval')
    parser.add_argument('--lr-values', type=str, default='0.00075;0.0001;0.00001', help='learning rate values')
    parser.add_argument('--lr-boundaries', type=str, default='320000;400000', help='learning rate chage boundaries (in batches)')
    parser.add_argument('--momentum', type=float, default=0.9, help='momentum for the optimizer')
    parser.add_argument('--weight-decay', type=float, default=None, help='L2 normalization factor (the term in the loss and the gradient); default: 0.0005 under --optimizer momentum, 0 under adamw')
    parser.add_argument('--optimizer', default='momentum', choices=['momentum', 'adamw'], help="the update rule: momentum = the reference's acc = m*acc + g; w -= lr*acc; adamw = AdamW on the GPU, exact in fp32, with a decoupled decay on the filters (DESIGN.md 35); composes with --clip-norm; --continue-training takes the checkpoint's")
    parser.add_argument('--adam-beta1', type=float, default=0.9, help='--optimizer adamw: decay rate of the first moment, in [0, 1)')
    parser.add_argument('--adam-beta2', type=float, default=0.999, help='--optimizer adamw: decay rate of the second moment, in [0, 1)')
    parser.add_argument('--adam-eps', type=float, default=1e-8, help='--optimizer adamw: the term added to the root of the second moment, > 0')
    parser.add_argument('--adam-decay', type=float, default=0.01, help='--optimizer adamw: the decoupled weight decay, w -= lr * decay * w on the filters, >= 0')
    parser.add_argument('--ema-decay', type=float, default=0.0, help='keep an exponential moving average of the weights on the GPU, updated behind every update with min(D, (1 + t) / (10 + t)): 0 = off; D in (0, 1), e.g. 0.999 = on -- validation, its AP and its annotated samples then run on the average and the checkpoints hold both sets (DESIGN.md 37); --continue-training takes the checkpoint\'s')
    parser.add_argument('--continue-training', type=str2bool, default='False', help='continue training from the latest checkpoint')
    parser.add_argument('--num-workers', type=int, default=0, help='number of parallel generators')
    parser.add_argument('--decoder', default='pillow', choices=['pillow', 'gpu'], help='a real --data-dir: pillow = the workers decode the files; gpu = they run the Huffman stage only and the GPU decodes in front of the augmentation kernel')
    parser.add_argument('--cache-gb', type=float, default=0, help='--decoder gpu: keep up to this many GB of decoded pictures in HBM; a cached picture costs no file read, no decode and no upload from its second epoch on (0 = off)')
    parser.add_argument('--mosaic', type=float, default=0.0, help='mosaic augmentation: the probability that a training sample becomes a 2 x 2 mosaic of its own picture and three partners, each through the train recipe, composed on the GPU (DESIGN.md 39); needs a real --data-dir or --augment true; 0 = off')
    parser.add_argument('--mosaic-center', type=float, nargs=2, default=[0.3, 0.7], metavar=('LO', 'HI'), help='--mosaic: the range of the mosaic centre, as fractions of the sample\'s sides')
    parser.add_argument('--mosaic-off-epochs', type=int, default=0, help='--mosaic: the last N epochs of the run train without mosaics')
    parser.add_argument('--preset', default='vgg300')
    parser.add_argument('--data-source', default='pascal_voc', help='data source module for a real --data-dir')
    add_ap_arguments(parser)
    parser.add_argument('--dtype', default='f32', choices=['f32', 'bf16'], help='f32, or bf16 activations on the bf16 matrix cores (fp32 master weights, loss and optimizer)')
    parser.add_argument('--a-trous', type=str2bool, default='True', help='a fresh run: the a-trous graph (true) or the fc graph with the whole fc6 / fc7 (false; weights from <vgg-dir>/vgg16_ssd_fc.npz); --continue-training takes the checkpoint\'s')
    parser.add_argument('--match', default='reference', choices=['reference', 'paper'], help="which ground-truth boxes get positive anchors: reference = only boxes some anchor overlaps with IoU > 0.5; paper = the SSD paper's matching, every box first gets the anchor it overlaps best (DESIGN.md 29); --continue-training takes the checkpoint's")
    parser.add_argument('--loss', default='mining', choices=['mining', 'focal'], help="mining = the reference's softmax cross entropy over the positives and 3x as many hard negatives; focal = the focal loss, every anchor contributes, damped by (1 - p_t)^gamma (DESIGN.md 30); --continue-training takes the checkpoint's")
    parser.add_argument('--focal-gamma', type=float, default=2.0, help='--loss focal: the focusing exponent, 0..5')
    parser.add_argument('--focal-alpha', type=float, default=0.25, help='--loss focal: the weight of a positive anchor (background: 1 - alpha), inside (0, 1)')
    parser.add_argument('--loc-loss', default='smooth_l1', choices=['smooth_l1', 'giou'], help="the box regression half of the loss: smooth_l1 = the reference's, on the four encoded offsets; giou = 1 - generalized IoU of the predicted against the ground-truth box of every positive anchor (DESIGN.md 31); goes with either --loss; --continue-training takes the checkpoint's")
    parser.add_argument('--loc-weight', type=float, default=1.0, help='--loc-loss giou: the factor on the localization term, a finite number > 0')
    parser.add_argument('--clip-norm', type=float, default=0.0, help="clip the gradient by its global norm in the update, on the GPU: 0 = off; X > 0 = scale an update whose gradient norm exceeds X down to X and skip one whose gradient is not finite; inf = measure the norm of every update and never clip (DESIGN.md 34); --continue-training takes the checkpoint's")
    parser.add_argument('--focal-prior', type=float, default=0.01, help='a fresh --loss focal run: the classifier biases start at a total object probability of this per anchor')
    parser.add_argument('--shapes-size', default='0.2;0.5', help="--data-dir shapes: smallest and largest side of a rectangle, as fractions of the frame")
    parser.add_argument('--synthetic-train', type=int, default=64, help='synthetic training samples per epoch')
    parser.add_argument('--synthetic-valid', type=int, default=16)
    parser.add_argument('--synthetic-classes', type=int, default=20, help='class count of the synthetic data sets (1..127)')
    parser.add_argument('--augment', type=str2bool, default='False', help="run the reference's train augmentation recipe (process_dataset.py) on the GPU over a uint8 synthetic dataset")
    parser.add_argument('--allreduce-dtype', default='f32', choices=['f32', 'bf16'], help='data parallel: bf16 = the filter gradients cross the links as bf16 messages of half the bytes (fp32 masters, momentum and arenas untouched)')
    parser.add_argument('--allreduce-bucket-mb', type=float, default=44, help='data parallel: all-reduce finished gradient ranges of >= this many MB while backward still runs (0 = one all-reduce after backward); 44 = three buckets: heads ... mod_conv6 | conv5_x + conv4_3/4_2 | the rest')
    args = parser.parse_args(argv)
    if args.mosaic and not (args.augment or args.data_dir not in (None, '', 'synthetic', 'shapes')):
        print('[!] --mosaic needs the transform path: a real --data-dir or --augment true'); return 1

    rank, local, world = parallel.init()
    import torch
    torch.cuda.set_device(local)           # every backend: kernels, .cuda() tensors and collectives of this rank on ITS GPU
    _lib.set_device(local)                 # ... and the package's free functions (label encoder, AP)
    say = print if rank == 0 else (lambda *a, **k: None)
    say('[i] Project name:         ', args.name)
    say('[i] Data directory:       ', args.data_dir)
    say('[i] # epochs:             ', args.epochs)
    say('[i] Batch size:           ', args.batch_size, 'x', world, 'GPU(s)')
    say('[i] Tensorboard directory:', args.tensorboard_dir)
    say('[i] Checkpoint interval:  ', args.checkpoint_interval)
    say('[i] Learning rate values: ', args.lr_values)
    say('[i] Learning rate boundaries: ', args.lr_boundaries)
    say('[i] Momentum:             ', args.momentum)
    say('[i] Continue:             ', args.continue_training)
    say('[i] Number of workers:    ', args.num_workers)
    say('[i] Decoder:              ', args.decoder)
    say('[i] Picture cache (GB):   ', args.cache_gb)

    try:
        lr_values = [float(v) for v in args.lr_values.split(';')]
        lr_boundaries = [int(v) for v in args.lr_boundaries.split(';')] if args.lr_boundaries else []
    except ValueError:
        print('[!] Learning rate values or boundaries are invalid'); return 1            # train.py:174-185
    if len(lr_values) != len(lr_boundaries) + 1:
        print('[!] Learning rate values must be one more than boundaries'); return 1

    # ---- find an existing checkpoint (train.py:99-134) ---------------------------------------
    start_epoch = 0
    ckpt = None
    if args.continue_training:
        cands = [f for f in (os.listdir(args.name) if os.path.isdir(args.name) else [])
                 if f.startswith('e') and f.endswith('.npz') and f[1:-4].isdigit()]
        if not cands:
            print('[!] No network state found in ' + args.name); return 1
        start_epoch = max(int(f[1:-4]) for f in cands)
        ckpt = os.path.join(args.name, f'e{start_epoch}.npz')
        say('[i] Last checkpoint:      ', ckpt)
        ck_match = checkpoint_match(ckpt)
        if ck_match != args.match:
            say("[i] --match %s disagrees with the checkpoint: continuing with its rule, '%s'" % (args.match, ck_match))
            args.match = ck_match
        ck_loss = checkpoint_loss(ckpt)
        asked = (args.loss, args.focal_gamma, args.focal_alpha) if args.loss == 'focal' else (args.loss,)
        if asked != ck_loss[:len(asked)]:
            say("[i] --loss %s disagrees with the checkpoint: continuing with its loss, '%s'" % (args.loss, ck_loss[0]))
        args.loss, args.focal_gamma, args.focal_alpha = ck_loss
        ck_loc = checkpoint_loc_loss(ckpt)
        asked = (args.loc_loss, args.loc_weight) if args.loc_loss != 'smooth_l1' else (args.loc_loss,)
        if asked != ck_loc[:len(asked)]:
            say("[i] --loc-loss %s disagrees with the checkpoint: continuing with its localization loss, '%s'" % (args.loc_loss, ck_loc[0]))
        args.loc_loss, args.loc_weight = ck_loc
        ck_clip = checkpoint_clip_norm(ckpt)
        if args.clip_norm != 0.0 and args.clip_norm != ck_clip:
            say("[i] --clip-norm %g disagrees with the checkpoint: continuing with its value, %g" % (args.clip_norm, ck_clip))
        args.clip_norm = ck_clip
        ck_rule = checkpoint_update_rule(ckpt)
        asked = (args.optimizer,) + tuple(float(np.float32(x)) for x in (args.adam_beta1, args.adam_beta2, args.adam_eps, args.adam_decay))
        if args.optimizer != 'momentum' and asked != ck_rule:
            say("[i] --optimizer %s disagrees with the checkpoint: continuing with its rule, '%s'" % (args.optimizer, ck_rule[0]))
        args.optimizer, args.adam_beta1, args.adam_beta2, args.adam_eps, args.adam_decay = ck_rule
        ck_ema = checkpoint_ema(ckpt)
        if args.ema_decay != 0.0 and float(np.float32(args.ema_decay)) != ck_ema:
            say("[i] --ema-decay %g disagrees with the checkpoint: continuing with its value, %g" % (args.ema_decay, ck_ema))
        args.ema_decay = ck_ema
    elif rank == 0:
        try:
            os.makedirs(args.name, exist_ok=True)
        except OSError as e:
            print('[!] Cannot create directory {}: {}'.format(args.name, e)); return 1      # train.py:143-145

    say('[i] Matching rule:        ', args.match)
    try:
        from .ssdvgg import loss_config, loc_loss_config, grad_clip_config
        loss_config(args.loss, args.focal_gamma, args.focal_alpha)
        loc_loss_config(args.loc_loss, args.loc_weight)
        if args.loss == 'focal' and not 0.0 < args.focal_prior < 1.0:
            raise ValueError('--focal-prior must lie in (0, 1)')
    except ValueError as e:
        print('[!] Bad loss:', str(e)); return 1
    try:
        grad_clip_config(args.clip_norm)
    except ValueError as e:
        print('[!] Bad --clip-norm:', str(e)); return 1
    try:
        from .ssdvgg import update_rule_config
        update_rule_config(args.optimizer, args.adam_beta1, args.adam_beta2, args.adam_eps, args.adam_decay)
    except ValueError as e:
        print('[!] Bad --optimizer:', str(e)); return 1
    try:
        from .ssdvgg import ema_decay_config
        args.ema_decay = ema_decay_config(args.ema_decay)
    except ValueError as e:
        print('[!] Bad --ema-decay:', str(e)); return 1
    args.weight_decay = resolved_weight_decay(args.weight_decay, args.optimizer)
    say('[i] Update rule:          ', args.optimizer if args.optimizer == 'momentum' else '%s (beta1 %g, beta2 %g, eps %g)' % (
        args.optimizer, args.adam_beta1, args.adam_beta2, args.adam_eps))
    say('[i] Weight decay:         ', args.weight_decay, '(L2 term of the loss)')
    say('[i] Decoupled decay:      ', '%g' % args.adam_decay if args.optimizer == 'adamw' else 'none')
    say('[i] Loss:                 ', args.loss if args.loss != 'focal' else 'focal (gamma %g, alpha %g)' % (args.focal_gamma, args.focal_alpha))
    say('[i] Localization loss:    ', args.loc_loss if args.loc_loss == 'smooth_l1' else '%s (weight %g)' % (args.loc_loss, args.loc_weight))
    say('[i] Gradient clipping:    ', 'off' if args.clip_norm == 0 else 'norm measured, never clipped' if math.isinf(args.clip_norm) else 'global norm <= %g' % args.clip_norm)
    say('[i] Weight EMA:           ', 'off' if args.ema_decay == 0 else 'decay %g; validation and its AP run on the average' % args.ema_decay)
    if args.cache_gb < 0 or (args.cache_gb and args.decoder != 'gpu'):
        print('[!] --cache-gb keeps pictures decoded on the GPU: it needs --decoder gpu and a size >= 0'); return 1
    say('[i] Mosaic:               ', 'off' if not args.mosaic else 'probability %g, centre in %g..%g of the sides, off in the last %d epochs' % (
        args.mosaic, args.mosaic_center[0], args.mosaic_center[1], args.mosaic_off_epochs))
    try:
        td = TrainingData(args.data_dir, args.preset, args.synthetic_train, args.synthetic_valid, rank=rank, world=world,
                          augment=args.augment, device=local, data_source=args.data_source,
                          synthetic_classes=args.synthetic_classes, decoder=args.decoder, cache_bytes=int(args.cache_gb * 1e9), match=args.match,
                          shapes_size=[float(v) for v in args.shapes_size.split(';')], mosaic=args.mosaic, mosaic_center=tuple(args.mosaic_center),
                          mosaic_off_epochs=args.mosaic_off_epochs, epochs=args.epochs)
    except (RuntimeError, ValueError) as e:
        print('[!] Unable to load training data:', str(e)); return 1                       # train.py:155-161
    say('[i] # training samples:   ', td.num_train)
    say('[i] # validation samples: ', td.num_valid)
    say('[i] # classes:            ', td.num_classes)
    say('[i] Image size:           ', td.preset.image_size)

    class_names = [td.lid2name[i] for i in range(td.num_classes)]
    lr = compute_lr(lr_values, lr_boundaries)
    bucket = int(args.allreduce_bucket_mb * 1e6 / 4)
    dev = torch.device('cuda', local)

    def rank_sum(values):
        if world <= 1:
            return list(values)
        t = torch.tensor(list(values), dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t)
        return t.tolist()

    with Session(local) as sess:
        say('[i] Creating the model...')
        net = SSDVGG(sess, td.preset)
        if ckpt:
            net.build_from_metagraph(None, ckpt, max_batch=args.batch_size, training=True, dtype=args.dtype)
            net.build_optimizer_from_metagraph()
        else:
            net.build_from_vgg(args.vgg_dir, td.num_classes, a_trous=args.a_trous, max_batch=args.batch_size, dtype=args.dtype,
                               background_prior=args.focal_prior if args.loss == 'focal' else None)
            net.build_optimizer(learning_rate=lr, weight_decay=args.weight_decay, momentum=args.momentum, loss=args.loss,
                                focal_gamma=args.focal_gamma, focal_alpha=args.focal_alpha, loc_loss=args.loc_loss,
                                loc_weight=args.loc_weight, clip_norm=args.clip_norm, optimizer=args.optimizer,
                                adam_beta1=args.adam_beta1, adam_beta2=args.adam_beta2, adam_eps=args.adam_eps,
                                adam_decay=args.adam_decay)
        if world > 1:
            torch.distributed.broadcast(net.params_flat, 0)
        net.set_stream(torch.cuda.current_stream().cuda_stream)
        if not ckpt and args.ema_decay != 0.0:
            # a fresh run's average starts here, one rank or many alike: from the weights every rank holds behind the broadcast, on
            # the stream the steps will run on (a continued run's came from the file, build_optimizer_from_metagraph)
            torch.cuda.synchronize()
            net.set_ema(args.ema_decay)

        writer = SummaryWriter(os.path.join(args.tensorboard_dir, os.path.basename(os.path.normpath(args.name)))) if rank == 0 else None
        if args.ap_protocol == 'coco':      # COCO's box AP / AR; the per-class values are AP averaged over 0.50:0.95
            if args.ap_on == 'gpu':
                training_ap_calc, validation_ap_calc = DeviceCOCOEvaluator(local, td.num_classes), DeviceCOCOEvaluator(local, td.num_classes)
            else:
                training_ap_calc, validation_ap_calc = COCOEvaluator(num_classes=td.num_classes), COCOEvaluator(num_classes=td.num_classes)
        elif args.ap_on == 'gpu':       # the detections stay on the GPU between the decode and the AP kernels
            training_ap_calc = DeviceAPCalculator(local, td.num_classes, args.ap_protocol)
            validation_ap_calc = DeviceAPCalculator(local, td.num_classes, args.ap_protocol)
        else:
            training_ap_calc = APCalculator(protocol=args.ap_protocol)
            validation_ap_calc = APCalculator(protocol=args.ap_protocol)
        labels = list(td.lname2id.keys())
        # with a weight EMA the validation epoch runs on the average (averaged_weights below) and its summaries say so; the training
        # epoch's numbers are collected from the training steps, on the raw weights
        valid_name = 'validation (averaged)' if net.get_ema()[0] != 0.0 else 'validation'
        training_ap = PrecisionSummary(writer, 'training', labels)
        validation_ap = PrecisionSummary(writer, valid_name, labels)
        training_loss = LossSummary(writer, 'training', td.num_train)
        validation_loss = LossSummary(writer, valid_name, td.num_valid)
        training_imgs = ImageSummary(writer, 'training', td.label_colors, td.lid2name) if rank == 0 else None      # train.py:248-249
        validation_imgs = ImageSummary(writer, valid_name, td.label_colors, td.lid2name) if rank == 0 else None

        loop = StepLoop(net, sess, td, args.batch_size, args.num_workers, world, rank, bucket, args.allreduce_dtype)
        if net.get_grad_clip() != 0.0:      # every rank holds the same arena: the same norms; rank 0 writes them
            loop.grad_norms = GradNormSummary(writer, net.global_step)

        def gathered_aps(calc, with_summary=False):
            """{label: AP} over the WHOLE sample (train.py:317-323): data parallel, every rank's detections and ground
            truth are gathered to rank 0, which computes; the other ranks get {}."""
            def aps(c):
                if not isinstance(c, (COCOEvaluator, DeviceCOCOEvaluator)):
                    return c.compute_aps()
                result = c.compute()      # one evaluation for the per-class values and the twelve numbers
                if with_summary:
                    say(format_summary(summarize(result), c.thresholds))
                return aps_of(result)

            if world <= 1:
                return aps(calc)
            states = [None] * world if rank == 0 else None
            torch.distributed.gather_object(calc.state(), states, dst=0)
            if rank != 0:
                return {}
            if isinstance(calc, DeviceCOCOEvaluator):
                merged = DeviceCOCOEvaluator(calc.device, calc.num_classes, calc.thresholds)
            elif isinstance(calc, COCOEvaluator):
                merged = COCOEvaluator(calc.thresholds, calc.num_classes)
            elif isinstance(calc, DeviceAPCalculator):
                merged = DeviceAPCalculator(calc.device, calc.num_classes, calc.protocol, calc.minoverlap)
            else:
                merged = APCalculator(calc.minoverlap, calc.protocol)
            for st in states:
                merged.merge(st)
            return aps(merged)

        say('[i] Training...')
        for e in range(start_epoch, args.epochs):
            td.epoch = e
            loop.run_epoch(td.train_generator, True, training_loss, training_ap_calc, e > 0, training_imgs)
            fs = dict(td.feeder_stats)        # (of the training generator: the validation generator replaces them)
            with net.averaged_weights():      # (nothing without --ema-decay)
                loop.run_epoch(td.valid_generator, False, validation_loss, validation_ap_calc, e > 0, validation_imgs)
            # ---- summaries (train.py:311-331) -----------------------------------------------------
            tl = training_loss.push(e + 1, rank_sum)
            vl = validation_loss.push(e + 1, rank_sum)
            say('[i] Train {:>2}/{}  total {:.4f}  localization {:.4f}  confidence {:.4f}  l2 {:.4f}'.format(
                e + 1, args.epochs, tl['total'], tl['localization'], tl['confidence'], tl['l2']))
            say('[i] Valid {:>2}/{}  total {:.4f}  localization {:.4f}  confidence {:.4f}  l2 {:.4f}'.format(
                e + 1, args.epochs, vl['total'], vl['localization'], vl['confidence'], vl['l2']))
            if args.mosaic:
                say('[i] Feed  {:>2}/{}  decoded {}  fallbacks {}  cache hits {}  mosaics {}  cells {}  area fallbacks {}'.format(
                    e + 1, args.epochs, fs.get('decoded', 0), fs.get('fallbacks', 0), fs.get('cache_hits', 0), fs.get('mosaics', 0), fs.get('cells', 0),
                    fs.get('area_fallbacks', 0)))
            if loop.grad_norms is not None:
                gn = loop.grad_norms.push(e + 1)
                say('[i] Grad  {:>2}/{}  norm median {:.4g}  max {:.4g}  clipped {}  skipped {}  of {} updates'.format(
                    e + 1, args.epochs, gn['median'], gn['max'], gn['clipped'], gn['skipped'], gn['updates']))
            # VOC07 11-point AP on the GPU, over all ranks' samples
            APs = gathered_aps(training_ap_calc); mAP = APs2mAP(APs)
            training_ap.push(e + 1, mAP, APs)
            vAPs = gathered_aps(validation_ap_calc, e > 0); vmAP = APs2mAP(vAPs)      # (coco: the validation's twelve numbers too)
            validation_ap.push(e + 1, vmAP, vAPs)
            if e > 0:
                say('[i] mAP  {:>2}/{}  training {:.4f}  {} {:.4f}'.format(e + 1, args.epochs, mAP, valid_name, vmAP))
            if rank == 0:                                                                       # train.py:328-329
                training_imgs.push(e + 1)
                validation_imgs.push(e + 1)
            training_ap_calc.clear(); validation_ap_calc.clear()
            if writer is not None:
                writer.flush()
            # ---- checkpoint (train.py:336-343) -------------------------------------------------
            if (e + 1) % args.checkpoint_interval == 0 and rank == 0:
                path = '{}/e{}.npz'.format(args.name, e + 1)
                net.save_checkpoint(path, lr, args.momentum, args.weight_decay, class_names=class_names, match=args.match)
                print('[i] Checkpoint saved:', path)
        if rank == 0:
            path = '{}/final.npz'.format(args.name)
            net.save_checkpoint(path, lr, args.momentum, args.weight_decay, class_names=class_names, match=args.match)
            print('[i] Checkpoint saved:', path)
        if writer is not None:
            writer.close()
        if rank == 0:
            training_imgs.close(); validation_imgs.close()
        td.close()
        if os.environ.get('SSD_PRINT_CHECKSUM'):      # replica agreement check of the multi-rank tests
            print('[checksum] rank %d step %d params %.12e' % (rank, net.global_step, float(net.params_flat.double().sum())), flush=True)
    if world > 1:
        torch.distributed.barrier()
    return 0


if __name__ == '__main__':
    sys.exit(main())
