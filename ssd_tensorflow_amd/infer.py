#!/usr/bin/env python3
"""Inference driver: the counterpart of the reference's infer.py loop (infer.py:213-280) over the
HIP library: restore a checkpoint, batch images, run the net, decode + NMS, keep [:200], AP statistics,
VOC summary files.  Same flags (infer.py:62-89) plus --synthetic / --preset / --dtype.

The loop is pipelined: images are resized on the GPU (the augmentation kernel's cv2.INTER_LINEAR path),
the net and decode + NMS run on the result where it lies, and the (small) detections of batch k are
collected after batch k+1 has been launched -- the [b, A, C+5] predictions only come to the host for
--dump-predictions.  Files: anything Pillow decodes, or .npy arrays (uint8 / float32 BGR).  --decoder gpu (the default) decodes baseline
JPEGs on the GPU instead (jpeg.py; same pixels; --decoder pillow: the host decode).  --annotate draws the
detections on the original-size image on the GPU, from the source bytes the resize was fed with and the decode's
device-visible output (annotate.py), and writes it to <output-dir>/<basename>.
"""
import argparse
import json
import os
import sys

import numpy as np

from .average_precision import APCalculator, DeviceAPCalculator, APs2mAP, add_ap_arguments
from .coco_eval import COCOEvaluator, DeviceCOCOEvaluator, aps_of, format_summary, summarize
from .ssdvgg import SSDVGG, Session, checkpoint_has_ema, NO_EMA_IN_FILE
from .ssdutils import get_preset_by_name, boxes_from_detection
from .training_data import default_class_names
from .pascal_summary import PascalSummary
from .utils import Size, Sample, Box, Point, str2bool, load_data_source, default_colors, prop2abs


def _has_jpeg_candidates(files):
    """the batch is for jpeg.decode_batch: all items are files, at least one of them is not a .npy array (a batch of arrays
    alone is packed and uploaded as before), and the arrays among them are uint8"""
    if not all(isinstance(f, str) for f in files):
        return False
    arrays = [f if f.endswith('.npy') else f + '.npy' for f in files if f.endswith('.npy') or os.path.exists(f + '.npy')]
    return len(arrays) < len(files) and all(np.load(a, mmap_mode='r').dtype == np.uint8 for a in arrays)


def sample_generator(samples, image_size, batch_size, device=0, with_sources=False, decoder='pillow', decoder_entropy='host'):
    """infer.py:44-54: cv2.resize(cv2.imread(file), image_size).astype(float32) per batch -- here a batch of load +
    INTER_LINEAR resize plans executed by the augmentation kernel; yields (CUDA tensor [b,H,W,3], indices, sizes).
    with_sources: a fourth item (device tensor, byte offsets, [(h, w)]) of the pixels to draw on: the packed original-size
    uint8 images the resize read, or, for float inputs, the network-size batch itself.
    decoder='gpu': a batch of files is decoded by jpeg.decode_batch (baseline JPEGs on the GPU, anything else loaded as before
    and copied into the same device buffer), the resize plans read that buffer and it is also the buffer to draw on; the pixels
    never exist on the host; decoder_entropy='gpu': the Huffman stage of that decode runs on the GPU too.  Batches of arrays alone (--synthetic, .npy files) take the path below either way."""
    from . import transforms as T
    for offset in range(0, len(samples), batch_size):
        files = samples[offset:offset + batch_size]
        if decoder == 'gpu' and _has_jpeg_candidates(files):
            from . import jpeg
            packed, offs, shapes, _ = jpeg.decode_batch(files, device=device, entropy=decoder_entropy)
            plans = []
            for i in range(len(files)):
                plan = T.ImagePlan((packed, offs[i], shapes[i]))
                plan.resize = (image_size.w, image_size.h, T.INTER_LINEAR)
                plans.append(plan)
            x = T.augment_batch(plans, image_size.w, image_size.h, device=device)
            idxs = list(range(offset, offset + len(files)))
            sizes = [Size(w, h) for h, w in shapes]
            if with_sources:
                yield x, idxs, sizes, (packed, offs, shapes)
            else:
                yield x, idxs, sizes
            continue
        plans, idxs, sizes, ready = [], [], [], []
        for i, f in enumerate(files):
            img = f if isinstance(f, np.ndarray) else T.load_image_bgr(f)
            idxs.append(offset + i)
            sizes.append(Size(img.shape[1], img.shape[0]))
            if img.dtype == np.uint8:
                plan = T.ImagePlan(img)
                plan.resize = (image_size.w, image_size.h, T.INTER_LINEAR)
                plans.append(plan); ready.append(None)
            else:       # a float image is fed as it is (the reference's resize would run on uint8 pixels)
                if img.shape[:2] != (image_size.h, image_size.w):
                    raise ValueError(f'{f}: float images must already be {image_size.h}x{image_size.w}, got {img.shape[:2]}')
                ready.append(np.ascontiguousarray(img, np.float32))
        import torch
        dev = torch.device('cuda', device)
        x = torch.empty((len(files), image_size.h, image_size.w, 3), dtype=torch.float32, device=dev)
        sources = None
        if with_sources and plans and len(plans) != len(files):
            raise ValueError('uint8 and float images cannot share an annotated batch')
        if plans:
            res = T.augment_batch(plans, image_size.w, image_size.h, device=device, return_images=with_sources)
            if with_sources:
                res, packed, offs = res
                sources = (packed, offs, [(s.h, s.w) for s in sizes])
            k = 0
            for i, r in enumerate(ready):
                if r is None:
                    x[i] = res[k]; k += 1
        for i, r in enumerate(ready):
            if r is not None:
                x[i] = torch.from_numpy(r).to(dev)
        if with_sources:
            if sources is None:
                n = image_size.h * image_size.w * 12
                sources = (x, [i * n for i in range(len(files))], [(image_size.h, image_size.w)] * len(files))
            yield x, idxs, sizes, sources
        else:
            yield x, idxs, sizes


def add_fp8_arguments(parser):
    """--fp8-calibration / --fp8-calibrate-images of the deployment tools (their --dtype fp8)"""
    parser.add_argument('--fp8-calibration', default=None, metavar='FILE.npz',
                        help='--dtype fp8: activation scales; loaded if the file exists, else written after calibrating on the first inputs')
    parser.add_argument('--fp8-calibrate-images', type=int, default=32,
                        help='--dtype fp8 without stored scales: this many of the first inputs calibrate the net before the first inference')


def check_fp8_arguments(parser, args):
    """--fp8-calibration with --dtype mxfp8 or mxfp6 is an argument error: such a net has nothing to calibrate"""
    if args.dtype in ('mxfp8', 'mxfp6') and args.fp8_calibration:
        parser.error('--fp8-calibration does not apply to --dtype %s: an %s net has no calibration scales' % (args.dtype, args.dtype))


def fp8_batches(net, batches, calibration_file=None, calibrate_images=32):
    """The batches of sample_generator, unchanged, for a net that is not fp8 (an mxfp8 net among them: it needs no scales).  For an fp8 net the scales are in place before the
    first batch is handed on: from calibration_file if it exists, else from the first calibrate_images inputs (whole batches
    are held back for that and handed on afterwards, so every input is still inferred), written to calibration_file if given."""
    if getattr(net, 'dtype', None) != 'fp8':
        yield from batches
        return
    if calibration_file and os.path.exists(calibration_file):
        with np.load(calibration_file, allow_pickle=False) as f:
            net.fp8_scales = {k: float(f[k]) for k in f.files}
        print('[i] fp8 scales:         loaded from', calibration_file)
        yield from batches
        return
    held, seen = [], 0
    batches = iter(batches)
    for batch in batches:
        take = min(batch[0].shape[0], max(int(calibrate_images), 1) - seen)
        net.calibrate_fp8(batch[0][:take], accumulate=seen > 0)
        held.append(batch)
        seen += take
        if seen >= calibrate_images:
            break
    if not held:
        return
    print('[i] fp8 scales:         calibrated on the first', seen, 'inputs')
    if calibration_file:
        with open(calibration_file, 'wb') as f:      # (a file object: numpy leaves the name as given)
            np.savez(f, **net.fp8_scales)
    yield from held
    yield from batches


def add_decode_arguments(parser):
    """--decode / --nms-top-k / --keep-top-k of the deployment tools"""
    parser.add_argument('--decode', default='argmax', choices=['argmax', 'all'],
                        help="argmax: the reference's decode, one candidate per anchor (its best class); all: the SSD paper's DetectionOutput, "
                             'every class of an anchor above the threshold is a candidate, the best --nms-top-k per class go through NMS and '
                             'the best --keep-top-k of the image are kept, in confidence order')
    parser.add_argument('--nms-top-k', type=int, default=400, help='--decode all: candidates per class that enter NMS (1..1024)')
    parser.add_argument('--keep-top-k', type=int, default=200, help='--decode all: detections kept per image (1..1024)')
    parser.add_argument('--soft-nms', default='off', choices=['off', 'linear', 'gaussian'],
                        help='--decode all (with --tile: --tile-decode all): Soft-NMS in the place of the NMS per class. A box that overlaps a '
                             'better one of its class keeps a lower confidence instead of being deleted: linear: times 1 - IoU above '
                             '--soft-nms-iou; gaussian: times exp(-IoU^2 / --soft-nms-sigma). The picks are re-ranked after every decay and '
                             'end below --soft-nms-min-score; the reported confidence is the decayed one (DESIGN.md 38)')
    parser.add_argument('--soft-nms-iou', type=float, default=0.45, help='--soft-nms linear: overlaps above it decay the score (0..1)')
    parser.add_argument('--soft-nms-sigma', type=float, default=0.5, help='--soft-nms gaussian: the width of the decay (> 0)')
    parser.add_argument('--soft-nms-min-score', type=float, default=None,
                        help='--soft-nms: a candidate whose decayed score falls below it is dropped (default: --threshold)')


def check_decode_arguments(parser, args):
    """--decode all with --tile is an argument error: the tile merge takes one record per anchor"""
    if args.soft_nms != 'off':
        if args.tile and args.tile_decode != 'all':
            parser.error('--soft-nms %s needs --tile-decode all with --tile: the argmax decode of the windows keeps the hard rule' % args.soft_nms)
        if not args.tile and args.decode != 'all':
            parser.error('--soft-nms %s needs --decode all: the argmax decode keeps the hard rule' % args.soft_nms)
        if not 0.0 <= args.soft_nms_iou <= 1.0:
            parser.error('--soft-nms-iou must be in 0..1')
        if not (args.soft_nms_sigma > 0.0 and args.soft_nms_sigma < float('inf')):
            parser.error('--soft-nms-sigma must be finite and > 0')
        if args.soft_nms_min_score is not None and not 0.0 <= args.soft_nms_min_score < float('inf'):
            parser.error('--soft-nms-min-score must be finite and >= 0')
    if args.decode == 'all' and args.tile:
        parser.error('--decode all does not apply to --tile: the tile merge takes one record per anchor (use --decode argmax)')
    for name in ('nms_top_k', 'keep_top_k'):
        if args.decode == 'all' and not 1 <= getattr(args, name) <= 1024:
            parser.error('--%s must be in 1..1024' % name.replace('_', '-'))


def decode_keywords(args):
    """the decode keywords of SSDVGG.detect_last_launch for these arguments"""
    if args.decode == 'all':
        return dict(decode='all', nms_top_k=args.nms_top_k, keep_top_k=args.keep_top_k, **soft_nms_keywords(args))
    return {}


def soft_nms_keywords(args):
    """the four soft_nms keywords of the decode entry points for --soft-nms and its companions"""
    if getattr(args, 'soft_nms', 'off') == 'off':
        return {}
    return dict(soft_nms=args.soft_nms, soft_nms_iou=args.soft_nms_iou, soft_nms_sigma=args.soft_nms_sigma,
                soft_nms_min_score=args.soft_nms_min_score)


def nms_rule_text(args):
    """what the banner's decode line adds for the suppression rule (nothing for the hard rule: the line stays as it was)"""
    if getattr(args, 'soft_nms', 'off') == 'off':
        return ''
    min_score = 'the threshold' if args.soft_nms_min_score is None else '%g' % args.soft_nms_min_score
    if args.soft_nms == 'linear':
        return ', soft nms linear, iou %g, min score %s' % (args.soft_nms_iou, min_score)
    return ', soft nms gaussian, sigma %g, min score %s' % (args.soft_nms_sigma, min_score)


def resolve_class_names(num_classes, source_names=None, stored=None):
    """{class id: name}: the data source's names, else the checkpoint's __class_names__, else (a checkpoint written before
    names were stored, or no checkpoint) the VOC names for 20 classes and 'class_<id>' otherwise."""
    if source_names is not None:
        return dict(source_names)
    if stored is not None:
        return {i: str(n) for i, n in enumerate(stored)}
    return dict(enumerate(default_class_names(num_classes)))


def synthetic_ground_truth(n, boxes_per_image, num_classes, lid2name, size):
    """--synthetic-boxes: seeded ground truth for the --synthetic images, so that the AP path runs without a data set"""
    rng = np.random.default_rng(2)
    samples = []
    for i in range(n):
        boxes = []
        for _ in range(boxes_per_image):
            k = int(rng.integers(0, num_classes))
            w, h = (float(v) for v in rng.uniform(0.1, 0.5, 2))
            cx, cy = float(rng.uniform(w / 2, 1 - w / 2)), float(rng.uniform(h / 2, 1 - h / 2))
            boxes.append(Box(lid2name.get(k, 'class_%d' % k), k, Point(cx, cy), Size(w, h)))
        samples.append(Sample('%06d.npy' % i, boxes, size))
    return samples


def coco_image_id(source, filename):
    """source.image_ids is keyed by the annotation's file_name: usually the path's last component, but it may carry a directory"""
    name = os.path.basename(filename)
    if name in source.image_ids:
        return source.image_ids[name]
    path = filename.replace(os.sep, '/')
    for key, image_id in source.image_ids.items():
        if path.endswith('/' + key):
            return image_id
    raise RuntimeError('--coco-results: the data source has no image id for ' + filename)


def coco_result_records(source, sample, boxes):
    """The records of one image's detections in COCO's results format: bbox [x, y, w, h] in pixels from the 1000-grid box."""
    image_id = coco_image_id(source, sample.filename)
    sx, sy = sample.imgsize.w / 1000.0, sample.imgsize.h / 1000.0
    out = []
    for conf, box in boxes:
        xmin, xmax, ymin, ymax = prop2abs(box.center, box.size, Size(1000, 1000))
        out.append(dict(image_id=image_id, category_id=source.category_ids[box.labelid],
                        bbox=[xmin * sx, ymin * sy, (xmax - xmin) * sx, (ymax - ymin) * sy], score=float(conf)))
    return out


def main(argv=None):
    parser = argparse.ArgumentParser(description='SSD inference')
    parser.add_argument('files', type=str, nargs='*', help='image files (anything Pillow decodes, or .npy arrays)')
    parser.add_argument('--name', default='test', help='project name')
    parser.add_argument('--checkpoint', type=int, default=-1, help='checkpoint to restore; -1 is the most recent')
    parser.add_argument('--training-data', default='', help='unused: class names come from the data source (VOC defaults)')
    parser.add_argument('--output-dir', default='test-output', help='directory for the resulting predictions')
    parser.add_argument('--annotate', type=str2bool, default='False', help='write the images with the detections drawn on them')
    parser.add_argument('--dump-predictions', type=str2bool, default='False', help='Dump raw predictions')
    parser.add_argument('--compute-stats', type=str2bool, default='True', help='Compute the mAP stats')
    parser.add_argument('--data-source', default=None, help='Use test files from the data source')
    parser.add_argument('--data-dir', default='pascal-voc', help='Use test files from the data source')
    parser.add_argument('--batch-size', type=int, default=32, help='batch size')
    parser.add_argument('--sample', default='test', choices=['test', 'trainval'], help='sample to run on')
    parser.add_argument('--threshold', type=float, default=0.5, help='confidence threshold')
    parser.add_argument('--pascal-summary', type=str2bool, default='False', help='dump the detections in Pascal VOC format')
    parser.add_argument('--synthetic', type=int, default=0, help='run on N synthetic images instead of files')
    parser.add_argument('--synthetic-boxes', type=int, default=0, help='--synthetic: this many seeded ground-truth boxes per image, and the mAP stats over them')
    parser.add_argument('--preset', default=None, help='preset when no checkpoint is given (random weights)')
    parser.add_argument('--num-classes', type=int, default=20, help='class count when no checkpoint is given (1..127)')
    parser.add_argument('--a-trous', type=str2bool, default='True', help='graph when no checkpoint is given: a-trous (true) or fc (false); a checkpoint carries its own')
    parser.add_argument('--dtype', default='f32', choices=['f32', 'bf16', 'fp8', 'mxfp8', 'mxfp6'],
                        help='f32, bf16 activations on the bf16 matrix cores, fp8: the bf16 net with conv3_2 ... mod_conv7 on e4m3 operands '
                             '(calibrated scales), or mxfp8: the same layers with block scales chosen from the data (no calibration; the fc graph\'s 7x7 fc6 joins '
                             'them when the environment has SSD_MXFP8_BIGK=1), or mxfp6: the mxfp8 layers on 6-bit e2m3 operands with block scales on '
                             'activations and filters (no calibration; fc6 stays on bf16)')
    parser.add_argument('--weights', default='auto', choices=['auto', 'raw', 'ema'],
                        help="a checkpoint of a run with --ema-decay holds two sets of weights: raw = the last iterate; ema = the average (an error "
                             "if the file has none); auto = the average where the file has one.  Every --dtype, and fp8's calibration, runs on the chosen set")
    add_fp8_arguments(parser)
    add_ap_arguments(parser)
    parser.add_argument('--coco-results', default=None, metavar='FILE',
                        help="write the run's detections as a COCO results JSON (image_id, category_id, bbox [x, y, w, h] in pixels, score); "
                             'needs a data source that keeps the annotation file\'s ids (coco)')
    parser.add_argument('--decoder', default='gpu', choices=['pillow', 'gpu'],
                        help='gpu: baseline JPEGs are decoded on the GPU, other files as with pillow (same pixels); pillow: every file is decoded on the host')
    parser.add_argument('--decoder-entropy', default='host', choices=['host', 'gpu'],
                        help='--decoder gpu: host: Huffman decoding on host threads; gpu: on the GPU as well, only the files\' bytes go to the device (same pixels)')
    parser.add_argument('--encoder', default='pillow', choices=['pillow', 'gpu'],
                        help='--annotate: gpu: pictures named .jpg / .jpeg are encoded as baseline JPEG on the GPU (what cv2.imwrite writes), other names as with pillow; pillow: every picture is encoded on the host')
    parser.add_argument('--jpeg-quality', type=int, default=95, help='--encoder gpu: JPEG quality 1..100 (95 = cv2.imwrite)')
    parser.add_argument('--jpeg-entropy', default='host', choices=['host', 'gpu'],
                        help='--encoder gpu: host: Huffman coding on host threads; gpu: on the GPU as well, only the files come back (same bytes)')
    from .tiling import add_arguments as add_tile_arguments, check_arguments as check_tile_arguments
    add_tile_arguments(parser)
    add_decode_arguments(parser)
    args = parser.parse_args(argv)
    check_fp8_arguments(parser, args)
    check_decode_arguments(parser, args)
    check_tile_arguments(parser, args)
    if args.tile and args.dump_predictions:
        parser.error('--dump-predictions does not apply to --tile: a tiled picture has one prediction tensor per window')
    if args.tile and args.synthetic:
        parser.error('--synthetic inputs are network-size float arrays: --tile reads source pictures')

    print('[i] Project name:      ', args.name)
    print('[i] Batch size:        ', args.batch_size)
    print('[i] Data source:       ', args.data_source)
    print('[i] Data directory:    ', args.data_dir)
    print('[i] Output directory:  ', args.output_dir)
    print('[i] Dump predictions:  ', args.dump_predictions)
    print('[i] Sample:            ', args.sample)
    print('[i] Threshold:         ', args.threshold)
    print('[i] Pascal summary:    ', args.pascal_summary)
    print('[i] Annotate:          ', args.annotate)
    if args.tile_decode != 'argmax':
        print('[i] Tile decode:       ', '%s (nms top k %d, keep top k %d%s)' % (args.tile_decode, args.nms_top_k, args.keep_top_k,
                                                                                   nms_rule_text(args)))
    if args.decode != 'argmax':
        print('[i] Decode:            ', '%s (nms top k %d, keep top k %d%s)' % (args.decode, args.nms_top_k, args.keep_top_k, nms_rule_text(args)))

    # ---- checkpoint lookup (infer.py:111-126) --------------------------------------------------
    ckpt = None
    if os.path.isdir(args.name):
        if args.checkpoint == -1:
            cands = [f for f in os.listdir(args.name) if f.endswith('.npz')]
            epochs = sorted((f for f in cands if f[0] == 'e' and f[1:-4].isdigit()), key=lambda f: int(f[1:-4]))
            ckpt = os.path.join(args.name, 'final.npz') if 'final.npz' in cands else (os.path.join(args.name, epochs[-1]) if epochs else None)
        else:
            ckpt = '{}/e{}.npz'.format(args.name, args.checkpoint)
    if ckpt is None or not os.path.exists(ckpt):
        if args.preset is None:
            if ckpt is None:
                print('[!] No network state found in ' + args.name)
            else:
                print('[!] Cannot find checkpoint ' + ckpt)
            return 1                                                                        # infer.py:111-126
        ckpt = None

    # ---- data source (infer.py:147-171) ----------------------------------------------------------
    compute_stats = False
    source, samples = None, None
    if args.data_source:
        print('[i] Configuring the data source...')
        try:
            source = load_data_source(args.data_source)
            if args.sample == 'test':
                source.load_test_data(args.data_dir)
                num_samples, samples = source.num_test, source.test_samples
            else:
                source.load_trainval_data(args.data_dir, 0)
                num_samples, samples = source.num_train, source.train_samples
            print('[i] # samples:         ', num_samples)
            print('[i] # classes:         ', source.num_classes)
        except (ImportError, AttributeError, RuntimeError, OSError) as e:
            print('[!] Unable to load data source:', str(e)); return 1
        compute_stats = bool(args.compute_stats)
    if args.coco_results and not (hasattr(source, 'image_ids') and hasattr(source, 'category_ids')):
        print('[!] --coco-results needs a data source with image_ids and category_ids (--data-source coco)'); return 1

    with Session(0) as sess:
        print('[i] Creating the model...')
        stored_names = None
        if ckpt:
            with np.load(ckpt, allow_pickle=False) as ck:
                pname, num_classes = str(ck['__preset__']), int(ck['__num_classes__'])
                if '__class_names__' in ck.files:
                    stored_names = ck['__class_names__']
                if args.weights == 'ema' and not checkpoint_has_ema(ck):
                    print('[!] Bad --weights:', NO_EMA_IN_FILE % (ckpt,)); return 1
            net = SSDVGG(sess, get_preset_by_name(pname))
            net.build_from_metagraph(None, ckpt, max_batch=args.batch_size, dtype=args.dtype, weights=args.weights)
            print('[i] Weights:           ', net.weights)
        else:
            num_classes = args.num_classes
            net = SSDVGG(sess, get_preset_by_name(args.preset))
            net.build_from_vgg(None, num_classes, a_trous=args.a_trous, max_batch=args.batch_size, training=False, dtype=args.dtype)
        lid2name = resolve_class_names(num_classes, source.lid2name if source else None, stored_names)
        if not source:
            print('[i] # classes:         ', num_classes)
        size = net.preset.image_size
        # ---- files to analyse (infer.py:177-193) ----------------------------------------------------
        if source:
            files = [s.filename for s in samples]
        elif args.synthetic:
            rng = np.random.default_rng(1)
            files = [rng.integers(0, 256, (size.h, size.w, 3)).astype(np.float32) for _ in range(args.synthetic)]
            if args.synthetic_boxes > 0:
                samples = synthetic_ground_truth(args.synthetic, args.synthetic_boxes, num_classes, lid2name, size)
                compute_stats = bool(args.compute_stats)
        else:
            files = list(args.files)
            if not files:
                print('[!] No files specified'); return 1
        keep = [i for i, f in enumerate(files) if isinstance(f, np.ndarray) or os.path.exists(f) or os.path.exists(f + '.npy')]
        files = [files[i] for i in keep]
        if samples is not None:
            samples = [samples[i] for i in keep]
        if files:
            os.makedirs(args.output_dir, exist_ok=True)
        print('[i] Compute stats:     ', compute_stats)
        print('[i] Network checkpoint:', ckpt or '(random weights, --preset ' + str(args.preset) + ')')
        print('[i] Image size:        ', size)
        print('[i] Number of files:   ', len(files))
        ap_dev = compute_stats and args.ap_on == 'gpu'
        coco = args.ap_protocol == 'coco'      # COCO's box AP / AR: classes of their own, the image sizes go along
        if ap_dev:
            ap_calc = DeviceCOCOEvaluator(sess.device, num_classes) if coco else DeviceAPCalculator(sess.device, num_classes, args.ap_protocol)
        elif compute_stats:
            ap_calc = COCOEvaluator(num_classes=num_classes) if coco else APCalculator(protocol=args.ap_protocol)
        else:
            ap_calc = None
        coco_records = [] if args.coco_results else None
        if args.ap_protocol != 'reference' or args.ap_on != 'host':
            print('[i] AP protocol:       ', args.ap_protocol)
            print('[i] AP detections on:  ', args.ap_on)
        pascal_summary = PascalSummary() if args.pascal_summary else None                    # infer.py:208-209
        style = None
        if args.annotate:                                                                    # infer.py:242-247
            from .annotate import Style, write_image, GpuJpegWriter
            names = [str(lid2name.get(i, 'class_%d' % i)) for i in range(num_classes)]
            cmap = dict(getattr(source, 'colors', None) or {}) if source else {}
            cmap = {**default_colors(names), **cmap}
            style = Style([cmap[n] for n in names], names, sess.device)
        writer = GpuJpegWriter(args.jpeg_quality, args.jpeg_entropy) if style is not None and args.encoder == 'gpu' else None

        def name_of(i):
            return files[i] if isinstance(files[i], str) else f'{i:06d}.npy'

        total = 0

        def collect(pending):
            nonlocal total
            ticket, idxs, sizes, drawn = pending
            if drawn is not None and writer is not None:
                writer.write(drawn)
            elif drawn is not None:
                for i, img in enumerate(drawn.get()):
                    write_image(os.path.join(args.output_dir, os.path.basename(name_of(idxs[i]))), img)
            if ap_dev and pascal_summary is None and coco_records is None:      # the accumulator has the detections: nothing needs them on the host
                return
            for i, det in enumerate(ticket.get()):
                # decode_boxes(enc, anchors, threshold, lid2name, None); suppress_overlaps(boxes)[:200]  (infer.py:233-235)
                boxes = boxes_from_detection(det, lid2name)
                total += len(boxes)
                if compute_stats and not ap_dev:                                             # infer.py:259-260
                    if coco:
                        ap_calc.add_detections(samples[idxs[i]].boxes, boxes, samples[idxs[i]].imgsize)
                    else:
                        ap_calc.add_detections(samples[idxs[i]].boxes, boxes)
                if coco_records is not None:
                    coco_records.extend(coco_result_records(source, samples[idxs[i]], boxes))
                if pascal_summary is not None:                                               # infer.py:263-264
                    pascal_summary.add_detections(name_of(idxs[i]), boxes, img_size=sizes[i])

        def add_pass(ticket, idxs):
            """--ap-on gpu: the pass just launched goes to the accumulator; COCO's evaluator takes the image sizes too"""
            gts = [samples[i].boxes for i in idxs]
            if coco:
                ap_calc.add_pass(ticket, gts, [samples[i].imgsize for i in idxs])
            else:
                ap_calc.add_pass(ticket, gts)

        pending = None
        if args.tile:       #  windows of the source picture through the net, their boxes merged on the GPU
            from . import tiling
            detector = tiling.TiledDetector(net, args.tile, args.tile_overlap, args.tile_whole, args.tile_edge_margin, args.threshold, 200, 200,
                                            **tiling.decode_keywords(args))
            for k, (packed, offs, shapes, idxs) in enumerate(tiling.source_batches(files, args.batch_size, sess.device, args.decoder,
                                                                                  args.decoder_entropy)):
                if k == 0:
                    tiling.fp8_ready(detector, (packed, offs, shapes), args.fp8_calibration, args.fp8_calibrate_images)
                ticket = detector.launch(packed, offs, shapes)
                if ap_dev:
                    add_pass(ticket, idxs)
                if writer is not None:
                    drawn = writer.launch(detector, (packed, offs, shapes), style,
                                          [os.path.join(args.output_dir, os.path.basename(name_of(i))) for i in idxs])
                else:
                    drawn = detector.annotate_last_launch(packed, offs, shapes, style) if style is not None else None
                if pending:
                    collect(pending)
                pending = (ticket, idxs, [Size(w, h) for h, w in shapes], drawn)
        for batch in () if args.tile else fp8_batches(net, sample_generator(files, size, args.batch_size, with_sources=style is not None, decoder=args.decoder,
                                                       decoder_entropy=args.decoder_entropy), args.fp8_calibration, args.fp8_calibrate_images):
            x, idxs, sizes = batch[:3]
            net.infer_dev(x)                                                                 # infer.py:225-227
            if args.decode == 'all':
                ticket = net.detect_last_launch(x.shape[0], args.threshold, **decode_keywords(args))
            else:
                ticket = net.detect_last_launch(x.shape[0], args.threshold, None, 200)
            if ap_dev:
                add_pass(ticket, idxs)
            if writer is not None:
                drawn = writer.launch(net, batch[3], style, [os.path.join(args.output_dir, os.path.basename(name_of(i))) for i in idxs])
            else:
                drawn = net.annotate_last_launch(*batch[3], style) if style is not None else None
            if args.dump_predictions:                                                        # infer.py:251-254
                enc_boxes = net._dev_result(x.shape[0], True)
                for i in range(x.shape[0]):
                    np.save(os.path.join(args.output_dir, os.path.basename(name_of(idxs[i])) + '.npy'), enc_boxes[i])
            if pending:
                collect(pending)
            pending = (ticket, idxs, sizes, drawn)
        if pending:
            collect(pending)
        if style is not None:
            style.close()

        if compute_stats:                                                                    # infer.py:269-273
            if coco:      # (one evaluation for the table and the twelve numbers)
                result = ap_calc.compute()
                aps, summary = aps_of(result), summarize(result)
            else:
                aps = ap_calc.compute_aps()
            for k, v in aps.items():
                print('[i] AP [{0}]: {1:.3f}'.format(k, v))
            print('[i] mAP: {0:.3f}'.format(APs2mAP(aps)))
            if coco:
                print(format_summary(summary, ap_calc.thresholds))
        if coco_records is not None:
            with open(args.coco_results, 'w') as f:
                json.dump(coco_records, f)
            print('[i] COCO results:      ', args.coco_results, '(%d detections)' % len(coco_records))
        if pascal_summary is not None:                                                       # infer.py:278-279
            pascal_summary.write_summary(args.output_dir)
        if ap_dev:
            total = ap_calc.num_detections()
            ap_calc.close()
        print('[i] Processed {} images, {} detections'.format(len(files), total))
    print('[i] All done.')
    return 0


if __name__ == '__main__':
    sys.exit(main())
