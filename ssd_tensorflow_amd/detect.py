#!/usr/bin/env python3
"""Deployment tool: the counterpart of the reference's detect.py (:41-125) over the HIP library.  Image files in; per image
`<name>.txt` with one '{label} {labelid} {cx} {cy} {w} {h}' line per detection (detect.py:119-122) and the image with the
detections drawn on it (annotate.py) out.  --model is a checkpoint .npz: it already carries the preset, the
graph and the class names the reference reads from its .pb + training-data pickle.  Threshold 0.5, NMS, [:200]
(detect.py:111-112)."""
import argparse
import os
import sys

import numpy as np

from .annotate import Style, write_image, GpuJpegWriter
from .infer import (sample_generator, resolve_class_names, add_fp8_arguments, check_fp8_arguments, fp8_batches, add_decode_arguments,
                    check_decode_arguments, decode_keywords)
from .ssdvgg import SSDVGG, Session, checkpoint_has_ema, NO_EMA_IN_FILE
from .ssdutils import get_preset_by_name, boxes_from_detection
from .utils import default_colors


def main(argv=None):
    parser = argparse.ArgumentParser(description='SSD inference')
    parser.add_argument('files', nargs='*')
    parser.add_argument('--model', default='model300.npz', help='model file (a checkpoint .npz)')
    parser.add_argument('--training-data', default='', help='unused: the checkpoint carries the preset and the class names')
    parser.add_argument('--output-dir', default='test-out', help='output directory')
    parser.add_argument('--batch-size', type=int, default=32, help='batch size')
    parser.add_argument('--dtype', default='f32', choices=['f32', 'bf16', 'fp8', 'mxfp8', 'mxfp6'],
                        help='f32, bf16 activations on the bf16 matrix cores, fp8: the bf16 net with conv3_2 ... mod_conv7 on e4m3 operands '
                             '(calibrated scales), or mxfp8: the same layers with block scales chosen from the data (no calibration; the fc graph\'s 7x7 fc6 joins '
                             'them when the environment has SSD_MXFP8_BIGK=1), or mxfp6: the mxfp8 layers on 6-bit e2m3 operands with block scales on '
                             'activations and filters (no calibration; fc6 stays on bf16)')
    parser.add_argument('--weights', default='auto', choices=['auto', 'raw', 'ema'],
                        help="a model file of a run with --ema-decay holds two sets of weights: raw = the last iterate; ema = the average (an error "
                             "if the file has none); auto = the average where the file has one.  Every --dtype, and fp8's calibration, runs on the chosen set")
    add_fp8_arguments(parser)
    parser.add_argument('--decoder', default='gpu', choices=['pillow', 'gpu'],
                        help='gpu: baseline JPEGs are decoded on the GPU, other files as with pillow (same pixels); pillow: every file is decoded on the host')
    parser.add_argument('--decoder-entropy', default='host', choices=['host', 'gpu'],
                        help='--decoder gpu: host: Huffman decoding on host threads; gpu: on the GPU as well, only the files\' bytes go to the device (same pixels)')
    parser.add_argument('--encoder', default='pillow', choices=['pillow', 'gpu'],
                        help='gpu: annotated pictures named .jpg / .jpeg are encoded as baseline JPEG on the GPU (what cv2.imwrite writes), other names as with pillow; pillow: every picture is encoded on the host')
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

    print('[i] Model:         ', args.model)
    print('[i] Training data: ', args.training_data)
    print('[i] Output dir:    ', args.output_dir)
    print('[i] Batch size:    ', args.batch_size)
    if not os.path.exists(args.model):
        print('[!] Cannot find model ' + args.model); return 1
    files = [f for f in args.files if os.path.exists(f) or os.path.exists(f + '.npy')]
    os.makedirs(args.output_dir, exist_ok=True)

    with Session(0) as sess:
        with np.load(args.model, allow_pickle=False) as ck:
            pname, num_classes = str(ck['__preset__']), int(ck['__num_classes__'])
            stored = ck['__class_names__'] if '__class_names__' in ck.files else None
            if args.weights == 'ema' and not checkpoint_has_ema(ck):
                print('[!] Bad --weights:', NO_EMA_IN_FILE % (args.model,)); return 1
        net = SSDVGG(sess, get_preset_by_name(pname))
        net.build_from_metagraph(None, args.model, max_batch=args.batch_size, dtype=args.dtype, weights=args.weights)
        print('[i] Weights:       ', net.weights)
        lid2name = resolve_class_names(num_classes, None, stored)
        names = [str(lid2name[i]) for i in range(num_classes)]
        colors = default_colors(names)
        style = Style([colors[n] for n in names], names, sess.device)

        writer = GpuJpegWriter(args.jpeg_quality, args.jpeg_entropy) if args.encoder == 'gpu' else None

        def collect(pending):
            ticket, idxs, drawn = pending
            if writer is not None:
                writer.write(drawn)
            else:
                images = drawn.get()
            for i, det in enumerate(ticket.get()):
                name = os.path.basename(files[idxs[i]])
                with open(os.path.join(args.output_dir, name + '.txt'), 'w') as f:
                    for _, box in boxes_from_detection(det, lid2name):
                        f.write('{} {} {} {} {} {}\n'.format(box.label, box.labelid, box.center.x, box.center.y, box.size.w, box.size.h))
                if writer is None:
                    write_image(os.path.join(args.output_dir, name), images[i])

        pending = None
        if args.tile:       #  windows of the source picture through the net, their boxes merged on the GPU
            from . import tiling
            detector = tiling.TiledDetector(net, args.tile, args.tile_overlap, args.tile_whole, args.tile_edge_margin, 0.5, 200, 200,
                                            **tiling.decode_keywords(args))
            for k, (packed, offs, shapes, idxs) in enumerate(tiling.source_batches(files, args.batch_size, sess.device, args.decoder,
                                                                                  args.decoder_entropy)):
                if k == 0:
                    tiling.fp8_ready(detector, (packed, offs, shapes), args.fp8_calibration, args.fp8_calibrate_images)
                ticket = detector.launch(packed, offs, shapes)
                if writer is not None:
                    drawn = writer.launch(detector, (packed, offs, shapes), style,
                                          [os.path.join(args.output_dir, os.path.basename(files[i])) for i in idxs])
                else:
                    drawn = detector.annotate_last_launch(packed, offs, shapes, style)
                if pending:
                    collect(pending)
                pending = (ticket, idxs, drawn)
        for x, idxs, sizes, sources in () if args.tile else fp8_batches(net, sample_generator(files, net.preset.image_size, args.batch_size, with_sources=True,
                                                                          decoder=args.decoder, decoder_entropy=args.decoder_entropy),
                                                   args.fp8_calibration, args.fp8_calibrate_images):
            net.infer_dev(x)
            if args.decode == 'all':
                ticket = net.detect_last_launch(x.shape[0], 0.5, **decode_keywords(args))
            else:
                ticket = net.detect_last_launch(x.shape[0], 0.5, None, 200)                  # detect.py:111-112
            if writer is not None:
                drawn = writer.launch(net, sources, style, [os.path.join(args.output_dir, os.path.basename(files[i])) for i in idxs])
            else:
                drawn = net.annotate_last_launch(*sources, style)
            if pending:
                collect(pending)
            pending = (ticket, idxs, drawn)
        if pending:
            collect(pending)
        style.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
