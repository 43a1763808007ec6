#!/usr/bin/env python3
"""Measures what feeding training from JPEG files costs: one epoch of the train recipe through TrainingData with
num_workers planning processes, per round and interleaved in one process, for

  (a) decoder='pillow'            the workers decode every file (once per try of the redraw loop) and ship pixels
  (b) decoder='gpu'               the workers run the Huffman stage once per sample and ship coefficients; the GPU decodes
  (c) decoder='gpu' + cache       (b) with every picture kept in HBM, measured in its SECOND epoch (and later ones)

on N files of VOC shape in a VOC tree the tool writes itself: the 500 x 375 fixture picture, shifted by a different offset each and
encoded by jpeg.encode_batch at quality 90, 4:2:0.  Per row: images/s by wall clock from the first batch to the last (the consumer
only takes the batches), CPU ms per sample in the worker processes (resource.getrusage(RUSAGE_CHILDREN): the workers are forked
directly and joined after the epoch, so the difference is theirs) and in the training process (time.process_time: feeder thread
and consumer), and the bytes of the batch's arrays that go up per batch.  Nothing is sized from the machine's core count.

    python tools/feeder_rate.py [--files 512] [--rounds 5] [--batch 32] [--workers 4] [--out profiles/feeder_decode_rate.txt]

--mosaic P [P ...] measures every decoder once per mosaic probability, all interleaved in the same rounds -- name
0 among them: it is the yardstick of the same run -- and adds the mosaics and cells per epoch and the images/s against P = 0:

    python tools/feeder_rate.py --mosaic 0 0.5 1 --out profiles/mosaic_feeder_rate.txt
"""
import argparse
import os
import resource
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ['SSD_FEEDER_START'] = 'fork'        # the workers are this process's children: their CPU time shows in RUSAGE_CHILDREN

ANNOTATION = ('<annotation><filename>%s</filename><size><width>500</width><height>375</height><depth>3</depth></size>'
              '<object><name>dog</name><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>'
              '<object><name>person</name><bndbox><xmin>300</xmin><ymin>40</ymin><xmax>460</xmax><ymax>330</ymax></bndbox></object>'
              '</annotation>')


def make_voc_tree(directory, n, batch=32):
    """n 500 x 375 JPEGs with two boxes each under <directory>/trainval/VOCdevkit/VOC2007, the other lists empty"""
    from ssd_tensorflow_amd import jpeg
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'j1_jpeg.npz')) as g:
        bgr = jpeg.decode(g['voc_000232_jpg'].tobytes())
    big = np.pad(bgr, ((0, 32), (0, 32), (0, 0)), mode='reflect')
    roots = {k: os.path.join(directory, *k.split('/')) for k in ('trainval/VOCdevkit/VOC2007', 'trainval/VOCdevkit/VOC2012', 'test/VOCdevkit/VOC2007')}
    for k, root in roots.items():
        for sub in ('ImageSets/Main', 'Annotations', 'JPEGImages'):
            os.makedirs(os.path.join(root, sub), exist_ok=True)
        for name in ('trainval', 'test'):
            open(os.path.join(root, 'ImageSets', 'Main', name + '.txt'), 'w').close()
    root = roots['trainval/VOCdevkit/VOC2007']
    names = ['%06d' % i for i in range(n)]
    for o in range(0, n, batch):
        crops = [np.ascontiguousarray(big[(i // 32) % 32:(i // 32) % 32 + 375, i % 32:i % 32 + 500]) for i in range(o, min(o + batch, n))]
        for name, data in zip(names[o:], jpeg.encode_batch(crops, quality=90, subsampling='4:2:0')):
            with open(os.path.join(root, 'JPEGImages', name + '.jpg'), 'wb') as f:
                f.write(data)
    for i, name in enumerate(names):
        x0, y0 = 20 + i % 60, 30 + i % 40
        with open(os.path.join(root, 'Annotations', name + '.xml'), 'w') as f:
            f.write(ANNOTATION % (name + '.jpg', x0, y0, x0 + 220, y0 + 260))
    with open(os.path.join(root, 'ImageSets', 'Main', 'trainval.txt'), 'w') as f:
        f.write('\n'.join(names) + '\n')


def cpu_children():
    r = resource.getrusage(resource.RUSAGE_CHILDREN)
    return r.ru_utime + r.ru_stime


def epoch(td, epoch_no, batch, workers, uploads):
    """one epoch of the train set -> dict of the row's figures"""
    import torch
    td.epoch = epoch_no
    del uploads[:]
    c0, p0 = cpu_children(), time.process_time()
    n = first = 0
    t_first = None
    for x, y, gts in td.train_generator(batch, workers):
        if t_first is None:
            torch.cuda.synchronize()
            t_first, first = time.perf_counter(), len(gts)
        n += len(gts)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t_first
    recipe = td._recipes['train']
    recipe.pool.close()                        # joins the workers: their CPU time is accounted now
    recipe.pool = None
    st = td.feeder_stats
    return dict(rate=(n - first) / wall, worker_ms=(cpu_children() - c0) / n * 1e3, parent_ms=(time.process_time() - p0) / n * 1e3,
                h2d=statistics.mean(sum(u.values()) for u in uploads), arrays=sorted({k for u in uploads for k, v in u.items() if v}),
                decoded=st['decoded'], fallbacks=st['fallbacks'], cache_hits=st['cache_hits'], n=n,
                mosaics=st.get('mosaics', 0), cells=st.get('cells', 0), area_fallbacks=st.get('area_fallbacks', 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--workers', type=int, default=4)
    ap.add_argument('--mosaic', type=float, nargs='+', default=None, help='mosaic probabilities to measure every decoder at (0 = the yardstick)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'feeder_decode_rate.txt'))
    args = ap.parse_args()
    import torch
    from ssd_tensorflow_amd.training_data import TrainingData
    wide = 40 if args.mosaic else 26          # the name column: the rows of a --mosaic run carry the probability
    uploads = []

    def watched(td):
        """TrainingData whose prefetching upload notes the bytes of the arrays it sends up"""
        inner = td._upload_async

        def upload(ring, slot_arr, arrays, *a, **k):
            uploads.append({name: int(v.nbytes) for name, v in arrays.items()})
            return inner(ring, slot_arr, arrays, *a, **k)
        td._upload_async = upload
        return td

    with tempfile.TemporaryDirectory() as d:
        make_voc_tree(d, args.files, args.batch)
        kw = dict(preset='vgg300', valid_fraction=0)
        tds = {}
        for p in args.mosaic or [None]:
            tag = '' if p is None else ', mosaic %g' % p
            mk = {} if p is None else dict(mosaic=p)
            tds['pillow' + tag] = watched(TrainingData(d, **kw, **mk))
            tds['gpu' + tag] = watched(TrainingData(d, decoder='gpu', **kw, **mk))
            tds['gpu + cache, epoch >= 2' + tag] = watched(TrainingData(d, decoder='gpu', cache_bytes=args.files * 500 * 375 * 3 + (1 << 20), **kw, **mk))
        for name, td in tds.items():           # warm-up: code paths, allocations; fills the cache
            first = epoch(td, 0, args.batch, args.workers, uploads)
            print('warm-up %-*s %8.0f images/s' % (wide - 2, name, first['rate']), flush=True)
        rows = {name: [] for name in tds}
        for r in range(args.rounds):
            for name, td in tds.items():
                rows[name].append(epoch(td, 1 + r, args.batch, args.workers, uploads))
        for td in tds.values():
            td.close()

    lines = ['feeder: one epoch of the train recipe over %d JPEG files of 500 x 375 (quality 90, 4:2:0), batch %d, %d workers, vgg300' %
             (args.files, args.batch, args.workers),
             '%s, torch %s; %d interleaved rounds in one process, medians (min .. max)' % (torch.cuda.get_device_name(0), torch.__version__, args.rounds),
             'worker CPU: user + system time of the joined worker processes; parent CPU: time.process_time of the training process',
             '',
             '%-*s %22s %28s %28s %16s' % (wide, 'decoder', 'images/s', 'worker CPU ms/sample', 'parent CPU ms/sample', 'H2D bytes/batch')]
    med = lambda v: '%.3f (%.3f .. %.3f)' % (statistics.median(v), min(v), max(v))
    for name, rs in rows.items():
        rate = [r['rate'] for r in rs]
        lines.append('%-*s %22s %28s %28s %16.0f' % (wide, name, '%.0f (%.0f .. %.0f)' % (statistics.median(rate), min(rate), max(rate)),
                                                      med([r['worker_ms'] for r in rs]), med([r['parent_ms'] for r in rs]),
                                                      statistics.median(r['h2d'] for r in rs)))
    lines.append('')
    for name, rs in rows.items():
        lines.append('%-*s arrays that go up: %s; per epoch decoded %d, fallbacks %d, cache hits %d of %d samples' %
                     (wide, name, ', '.join(rs[-1]['arrays']), rs[-1]['decoded'], rs[-1]['fallbacks'], rs[-1]['cache_hits'], rs[-1]['n']))
    if args.mosaic and 0 in args.mosaic:
        # against P = 0 of the same run: a sample is one delivered image whatever it was composed of; the bf16 step takes 6.8 ms at
        # batch 32 (README), so a feeder hides behind it while it delivers more than batch / 6.8 ms images/s
        need = args.batch / 6.8e-3
        lines += ['', 'against mosaic 0 of the same run (a mosaic is ONE delivered image made of four source pictures); the bf16 step of 6.8 ms at '
                  'batch %d consumes %.0f images/s:' % (args.batch, need)]
        for dec in ('pillow', 'gpu', 'gpu + cache, epoch >= 2'):
            base = [r['rate'] for r in rows[dec + ', mosaic 0']]
            for p in args.mosaic:
                rs = rows[dec + ', mosaic %g' % p]
                rate = [r['rate'] for r in rs]
                apart = 'separate' if max(rate) < min(base) or min(rate) > max(base) else 'overlap'
                lines.append('%-40s %.2f x mosaic 0 (rounds %s); %d mosaics, %d cells, %d area fallbacks per epoch; %s the bf16 step' % (
                    dec + ', mosaic %g' % p, statistics.median(rate) / statistics.median(base), apart, rs[-1]['mosaics'], rs[-1]['cells'],
                    rs[-1]['area_fallbacks'], 'hides behind' if min(rate) > need else 'does NOT hide behind'))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
