"""Batch feeder for the step loop: the counterpart of the reference's TrainingData /
DataQueue (training_data.py:35-206, data_queue.py:26-112) for the path this build covers.

The reference forks N workers that run cv2 transforms and copy finished float32 batches through
shared-memory slots to ONE device.  Here every rank feeds only its own shard (parallel.ShardSampler) and
a batch is born in HBM: the images come out of the batch augmentation kernels (transforms.augment_batch:
the reference's transform recipe, decisions on the host, pixels on the GPU), the label vectors out of the
HIP label encoder (ssd_encode_labels_dev) -- only the images' source bytes and a handful of boxes go up,
nothing of a batch ever comes down.  A generator yields `(images, labels, gt_boxes)` like the
reference's, with `images` / `labels` float32 CUDA tensors (device_tensors=False: numpy arrays).

`gen_batch(batch_size, num_workers)` means what the reference's means (training_data.py:137-195):

  * num_workers == 0: the serial generator -- batch k+1 is prepared when the caller asks for it;
  * num_workers  > 0: that many forked worker processes run the host half of the recipe (file decode, the
    transforms' decisions incl. the <= 50 redraws, packing) into the slots of a data_queue.DataQueue,
    while a feeder thread of the training process uploads finished slots IN ORDER and launches the
    augmentation + label kernels on its own stream into a ring of three device slots.  Batch k+1 is
    therefore ready in HBM while step k runs; the consumer's stream waits for the slot's event, and a
    slot is rewritten only after the kernels the consumer enqueued on it have run.  A yielded batch is
    valid until the next one is requested.

The two are bit-identical: every sample's decisions are drawn from Python's `random` seeded with
(seed, data set, epoch, sample index), so a batch does not depend on which process prepared it or on what
was drawn before (tests/test_feeder_cpu.py, tests/test_gpu_feeder.py).  The reference's workers all start
from the parent's `random` state and its batches arrive in completion order: an epoch there is not
reproducible; that is not mirrored.

Sources:
  * data_dir None / '' / 'synthetic'  -- SURVEY.md 8d: float32 preset-sized images (augment=False) or a
    uint8 "dataset" of variously sized images that goes through the whole recipe (augment=True);
  * any other data_dir                 -- a dataset directory read through a data source module
    (`source_<data_source>.get_source()`, utils.py:44-55 / process_dataset.py:199-204), e.g. the Pascal
    VOC tree.  The reference splits this in two programs: process_dataset.py pickles the sample lists and
    the transform objects, train.py unpickles them (training_data.py:41-69).  Those pickles hold instances
    of the reference's own classes; here the same sample lists and the same recipes
    (transforms.build_train_transforms / build_valid_transforms) are built in process.  Images are
    decoded by transforms.load_image_bgr (.npy arrays or Pillow; decoder parity with OpenCV unpinned).

decoder='gpu' (DESIGN.md 17): the workers run only the Huffman stage of a JPEG (ssd_jpeg_entropy_decode, host only) and ship int16
coefficients; the feeder launches ssd_jpeg_decode_batch_dev in front of the augmentation kernel, so the pixels are born in HBM too.
cache_bytes > 0 keeps them there (_SourceArena): from the second epoch on a cached sample costs its worker no file and the bus
nothing but its parameter record and boxes.

mosaic > 0: with that probability a training sample is a 2 x 2 mosaic of its own picture and three partners.  A
batch is then a plan list of up to four source pictures per sample plus 'cells' (where each lands) and 'src_idx' (which picture of
the data set each is); the decode, the cache and the fallback work per source picture, ssd_augment_cells_dev composes the samples,
and slots, staging, arena scratch and workspace are sized for four sources per sample.
"""
import multiprocessing as mp
import os
import queue
import random
import threading
import time
import traceback

import numpy as np

from .data_queue import DataQueue, WorkerError
from .parallel import ShardSampler
from .ssdutils import (encode_labels_batch, encode_labels_batch_dev, get_preset_by_name, has_positive_anchor, match_id,
                       prime_anchor_table)
from .utils import Box, Point, Size, Sample, load_data_source

VOC_NAMES = ['aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog',
             'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor']

DEVICE_SLOTS = 3            # one under the step, one ready, one being filled
DECODERS = ('pillow', 'gpu')
SRC_PIXELS, SRC_COEF, SRC_CACHED = 0, 1, 2      # 'src_kind' of a sample (decoder='gpu'): pixels in 'packed', coefficients in 'coef', nothing
MAX_CLASSES = 127           # the library's range: 1..127 classes (include/ssdvgg_hip.h)


def default_class_names(num_classes):
    """Names of classes no data source names: the VOC names for 20 classes, else 'class_<id>'."""
    if num_classes == len(VOC_NAMES):
        return list(VOC_NAMES)
    return ['class_%d' % i for i in range(num_classes)]


CACHE_SYNTHETIC_UP_TO = 4096  # synthetic "files" kept in RAM (a real source reads its files instead)


def _gt_arrays(gts):
    bxs = [np.array([[b.center.x, b.center.y, b.size.w, b.size.h] for b in g], np.float64).reshape(-1, 4) for g in gts]
    cls = [np.array([b.labelid for b in g], np.int32) for g in gts]
    return bxs, cls


def _gt_packed(gts, num_classes):
    """The batch's boxes as the label encoder's three arrays (what ssd_encode_labels* take): [ntot, 4] float64
    proportional (cx, cy, w, h), [ntot] int32 class ids, [b + 1] int32 offsets.  They ride in the batch's slot and
    reach the GPU with the images' bytes; the class range is checked here (the resident encoder does not)."""
    from .ssdutils import _pack_gt
    bxs, cls = _gt_arrays(gts)
    gt, gcls, goff = _pack_gt(bxs, cls)
    if gcls.size and (gcls.min() < 0 or gcls.max() >= num_classes):
        raise ValueError('a ground-truth class id lies outside 0..%d' % (num_classes - 1))
    return {'gt': gt, 'gcls': gcls, 'goff': goff}


class _Recipe:
    """One data set of a TrainingData (train or valid): where its samples come from and how a list of sample
    indices becomes the host half of a batch.  Lives in the parent and, by fork, in the workers."""

    def __init__(self, td, which, total, salt, sample_at=None, transforms=None):
        self.td, self.which, self.total, self.salt = td, which, total, salt
        self.sample_at, self.transforms = sample_at, transforms
        self.pool = None
        self.active = False
        self.dev = None                        # this data set's device-side slot ring + feeder stream (TrainingData._device_ring)
        # decoder='gpu' on a data set of files: JPEGs travel as coefficients and are decoded in front of the augmentation kernel
        self.gpu_decode = td.decoder == 'gpu' and td._real_dataset and transforms is not None
        self.stats = None                      # the feeder_stats of this data set's live generator

    def __getstate__(self):      # what a worker needs: not the pool it belongs to, nothing that lives on the GPU
        st = dict(self.__dict__)
        st['pool'] = None
        st['dev'] = None
        st['active'] = False
        return st

    # ---- host half of a batch: runs in a worker process or, for num_workers == 0, in the caller --------------------
    def plan(self, epoch, idx, known=None):
        """known (decoder='gpu'): {position in idx: (h, w)} of the samples whose pixels the training process holds in HBM.
        (The transforms draw from the module-level `random`, seeded per sample below.  In the serial generator this runs in the
        caller's process: its generator state is put back afterwards -- the reference never reseeds, and whatever else draws from
        `random` in the driver must not become a function of the last sample index.)"""
        state = random.getstate()
        try:
            return self._plan(epoch, idx, known)
        finally:
            random.setstate(state)

    def _plan(self, epoch, idx, known=None):
        td = self.td
        if self.transforms is None:                              # preset-sized float32 synthetic images
            imgs, gts = [], []
            for i in idx:
                # redrawn (<= 50 times) until at least one anchor is positive (training_data.py:92-98)
                for tries in range(50):
                    img, gt = td._sample(int(i) + 7919 * tries, self.salt)
                    if has_positive_anchor(td.preset, gt, td.match):
                        break
                imgs.append(img); gts.append(gt)
            return dict({'images': np.stack(imgs)}, **_gt_packed(gts, td.num_classes)), gts
        from . import transforms as T
        host_tfs = [t for t in self.transforms if not isinstance(t, T.LabelCreatorTransform)]
        mosaics = td.mosaic_prob(self, epoch) > 0            # (False: nothing new is drawn, no new array travels)
        sources = self.sources(epoch, idx) if mosaics else [([int(i)], None) for i in idx]
        return self._plan_sources(epoch, sources, known, host_tfs, mosaics)

    def _pack(self, plans, gts, extra=None):
        """The planned pictures and the samples' boxes as the arrays that travel.  extra (a batch with mosaics): 'cells' [n_src][5]
        int32 (sample, x0, y0, w, h), 'src_idx' (the data set index of every source picture) and 'mosaic_stats'."""
        from . import transforms as T
        td = self.td
        W, H = td.preset.image_size.w, td.preset.image_size.h
        extra = extra or {}
        cells = extra.get('cells')
        if not self.gpu_decode:
            arr, packed = T.plan_params(plans, W, H, cells=cells)
            return dict({'params': np.frombuffer(arr, np.uint8).copy(), 'packed': packed}, **extra, **_gt_packed(gts, td.num_classes)), gts
        coef, descs = self._entropy_stage(plans)
        arr, packed = T.plan_params(plans, W, H, cells=cells)
        kind = np.array([SRC_PIXELS if p.jpeg is None else SRC_COEF if p.jpeg.data is not None else SRC_CACHED for p in plans], np.int32)
        for d, k in zip(descs, np.flatnonzero(kind == SRC_COEF)):
            d.dst_off = arr[k].src_off
        return dict({'params': np.frombuffer(arr, np.uint8).copy(), 'packed': packed, 'coef': coef,
                     'descs': np.frombuffer(b''.join(bytes(d) for d in descs), np.uint8).copy(), 'src_kind': kind},
                    **extra, **_gt_packed(gts, td.num_classes)), gts

    # ---- mosaic augmentation ------------------------------------------------------------------------------
    def sources(self, epoch, idx):
        """Per sample of idx: (the data set indices of its source pictures -- itself, or itself and its three partners --, the
        mosaic centre or None).  A pure function of (seed, epoch, index): the parent computes it without running a transform (the
        arena's `known` table of a task), the worker that plans the batch computes the same."""
        from . import transforms as T
        td = self.td
        p = td.mosaic_prob(self, epoch)
        W, H = td.preset.image_size.w, td.preset.image_size.h
        out = []
        for i in idx:
            d = T.mosaic_draw(td._sample_seed(self.salt, epoch, int(i)), p, self.total, W, H, td.mosaic_center) if p > 0 else None
            out.append(([int(i)], None) if d is None else ([int(i)] + d[0], d[1]))
        return out

    def _plan_sources(self, epoch, sources, known, host_tfs, mosaics):
        """The transform path of _plan.  sources: per sample (its source pictures, the mosaic centre or None).  A sample that is no
        mosaic runs the transform list seeded from its sample seed, as ever (with mosaics it is also booked as the one cell
        (0, 0, W, H)); a mosaic's four cells run the cell transform list (transforms.mosaic_cell_transforms), each seeded from
        (sample seed, try, cell).  Either is redrawn (<= 50 times) until at least one anchor is positive (training_data.py:88-98;
        the label of a try is only LOOKED at there, so the test runs on the host and the label vectors of the whole batch are
        encoded once, on the GPU); a mosaic's test sees the MERGED boxes and redraws the four recipes, never the partners.
        known: {position in the batch's flat source list: (h, w)}."""
        from . import transforms as T
        td = self.td
        W, H = td.preset.image_size.w, td.preset.image_size.h
        loader = host_tfs[0]
        preset_images = getattr(loader, 'images', None)
        cell_tfs, resize = T.mosaic_cell_transforms(self.transforms) if mosaics else (None, None)
        plans, gts, cells, src_idx = [], [], [], []
        stats = np.zeros(3, np.int64)          # mosaics, cells, area_fallbacks

        def load(i, pos):                      # the loader's state for source picture i at position pos of the flat source list
            s = self.sample_at(i)
            if not isinstance(s, Sample):                        # synthetic: the pixels travel with the record
                loader.images, sample = s
            else:
                loader.images, sample = preset_images, s
            if self.gpu_decode:                                  # the file is read once per sample, or not at all
                loader.kept = None
                if known and pos in known and isinstance(s, Sample):
                    loader.kept = (s.filename, T.DeferredJpeg(None, known[pos], s.filename))
            return sample

        try:
            for k, (srcs, centre) in enumerate(sources):
                seed = td._sample_seed(self.salt, epoch, srcs[0])
                pos = len(plans)
                if centre is None:
                    sample = load(srcs[0], pos)
                    random.seed(seed)
                    for _ in range(50):
                        args = (None, None, sample)
                        for t in host_tfs:
                            args = t(*args)
                        if has_positive_anchor(td.preset, args[2].boxes, td.match):
                            break
                    plans.append(args[0]); gts.append(args[2].boxes)
                    cells.append((k, 0, 0, W, H)); src_idx.append(srcs[0])
                    stats[1] += 1
                    continue
                layout = T.mosaic_layout(centre[0], centre[1], W, H)
                kept = [None] * 4              # decoder='gpu': each file is read once per sample, whatever the number of tries
                for tries in range(50):
                    got, merged, fell = [], [], 0
                    for c, (src, cell) in enumerate(zip(srcs, layout)):
                        sample = load(src, pos + c)
                        if self.gpu_decode and kept[c] is not None:
                            loader.kept = kept[c]
                        random.seed((seed << 16) | (tries << 4) | (c + 1))
                        args = (None, None, sample)
                        for t in cell_tfs:
                            args = t(*args)
                        if self.gpu_decode:
                            kept[c] = loader.kept
                        data, _, gt, f = T.mosaic_cell_resize(resize, args[0], args[1], args[2], cell[2], cell[3])
                        got.append(data); fell += f
                        merged += [T.mosaic_box(b, cell, W, H) for b in gt.boxes]
                    if has_positive_anchor(td.preset, merged, td.match):
                        break
                plans += got; gts.append(merged)
                cells += [(k,) + cell for cell in layout]; src_idx += srcs
                stats += (1, 4, fell)
        finally:
            loader.images = preset_images
            if self.gpu_decode:
                loader.kept = None
        if not mosaics:
            return self._pack(plans, gts)
        return self._pack(plans, gts, {'cells': np.array(cells, np.int32).reshape(-1, 5), 'src_idx': np.array(src_idx, np.int64),
                                       'mosaic_stats': stats})

    @staticmethod
    def _entropy_stage(plans):
        """The Huffman stage of the batch's deferred JPEGs, host only: (int16 coefficients of all of them, each file's at a
        16-byte aligned offset; their ssd_jpeg_desc records, coef_off relative to that array).  A file the 32-bit range guard
        refuses becomes a host-pixel plan in place (its decisions stand: they depend on the size alone); a corrupt stream raises
        JpegError with the file's name."""
        import ctypes as C
        from . import jpeg as J, transforms as T
        from ._lib import lib, last_error
        todo = [p for p in plans if p.jpeg is not None and p.jpeg.data is not None]
        bufs = [J._buf(p.jpeg.data) for p in todo]
        sizes = [(lib.ssd_jpeg_coef_bytes(a[1], a[2]) + 15) // 16 * 16 for a in bufs]
        coef = np.zeros(sum(sizes) // 2, np.int16)
        descs, off = [], 0
        for p, (_, ptr, n), size in zip(todo, bufs, sizes):
            d, st = J.Desc(), C.c_int()
            if lib.ssd_jpeg_entropy_decode(ptr, n, coef.ctypes.data + off, size, C.byref(d), st) != 0:
                raise J.JpegError('%s: %s' % (p.jpeg.filename, last_error()))
            if st.value != J.OK:                                 # the range guard (max_l1 > SSD_JPEG_MAX_L1): the pixel path
                img = np.ascontiguousarray(T.load_image_bgr(p.jpeg.filename))
                if img.dtype != np.uint8 or img.shape != (p.src.h, p.src.w, 3):
                    raise ValueError('%s: the decoded image is %s %s, its header says %d x %d' %
                                     (p.jpeg.filename, img.dtype, img.shape, p.src.w, p.src.h))
                coef[off // 2:(off + size) // 2] = 0
                p.image, p.jpeg = img, None
                continue
            for c in range(3):
                d.coef_off[c] += off // 2
            descs.append(d)
            off += size
        return coef[:off // 2], descs

    def slot_bytes(self, batch_size):
        td = self.td
        W, H = td.preset.image_size.w, td.preset.image_size.h
        if self.transforms is None:
            return batch_size * (H * W * 3 * 4 + 4096) + 8192
        # (decoder='gpu': a sample travels as pixels OR as coefficients, and the coefficients' bound is the larger one)
        per_image = max(td._max_image_bytes, td._max_coef_bytes + 512 if self.gpu_decode else 0)
        return td.sources_per_batch(self, batch_size) * (per_image + 16 + 256 + 4096) + 8192


def _worker_main(recipe, tasks, results, anchors_abs=None):
    """batch_producer of the reference (training_data.py:109-134).  The workers never touch the GPU: the anchor table of
    the redraw test is computed by the training process before they start and handed over (`anchors_abs`; a forked worker
    has inherited it as well)."""
    if anchors_abs is not None:
        prime_anchor_table(recipe.td.preset, anchors_abs)
    try:
        import signal
        signal.signal(signal.SIGINT, signal.SIG_IGN)
    except Exception:
        pass
    parent = os.getppid()
    while True:
        try:
            task = tasks.get(timeout=5.0)
        except queue.Empty:
            if os.getppid() != parent:      # the training process is gone (killed): do not linger
                break
            continue
        if task is None:
            break
        gen, seq, slot, epoch, idx, known = task
        try:
            arrays, gts = recipe.plan(epoch, idx, known)
            results.put((gen, seq), slot, arrays, gts)
        except BaseException:
            results.put_error((gen, seq), slot, traceback.format_exc())


class _SourceArena:
    """Where the source pixels of decoder='gpu' batches lie: ONE uint8 device buffer (ssd_augment_batch_dev reads all sources of a
    batch from one buffer) of `cache_bytes` that decoded pictures are appended to and never leave, plus a scratch tail with one
    region per data set and device slot (and one for each data set's serial generator) for the pictures that are not kept.
    Append-only: an entry is never moved, evicted or rewritten, so a reader needs no more than stream order behind the append
    that wrote its entry -- `event` is recorded behind the last append and a batch enqueued on another stream waits for it first.
    `lock` is held from placing a batch's pictures until that event is recorded: two data sets' feeder threads share the arena."""

    def __init__(self, cache_bytes, max_image_bytes):
        self.cache_bytes = int(cache_bytes) // 256 * 256
        self.max_image_bytes = int(max_image_bytes)
        self.image_bytes = (self.max_image_bytes + 16 + 255) // 256 * 256
        self.buf, self.batch = None, 0
        self.scale = {'train': 1, 'valid': 1}      # source pictures per sample of a data set's batches (a mosaic has four)
        self.table = {}                        # (data set, sample index) -> (byte offset, h, w)
        self.used = 0
        self.event, self.event_stream = None, None
        self.lock = threading.Lock()

    def ensure(self, batch_size, dev, busy):
        """The buffer with scratch regions for batches of batch_size.  A larger batch than any before needs a larger tail: the
        buffer is replaced and the entries copied to the same offsets, which only works while no generator is using it."""
        import torch
        with self.lock:
            if self.buf is not None and self.batch >= batch_size:
                return
            if self.buf is not None and busy:
                raise RuntimeError('a larger batch size needs a larger source arena: finish the live generators first')
            size = self.cache_bytes + (DEVICE_SLOTS + 1) * sum(self.scale.values()) * batch_size * self.image_bytes
            buf = torch.empty((size,), dtype=torch.uint8, device=dev)
            cur = torch.cuda.current_stream(dev)
            if self.buf is not None and self.used:
                if self.event is not None:
                    cur.wait_event(self.event)
                buf[:self.used].copy_(self.buf[:self.used])
                self.event = torch.cuda.Event()
                self.event.record(cur)
                self.event_stream = cur.cuda_stream
            self.buf, self.batch = buf, batch_size

    def region(self, which, slot):
        """(byte offset, bytes) of the scratch of a data set's device slot (None: its serial generator)"""
        n = self.scale[which] * self.batch * self.image_bytes
        first = 0 if which == 'train' else (DEVICE_SLOTS + 1) * self.scale['train'] * self.batch * self.image_bytes
        return self.cache_bytes + first + (0 if slot is None else 1 + slot) * n, n


class _SharedImageCache:
    """The synthetic data sets' "files" (uint8 images) in shared memory: written once by the training process while it builds
    its sample list, read as views by every worker however it was started (a forked worker used to inherit a dict of arrays;
    one that comes from the fork server inherits nothing).  A real source reads its files in the workers instead."""
    CHUNK = 128 << 20

    def __init__(self, limit):
        self.limit, self.chunks, self.used, self.index, self.records = limit, [], 0, {}, {}

    def get(self, key):
        e = self.index.get(key)
        if e is None:
            return None
        c, off, h, w = e
        name, sample = self.records[key]
        img = np.frombuffer(self.chunks[c], dtype=np.uint8, count=h * w * 3, offset=off).reshape(h, w, 3)
        return {name: img}, sample

    def put(self, key, name, img, sample):
        if len(self.index) >= self.limit:
            return
        n = int(img.nbytes)
        if not self.chunks or self.used + n > len(self.chunks[-1]):
            self.chunks.append(mp.get_context('fork').RawArray('B', max(self.CHUNK, n)))
            self.used = 0
        c, off = len(self.chunks) - 1, self.used
        np.frombuffer(self.chunks[c], dtype=np.uint8, count=n, offset=off)[:] = img.reshape(-1)
        self.used += (n + 255) // 256 * 256
        self.index[key] = (c, off, img.shape[0], img.shape[1])
        self.records[key] = (name, sample)

    def __len__(self):
        return len(self.index)


def _start_context():
    """How the planning workers come to life.  Default `forkserver`: the training process asks a small server process --
    started once with a fresh interpreter, this module preloaded, never a HIP call -- to fork the workers, so what a worker
    costs does not depend on the training process: forking THAT copies the page tables of everything it has ever mapped
    (6-8 ms in a fresh process with 7 GB of HBM mapped, SECONDS in one that has created and destroyed a hundred handles:
    profiles/r03_b_fork_probe.txt -- round 3 ordered its test suite around this).  The recipe, the shared-memory slots and the
    anchor table travel to the worker as pickled Process arguments.  SSD_FEEDER_START=fork restores the direct fork."""
    method = os.environ.get('SSD_FEEDER_START', 'forkserver')
    if method not in ('fork', 'forkserver', 'spawn'):
        raise ValueError('SSD_FEEDER_START must be fork, forkserver or spawn, got %r' % (method,))
    ctx = mp.get_context(method)
    if method == 'forkserver':
        try:
            ctx.set_forkserver_preload(['ssd_tensorflow_amd.training_data', 'ssd_tensorflow_amd.transforms'])
        except Exception:
            pass
    return ctx


class _NoMainReimport:
    """While the workers start: keep multiprocessing from re-importing the launching script in them.  A worker that comes from
    the fork server (or from spawn) is told the parent's `__main__` -- by path or by module name -- and runs it again as
    `__mp_main__` before its target; everything a worker needs (`_worker_main`, the recipe's classes) is importable from this
    package, while a training script WITHOUT an `if __name__ == '__main__':` guard would run a second time in every worker (and
    die at its own first worker start: BrokenPipeError in the parent).  Nothing defined in `__main__` can therefore travel to a
    worker: a data source or transform belongs in a module."""

    def __enter__(self):
        import sys
        self.main = sys.modules.get('__main__')
        self.saved = {}
        for k in ('__spec__', '__file__'):
            if self.main is not None and hasattr(self.main, k):
                self.saved[k] = getattr(self.main, k)
                try:
                    if k == '__spec__':
                        setattr(self.main, k, None)
                    else:
                        delattr(self.main, k)
                except Exception:
                    self.saved.pop(k)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(self.main, k, v)
        return False


class _SampleAt:
    """sample #i of a data set (picklable: it travels to the workers)."""

    def __init__(self, td, which, salt):
        self.td, self.which, self.salt = td, which, salt

    def __call__(self, i):
        td = self.td
        samples = td.train_samples if self.which == 'train' else td.valid_samples
        if td._real_dataset:
            return samples[i]
        return td._dataset_sample(i, self.salt)


class _WorkerPool:
    def __init__(self, recipe, num_workers, slot_bytes):
        ctx = _start_context()
        self.num_workers, self.slot_bytes = num_workers, slot_bytes
        self.nslots = num_workers + 2
        self.tasks = ctx.Queue()
        self.results = DataQueue(slot_bytes, self.nslots, ctx)
        self.free_slots = list(range(self.nslots))
        self.outstanding = {}                 # (gen, seq) -> slot of tasks whose result has not been seen
        self.generation = 0
        self.pinned = []
        self.workers = []
        anchors_abs = prime_anchor_table(recipe.td.preset)      # (computed once per process, on the GPU unless a test installed one)
        try:
            with _NoMainReimport():
                for _ in range(num_workers):
                    w = ctx.Process(target=_worker_main, args=(recipe, self.tasks, self.results, anchors_abs), daemon=True)
                    w.start()
                    self.workers.append(w)
        except Exception as e:      # no fork server to be had (e.g. nothing picklable about a custom source): the direct fork still works
            if ctx.get_start_method() == 'fork':
                raise
            import warnings
            warnings.warn('feeder workers could not be started through %s (%s: %s); forking them directly' %
                          (ctx.get_start_method(), type(e).__name__, e), RuntimeWarning)
            for w in self.workers:
                try:
                    w.terminate()
                except Exception:
                    pass
            self.workers = []
            fork = mp.get_context('fork')
            for _ in range(num_workers):
                w = fork.Process(target=_worker_main, args=(recipe, self.tasks, self.results, anchors_abs), daemon=True)
                w.start()
                self.workers.append(w)

    def pin(self, device):
        """Page-lock the slots so the uploads are asynchronous DMA transfers (a refusal is harmless: the copies are
        then staged by the runtime)."""
        import torch
        if self.pinned or not torch.cuda.is_available():
            return
        rt = torch.cuda.cudart()
        for a in self.results.array_pool:
            try:
                rc = rt.cudaHostRegister(a.ctypes.data, a.nbytes, 0)
                self.pinned.append(int(rc) == 0)
            except Exception:
                self.pinned.append(False)

    def check_alive(self):
        for w in self.workers:
            if not w.is_alive():
                raise RuntimeError('a feeder worker process died (exit code %s)' % (w.exitcode,))

    def unpin(self):
        """Before the slots' memory goes away: a registration that outlives its pages poisons whatever the allocator
        maps at that address next (a later hipMemcpy from an ordinary buffer there fails with "invalid argument")."""
        if not any(self.pinned):
            self.pinned = []
            return
        import torch
        rt = torch.cuda.cudart()
        for a, ok in zip(self.results.array_pool, self.pinned):
            if ok:
                try:
                    rt.cudaHostUnregister(a.ctypes.data)
                except Exception:
                    pass
        self.pinned = []

    def close(self):
        self.unpin()
        for _ in self.workers:
            try:
                self.tasks.put(None)
            except Exception:
                pass
        for w in self.workers:
            w.join(timeout=2)
            if w.is_alive():
                w.terminate()
        self.workers = []


class TrainingData:
    """Same attributes the drivers read from the reference's TrainingData: preset, num_classes,
    lid2name, lname2id, num_train, num_valid, train_samples, valid_samples, train_generator,
    valid_generator.  `global_count` holds the size of the global batch the generator yielded last
    (what parallel.train_step_dp needs when the last batch of an epoch is short)."""

    def __init__(self, data_dir=None, preset='vgg300', num_train=64, num_valid=16, seed=1234, rank=0, world=1,
                 augment=False, sampler_trials=50, expand_prob=0.5, device=0, device_tensors=True,
                 data_source='pascal_voc', valid_fraction=0.025, images=None, synthetic_classes=20, decoder='pillow', cache_bytes=0,
                 match='reference', shapes_size=(0.2, 0.5), mosaic=0.0, mosaic_center=(0.3, 0.7), mosaic_off_epochs=0, epochs=None):
        """mosaic: the probability that a TRAINING sample becomes a 2 x 2 mosaic of its own picture and three partners
        (needs the transform path: a real data_dir or augment=True); mosaic_center: the range of the centre as fractions of the
        sample's sides; mosaic_off_epochs: the last N of `epochs` (the run's epoch count, which the driver passes) train without."""
        match_id(match)                        # 'reference' or 'paper' (DESIGN.md 29); anything else: ValueError
        self.match = match
        lo, hi = (float(v) for v in shapes_size)   # 'shapes': the rectangles' sides, as fractions of the frame
        if not 0 < lo <= hi <= 1:
            raise ValueError('shapes_size must be (lo, hi) with 0 < lo <= hi <= 1 (got %r)' % (shapes_size,))
        self.shapes_size = (lo, hi)
        if decoder not in DECODERS:
            raise ValueError("decoder must be 'pillow' or 'gpu' (got %r)" % (decoder,))
        if int(cache_bytes) < 0 or (cache_bytes and decoder != 'gpu'):
            raise ValueError("cache_bytes keeps pictures decoded on the GPU: it needs decoder='gpu' and a size >= 0")
        self.decoder, self.cache_bytes = decoder, int(cache_bytes)
        self.mosaic = float(mosaic)
        lo_c, hi_c = (float(v) for v in mosaic_center)
        if not 0.0 <= self.mosaic <= 1.0:
            raise ValueError('mosaic is a probability (got %r)' % (mosaic,))
        if not 0.0 < lo_c <= hi_c < 1.0:
            raise ValueError('mosaic_center must be (lo, hi) with 0 < lo <= hi < 1 (got %r)' % (mosaic_center,))
        if int(mosaic_off_epochs) < 0 or (int(mosaic_off_epochs) > 0 and self.mosaic > 0 and epochs is None):
            raise ValueError('mosaic_off_epochs counts back from the end of the run: it needs epochs, the number of epochs')
        self.mosaic_center, self.mosaic_off_epochs, self.epochs = (lo_c, hi_c), int(mosaic_off_epochs), epochs
        self._arena = None
        self._max_coef_bytes = 0
        self.preset = get_preset_by_name(preset) if isinstance(preset, str) else preset
        self.seed, self.rank, self.world = seed, rank, world
        self.epoch = 0
        self.device, self.device_tensors = device, bool(device_tensors)
        self.global_count = 0
        self._upload_hook = None               # tests: replaces the GPU half of a batch
        self._synthetic_cache = _SharedImageCache(CACHE_SYNTHETIC_UP_TO)
        # where a prefetched epoch's time went (seconds, reset by every gen_batch call with workers): the consumer waiting
        # for a batch, the feeder thread waiting for the workers / for a free device slot / uploading
        # decoder='gpu': samples whose JPEG the GPU decoded / that travelled as pixels / that were served from the arena
        # mosaic > 0: samples that became mosaics / cells planned (a plain sample is one) / INTER_AREA cells that fell back to INTER_LINEAR
        self.feeder_stats = dict(consumer_wait=0.0, worker_wait=0.0, slot_wait=0.0, upload=0.0, batches=0, decoded=0, fallbacks=0, cache_hits=0,
                                 mosaics=0, cells=0, area_fallbacks=0)
        from . import transforms as T
        # 'shapes': the learnable synthetic set (textured rectangles, class = texture; _shapes_canvas) -- same plumbing as
        # 'synthetic', whose uniform-noise images carry nothing a detector could learn
        self._shapes = data_dir == 'shapes'
        self._real_dataset = data_dir not in (None, '', 'synthetic', 'shapes')
        if data_dir not in (None, '', 'synthetic', 'shapes'):
            # ---- a real dataset directory (training_data.py:41-69 + process_dataset.py:199-252) ----
            try:
                source = load_data_source(data_source)
                source.load_trainval_data(data_dir, valid_fraction)
            except (ImportError, AttributeError, OSError) as e:
                raise RuntimeError(str(e))                                              # training_data.py:48-49
            self.num_classes = source.num_classes
            self.label_colors = source.colors
            self.lid2name, self.lname2id = source.lid2name, source.lname2id
            self.train_samples, self.valid_samples = list(source.train_samples), list(source.valid_samples)
            self.num_train, self.num_valid = len(self.train_samples), len(self.valid_samples)
            self.augment = True
            self.train_transforms = T.build_train_transforms(self.preset, self.num_classes, sampler_trials, expand_prob, images, decoder, match)
            self.valid_transforms = T.build_valid_transforms(self.preset, self.num_classes, images, decoder, match)
            self._max_image_bytes = max([s.imgsize.w * s.imgsize.h * 3 for s in self.train_samples + self.valid_samples] + [1])
            if decoder == 'gpu':
                # int16 coefficients: at most 6 bytes per pixel of the MCU-padded frame (4:4:4; an MCU is at most 16 x 16)
                self._max_coef_bytes = max([6 * ((s.imgsize.w + 15) // 16 * 16) * ((s.imgsize.h + 15) // 16 * 16)
                                            for s in self.train_samples + self.valid_samples] + [1])
                self._arena = _SourceArena(self.cache_bytes, self._max_image_bytes)
            self._recipes = {
                'train': _Recipe(self, 'train', self.num_train, 0, _SampleAt(self, 'train', 0), self.train_transforms),
                'valid': _Recipe(self, 'valid', self.num_valid, 1 << 20, _SampleAt(self, 'valid', 1 << 20), self.valid_transforms)}
        else:
            # the synthetic sets: `synthetic_classes` class ids ('shapes' draws its textures from the first four)
            if not 1 <= int(synthetic_classes) <= MAX_CLASSES:
                raise RuntimeError('synthetic_classes must be in 1..%d (got %s)' % (MAX_CLASSES, synthetic_classes))
            self.num_classes = int(synthetic_classes)
            self.label_colors = {}
            self.lid2name = dict(enumerate(default_class_names(self.num_classes)))
            self.lname2id = {n: i for i, n in self.lid2name.items()}
            self.num_train, self.num_valid = num_train, num_valid
            self.augment = bool(augment)
            if self.augment:
                self.train_transforms = T.build_train_transforms(self.preset, self.num_classes, sampler_trials, expand_prob, match=match)
                self.valid_transforms = T.build_valid_transforms(self.preset, self.num_classes, match=match)
                self.train_samples = [self._dataset_sample(i, 0)[1] for i in range(num_train)]
                self.valid_samples = [self._dataset_sample(i, 1 << 20)[1] for i in range(num_valid)]
                self._max_image_bytes = 640 * 640 * 3
                self._recipes = {
                    'train': _Recipe(self, 'train', num_train, 0, _SampleAt(self, 'train', 0), self.train_transforms),
                    'valid': _Recipe(self, 'valid', num_valid, 1 << 20, _SampleAt(self, 'valid', 1 << 20), self.valid_transforms)}
            else:
                self.train_samples = self.valid_samples = None
                self._recipes = {'train': _Recipe(self, 'train', num_train, 0), 'valid': _Recipe(self, 'valid', num_valid, 1 << 20)}
        if self.mosaic > 0 and self._recipes['train'].transforms is None:
            raise ValueError('mosaic needs the transform path: a real data_dir or augment=True')
        self._scale_arena()
        self.train_generator = self._make_generator(self._recipes['train'])
        self.valid_generator = self._make_generator(self._recipes['valid'])

    # ---- what travels to a worker process (forkserver / spawn start: _start_context) ------------------------------
    def __getstate__(self):
        st = dict(self.__dict__)
        for k in ('_upload_hook', 'train_generator', 'valid_generator', '_arena'):
            st[k] = None
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)

    # ---- lifetime of the worker processes ----------------------------------------------------------------------
    def close(self):
        for r in self._recipes.values():
            if r.pool is not None:
                r.pool.close()
                r.pool = None
            r.dev = None
        if self._arena is not None:            # the cached pictures go with the buffer
            self._arena = _SourceArena(self.cache_bytes, self._arena.max_image_bytes)
            self._scale_arena()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- mosaic augmentation -------------------------------------------------------------------------------------------------
    def mosaic_prob(self, recipe, epoch):
        """The mosaic probability of a data set in an epoch: validation never mosaics, nor do the last mosaic_off_epochs epochs."""
        if self.mosaic <= 0 or recipe.which != 'train' or recipe.transforms is None:
            return 0.0
        if self.mosaic_off_epochs > 0 and int(epoch) >= int(self.epochs) - self.mosaic_off_epochs:
            return 0.0
        return self.mosaic

    def sources_per_batch(self, recipe, batch_size):
        """How many source pictures a batch of a data set can carry: what the slots, the staging tensors, the source arena's scratch
        and the kernels' workspace are sized for."""
        return batch_size * (4 if self.mosaic > 0 and recipe.which == 'train' and recipe.transforms is not None else 1)

    def _scale_arena(self):
        """the arena's scratch regions per data set: the training set's hold four sources per sample with mosaics, the validation
        set's keep their size"""
        if self._arena is not None:
            self._arena.scale = {w: self.sources_per_batch(r, 1) for w, r in self._recipes.items()}

    def _note_mosaics(self, stats, arrays):
        if 'mosaic_stats' in arrays:
            m = arrays['mosaic_stats']
            stats['mosaics'] += int(m[0]); stats['cells'] += int(m[1]); stats['area_fallbacks'] += int(m[2])

    def _sample_seed(self, salt, epoch, index):
        """The seed of sample #index's decisions in `epoch` of data set `salt`: one integer whose 32-bit words all
        enter random.seed's init_by_array."""
        return ((int(self.seed) & 0xffffffff) << 96) | (int(salt) << 64) | (int(epoch) << 32) | int(index)

    # ---- labels: encoded once per batch on the GPU, left there ---------------------------------------------------
    def _labels(self, gts, out=None):
        bxs, cls = _gt_arrays(gts)
        if self.device_tensors:
            return encode_labels_batch_dev(self.preset, self.num_classes, bxs, cls, self.device, out=out, match=self.match)
        return encode_labels_batch(self.preset, self.num_classes, bxs, cls, match=self.match)

    # ---- the learnable synthetic set ('shapes') --------------------------------------------------------------------
    SHAPE_CLASSES = 4      # textures, booked under the first four class ids (the net keeps the benchmark's shape)

    def _shapes_canvas(self, rng, W, H):
        """uint8 BGR image [H, W, 3] + boxes: 1..3 non-overlapping rectangles of 20..50 % of the frame (shapes_size) on low-contrast
        noise, each filled with a two-colour texture that IS its class -- 0 horizontal stripes, 1 vertical stripes,
        2 checkerboard, 3 diagonal stripes (either direction: a horizontal flip keeps every class).  Texture, not colour,
        because the reference's training recipe permutes channels and shifts hue / saturation / contrast
        (process_dataset.py:66-140, transforms.py:117-240): a colour code would not survive it."""
        img = rng.integers(104, 152, (H, W, 3), dtype=np.uint8)
        n = int(rng.integers(1, 4))
        placed = []
        for _ in range(n):
            for _try in range(20):
                w, h = rng.uniform(self.shapes_size[0], self.shapes_size[1], 2)
                cx, cy = rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2)
                if all(abs(cx - q[0]) >= (w + q[2]) / 2 or abs(cy - q[1]) >= (h + q[3]) / 2 for q in placed):
                    placed.append((float(cx), float(cy), float(w), float(h)))
                    break
        boxes = []
        for cx, cy, w, h in placed:
            c = int(rng.integers(0, min(self.SHAPE_CLASSES, self.num_classes)))
            x0, x1 = int(round((cx - w / 2) * W)), int(round((cx + w / 2) * W))
            y0, y1 = int(round((cy - h / 2) * H)), int(round((cy + h / 2) * H))
            p = int(rng.integers(5, 12)) * max(1, min(W, H) // 300)          # stripe width in pixels
            yy, xx = np.mgrid[y0:y1, x0:x1]
            sgn = 1 if rng.integers(0, 2) else -1
            pat = [(yy // p) % 2, (xx // p) % 2, (yy // p + xx // p) % 2, ((yy + sgn * xx) // p) % 2][c].astype(bool)
            lo, hi = rng.integers(0, 64, 3), rng.integers(192, 256, 3)
            img[y0:y1, x0:x1] = np.where(pat[..., None], hi, lo).astype(np.uint8)
            boxes.append(Box(self.lid2name[c], c, Point(cx, cy), Size(w, h)))
        return img, boxes

    # ---- a dataset of variously sized uint8 images through the reference's transform recipe ---------------------
    def _dataset_sample(self, index, salt):
        """Deterministic synthetic "file" #index: ({name: uint8 BGR image}, Sample record with 1..5 boxes)."""
        key = (salt, index)
        hit = self._synthetic_cache.get(key)
        if hit is not None:
            return hit
        rng = np.random.default_rng([self.seed, salt, index, 77])
        W, H = int(rng.integers(200, 640)), int(rng.integers(200, 640))
        if self._shapes:
            img, boxes = self._shapes_canvas(rng, W, H)
            name = 'shapes/%d/%d' % (salt, index)
            out = ({name: img}, Sample(name, boxes, Size(W, H)))
            self._synthetic_cache.put(key, name, img, out[1])
            return out
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        n = int(rng.integers(1, 6))
        w = rng.uniform(0.1, 0.6, n); h = rng.uniform(0.1, 0.6, n)
        cx = rng.uniform(w / 2, 1 - w / 2); cy = rng.uniform(h / 2, 1 - h / 2)
        cls = rng.integers(0, self.num_classes, n)
        boxes = [Box(self.lid2name[int(c)], int(c), Point(float(x), float(y)), Size(float(ww), float(hh)))
                 for x, y, ww, hh, c in zip(cx, cy, w, h, cls)]
        name = 'synthetic/%d/%d' % (salt, index)
        out = ({name: img}, Sample(name, boxes, Size(W, H)))
        self._synthetic_cache.put(key, name, img, out[1])
        return out

    # ---- preset-sized float32 synthetic images (no transform recipe) ------------------------------------------------
    def _sample(self, index, salt):
        """Deterministic synthetic sample #index: image + 1..5 GT boxes."""
        rng = np.random.default_rng([self.seed, salt, index])
        H, W = self.preset.image_size.h, self.preset.image_size.w
        if self._shapes:
            img, gt = self._shapes_canvas(rng, W, H)
            return img.astype(np.float32), gt
        img = rng.integers(0, 256, (H, W, 3)).astype(np.float32)        # BGR 0..255, training_data.py:100
        n = int(rng.integers(1, 6))
        w = rng.uniform(0.1, 0.6, n); h = rng.uniform(0.1, 0.6, n)
        boxes = np.stack([rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2), w, h], 1)
        cls = rng.integers(0, self.num_classes, n)
        gt = [Box(self.lid2name[int(ci)], int(ci), Point(*map(float, bi[:2])), Size(*map(float, bi[2:]))) for bi, ci in zip(boxes, cls)]
        return img, gt

    # ---- GPU half of a batch ------------------------------------------------------------------------------------------
    def _device_ring(self, recipe, batch_size):
        """Three device slots (images, labels, staging for the source bytes, tap-table workspace) + the feeder stream, PER DATA
        SET: a training and a validation generator may be live at the same time (the reference's queues are independent,
        training_data.py:147-195) and must not fill each other's slots.  Never replaced under a live generator (_prefetched
        refuses a second generator of the same data set)."""
        import torch
        from ._lib import lib
        d = recipe.dev
        if d is not None and d['batch'] >= batch_size:
            return d
        dev = torch.device('cuda', self.device)
        W, H = self.preset.image_size.w, self.preset.image_size.h
        A, nv = self.preset.num_anchors, self.num_classes + 5
        n_src = self.sources_per_batch(recipe, batch_size)
        ws_bytes = lib.ssd_augment_ws_bytes(batch_size, W, H) if n_src == batch_size else lib.ssd_augment_cells_ws_bytes(n_src, W, H)
        d = {'batch': batch_size, 'sources': n_src, 'stream': torch.cuda.Stream(device=dev),
             'images': [torch.empty((batch_size, H, W, 3), dtype=torch.float32, device=dev) for _ in range(DEVICE_SLOTS)],
             'labels': [torch.empty((batch_size, A, nv), dtype=torch.float32, device=dev) for _ in range(DEVICE_SLOTS)],
             'packed': [None] * DEVICE_SLOTS, 'enc_ws': [None] * DEVICE_SLOTS, 'jpeg_ws': [None] * DEVICE_SLOTS,
             'ws': [torch.empty((ws_bytes,), dtype=torch.uint8, device=dev) for _ in range(DEVICE_SLOTS)]}
        recipe.dev = d
        return d

    def _known(self, recipe, idx, epoch=0):
        """{position in the batch's source list: (h, w)} of the source pictures that lie in the arena (what a task tells its worker),
        else None.  The source list is idx itself, or with mosaics every sample's picture and partners (_Recipe.sources)."""
        arena = self._arena
        if arena is None or not arena.table or not recipe.gpu_decode:
            return None
        if self.mosaic_prob(recipe, epoch) > 0:
            idx = [i for srcs, _ in recipe.sources(epoch, idx) for i in srcs]
        hits = {k: arena.table.get((recipe.which, int(i))) for k, i in enumerate(idx)}
        return {k: (e[1], e[2]) for k, e in hits.items() if e is not None} or None

    def _decode_sources(self, recipe, idx, arrays, slot, ring, coef_dev, packed_dev):
        """decoder='gpu': the batch's source pictures into the arena, on torch's current stream -> (arena buffer, the batch's
        ssd_augment_params with src_off = where each picture lies in it).  coef_dev / packed_dev: the worker's 'coef' and 'packed'
        arrays on the GPU (uint8 views).  A picture that is not cached yet is decoded (copied, for a fallback's pixels) into the
        arena's next free bytes and entered; when the arena is full, or the sample was cached while its task was under way, into
        this slot's scratch region.  Nothing is waited for."""
        import ctypes as C
        import torch
        from . import jpeg as J, transforms as T
        from ._lib import lib, check, last_error
        arena, stats = self._arena, recipe.stats          # (the stats of THIS data set's generator: two may be live)
        dev = torch.device('cuda', self.device)
        cur = torch.cuda.current_stream(dev)
        idx = arrays['src_idx'] if 'src_idx' in arrays else idx      # per SOURCE picture: a mosaic's partners are cached like any sample
        b = len(idx)
        kind = arrays['src_kind']
        params = (T._Params * b).from_buffer_copy(arrays['params'].tobytes())
        nd = int(np.count_nonzero(kind == SRC_COEF))
        if arrays['descs'].nbytes != nd * C.sizeof(J.Desc):
            raise RuntimeError('the batch carries %d descriptor bytes for %d JPEGs' % (arrays['descs'].nbytes, nd))
        descs = (J.Desc * max(nd, 1)).from_buffer_copy(arrays['descs'].tobytes() if nd else bytes(C.sizeof(J.Desc)))
        with arena.lock:
            buf = arena.buf
            if arena.event is not None and arena.event_stream != cur.cuda_stream:
                cur.wait_event(arena.event)          # entries appended on another stream (the other data set's feeder)
            base, room = arena.region(recipe.which, slot)
            scratch, j, at, appended = 0, 0, 0, False
            for k in range(b):
                h, w = params[k].src_h, params[k].src_w
                n = h * w * 3
                need = (n + 15) // 16 * 16
                key = (recipe.which, int(idx[k]))
                entry = arena.table.get(key)
                if kind[k] == SRC_CACHED:
                    if entry is None or entry[1:] != (h, w):
                        raise RuntimeError('sample %d of the %s set was planned as cached and is not in the arena' % (idx[k], recipe.which))
                    off = entry[0]
                    stats['cache_hits'] += 1
                else:
                    if entry is None and arena.used + need <= arena.cache_bytes:
                        off = arena.used
                        arena.used += need
                        arena.table[key] = (off, h, w)
                        appended = True
                    else:
                        if scratch + need > room:
                            raise RuntimeError('a batch of the %s set needs more than the %d bytes of source scratch its sample list announced '
                                               '(images larger than their imgsize?)' % (recipe.which, room))
                        off = base + scratch
                        scratch += need
                    if kind[k] == SRC_COEF:
                        descs[j].dst_off = off
                        j += 1
                        stats['decoded'] += 1
                    else:
                        if at + n > packed_dev.numel():
                            raise RuntimeError("the batch's 'packed' array is shorter than its host-pixel samples")
                        buf[off:off + n].copy_(packed_dev[at:at + n], non_blocking=True)
                        at += need
                        stats['fallbacks'] += 1
                params[k].src_off = off
            if nd:
                ws_bytes = lib.ssd_jpeg_ws_bytes(descs, nd)
                if ws_bytes == 0:
                    raise RuntimeError(last_error())
                ws = ring['jpeg_ws'][slot] if ring is not None else None
                if ws is None or ws.numel() < ws_bytes:          # (allocated under the current stream: the feeder's, in the ring)
                    ws = torch.empty((ws_bytes + ws_bytes // 4,), dtype=torch.uint8, device=dev)
                    if ring is not None:
                        ring['jpeg_ws'][slot] = ws
                check(lib.ssd_jpeg_decode_batch_dev(coef_dev.data_ptr(), coef_dev.numel(), descs, nd, buf.data_ptr(), buf.numel(),
                                                    ws.data_ptr(), ws.numel(), cur.cuda_stream))
            if appended:
                arena.event = torch.cuda.Event()
                arena.event.record(cur)
                arena.event_stream = cur.cuda_stream
        return buf, params

    def _upload(self, arrays, gts, slot=None, ring=None, recipe=None, idx=None):
        """Source bytes up, augmentation + label kernels on torch's current stream -> (images, labels) of this batch.
        slot None: fresh tensors (the serial generator); else the device slot to fill."""
        if self._upload_hook is not None:
            return self._upload_hook(arrays, gts, slot)
        import ctypes as C
        import torch
        from ._lib import lib, check
        b = len(gts)
        dev = torch.device('cuda', self.device)
        W, H = self.preset.image_size.w, self.preset.image_size.h
        ring = ring if slot is not None else None
        cells = arrays.get('cells')
        n_src = b if cells is None else int(cells.shape[0])
        ws_bytes = lambda: lib.ssd_augment_ws_bytes(b, W, H) if cells is None else lib.ssd_augment_cells_ws_bytes(n_src, W, H)
        if 'images' in arrays:
            src = torch.from_numpy(arrays['images'])
            if ring is not None:
                images = ring['images'][slot][:b]
                images.copy_(src, non_blocking=True)
            else:
                images = src.to(dev, non_blocking=True) if self.device_tensors else arrays['images']
        else:
            packed, params = arrays['packed'], arrays['params']
            if 'descs' in arrays:                # decoder='gpu': coefficients and the fallbacks' pixels up, the decode in front
                as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).to(dev)
                staged, params = self._decode_sources(recipe, idx, arrays, slot, ring, as_dev(arrays['coef']), as_dev(packed))
                if ring is not None:
                    images, ws = ring['images'][slot][:b], ring['ws'][slot]
                else:
                    images = torch.empty((b, H, W, 3), dtype=torch.float32, device=dev)
                    ws = torch.empty((ws_bytes(),), dtype=torch.uint8, device=dev)
                params = np.frombuffer(params, np.uint8)
            elif ring is not None:
                if ring['packed'][slot] is None or ring['packed'][slot].numel() < packed.size:
                    ring['packed'][slot] = torch.empty((max(packed.size, ring['sources'] * (self._max_image_bytes + 16)),), dtype=torch.uint8, device=dev)
                staged = ring['packed'][slot][:packed.size]
                staged.copy_(torch.from_numpy(packed), non_blocking=True)
                images, ws = ring['images'][slot][:b], ring['ws'][slot]
            else:
                staged = torch.from_numpy(packed).to(dev)
                images = torch.empty((b, H, W, 3), dtype=torch.float32, device=dev)
                ws = torch.empty((ws_bytes(),), dtype=torch.uint8, device=dev)
            self._augment(staged.data_ptr(), C.c_void_p(params.ctypes.data), cells, b, images, ws, torch.cuda.current_stream(dev).cuda_stream)
            if not self.device_tensors:
                images = images.cpu().numpy()
        labels = self._labels(gts, out=ring['labels'][slot][:b] if ring is not None else None)
        return images, labels

    def _augment(self, src_ptr, params, cells, b, images, ws, stream):
        """The batch's augmentation kernels: one picture per sample (ssd_augment_batch_dev, whenever the batch carries no cells), or
        the sources into their cells (ssd_augment_cells_dev)."""
        import ctypes as C
        from ._lib import lib, check
        W, H = self.preset.image_size.w, self.preset.image_size.h
        if cells is None:
            check(lib.ssd_augment_batch_dev(src_ptr, params, b, W, H, images.data_ptr(), ws.data_ptr(), stream))
            return
        cells = np.ascontiguousarray(cells, np.int32)
        need = lib.ssd_augment_cells_ws_bytes(int(cells.shape[0]), W, H)
        if ws.numel() < need:
            raise RuntimeError('a batch of %d source pictures needs %d bytes of augmentation workspace, the slot has %d' % (cells.shape[0], need, ws.numel()))
        check(lib.ssd_augment_cells_dev(src_ptr, params, C.c_void_p(cells.ctypes.data), int(cells.shape[0]), b, W, H, images.data_ptr(), ws.data_ptr(),
                                        stream))

    def _upload_async(self, ring, slot_arr, arrays, gts, dslot, recipe=None, idx=None):
        """The prefetching feeder's upload: ONE host-to-device transfer of the slot's used prefix (source bytes, parameter
        records, boxes), then the augmentation and label kernels, all enqueued on torch's current stream; nothing is waited
        for.  `arrays` are views into slot_arr (pinned when the registration succeeded): the slot must stay untouched until
        the returned work has run."""
        import ctypes as C
        import torch
        from ._lib import lib, check
        b = len(gts)
        dev = torch.device('cuda', self.device)
        W, H = self.preset.image_size.w, self.preset.image_size.h
        stream = torch.cuda.current_stream(dev).cuda_stream
        base = slot_arr.ctypes.data
        offs = {k: v.ctypes.data - base for k, v in arrays.items()}
        big = 'images' if 'images' in arrays else None
        small = [k for k in arrays if k != big and arrays[k].nbytes]
        lo = min(offs[k] for k in small)
        hi = max(offs[k] + arrays[k].nbytes for k in small)
        need = hi - lo
        staged = ring['packed'][dslot]
        if staged is None or staged.numel() < need:
            per_image = max(getattr(self, '_max_image_bytes', 0), self._max_coef_bytes + 512 if self._max_coef_bytes else 0)
            cap = max(need, ring['sources'] * (per_image + 16 + 256 + 4096) + 8192)
            staged = ring['packed'][dslot] = torch.empty((cap,), dtype=torch.uint8, device=dev)
        staged[:need].copy_(torch.from_numpy(slot_arr[lo:hi]), non_blocking=True)
        sp = staged.data_ptr() - lo
        images = ring['images'][dslot][:b]
        if big:
            images.copy_(torch.from_numpy(arrays['images']), non_blocking=True)
        elif 'descs' in arrays:
            part = lambda k: staged[offs[k] - lo:offs[k] - lo + arrays[k].nbytes] if arrays[k].nbytes else staged[:0]
            src, params = self._decode_sources(recipe, idx, arrays, dslot, ring, part('coef'), part('packed'))
            self._augment(src.data_ptr(), C.cast(params, C.c_void_p), arrays.get('cells'), b, images, ring['ws'][dslot], stream)
        else:
            self._augment(sp + offs['packed'], C.c_void_p(arrays['params'].ctypes.data), arrays.get('cells'), b, images, ring['ws'][dslot], stream)
        ntot = int(arrays['gcls'].shape[0])
        mid = match_id(self.match)
        ws_need = lib.ssd_encode_labels_ws_bytes_ex(ntot, b, mid)
        if ring['enc_ws'][dslot] is None or ring['enc_ws'][dslot].numel() < ws_need:
            ring['enc_ws'][dslot] = torch.empty((max(ws_need, lib.ssd_encode_labels_ws_bytes_ex(ring['batch'] * 16, ring['batch'], mid)),),
                                                dtype=torch.uint8, device=dev)
        labels = ring['labels'][dslot][:b]
        check(lib.ssd_encode_labels_resident_ex(self.preset.name.encode(), self.num_classes, self.device, sp + offs['gt'], sp + offs['gcls'],
                                                sp + offs['goff'], b, ntot, labels.data_ptr(), ring['enc_ws'][dslot].data_ptr(), stream,
                                                mid, None))
        return images, labels

    # ---- the generators ----------------------------------------------------------------------------------------------
    def _make_generator(self, recipe):
        def gen_batch(batch_size, num_workers=0):
            sampler = ShardSampler(recipe.total, batch_size, self.rank, self.world, self.seed + recipe.salt)
            batches = list(sampler.batches_with_count(self.epoch))
            arena = self._arena if recipe.gpu_decode and self._upload_hook is None else None
            if arena is not None:
                import torch
                arena.ensure(batch_size, torch.device('cuda', self.device), any(r.active for r in self._recipes.values()))
            if num_workers and num_workers > 0 and (self.device_tensors or self._upload_hook is not None):
                yield from self._prefetched(recipe, batches, self.epoch, batch_size, int(num_workers))
                return
            self.feeder_stats.update(mosaics=0, cells=0, area_fallbacks=0)
            if arena is not None:
                self.feeder_stats.update(decoded=0, fallbacks=0, cache_hits=0)
                recipe.stats = self.feeder_stats
            for idx, count in batches:
                if len(idx) == 0:              # an empty shard of a short last batch: the rank still takes the step
                    self.global_count = count
                    yield None, None, []
                    continue
                arrays, gts = recipe.plan(self.epoch, idx, self._known(recipe, idx, self.epoch) if arena is not None else None)
                self._note_mosaics(self.feeder_stats, arrays)
                images, labels = self._upload(arrays, gts, recipe=recipe, idx=idx)
                self.global_count = count
                yield images, labels, gts
        return gen_batch

    def _prefetched(self, recipe, batches, epoch, batch_size, num_workers):
        import torch
        if recipe.active:
            raise RuntimeError('one %s generator at a time: finish or close the previous one first' % recipe.which)
        slot_bytes = recipe.slot_bytes(batch_size)
        pool = recipe.pool
        if pool is not None and (pool.num_workers != num_workers or pool.slot_bytes < slot_bytes):
            pool.close()
            pool = None
        if pool is None:
            prime_anchor_table(self.preset)              # the workers must find it: they never call the GPU
            pool = recipe.pool = _WorkerPool(recipe, num_workers, slot_bytes)
        use_gpu = self._upload_hook is None
        if use_gpu:
            pool.pin(self.device)
            ring = self._device_ring(recipe, batch_size)
            fstream = ring['stream']
            dev = torch.device('cuda', self.device)
            # the device slots start out free: whatever the caller still has enqueued on batches of an earlier generator
            # (the last steps of the previous epoch) reads them and must have run before the first uploads land
            fstream.wait_stream(torch.cuda.current_stream(dev))
        pool.generation += 1
        gen = pool.generation
        nb = len(batches)
        ready = queue.Queue()
        dev_free = queue.Queue()
        for s in range(DEVICE_SLOTS):
            dev_free.put((s, None))
        cancel = threading.Event()
        stats = self.feeder_stats = dict(consumer_wait=0.0, worker_wait=0.0, slot_wait=0.0, upload=0.0, host_slot_wait=0.0, batches=0,
                                         decoded=0, fallbacks=0, cache_hits=0, mosaics=0, cells=0, area_fallbacks=0)
        cached = use_gpu and recipe.gpu_decode
        recipe.stats = stats
        clock = time.perf_counter
        inflight = []          # (host slot, event behind its upload): the slot returns to the pool when the event has passed

        def reap(block):
            """host slots whose upload has run; block: wait for the oldest one when none is free"""
            while inflight and (inflight[0][1] is None or inflight[0][1].query()):
                pool.free_slots.append(inflight.pop(0)[0])
            if block and inflight and not pool.free_slots:
                t0 = clock()
                inflight[0][1].synchronize()
                stats['host_slot_wait'] += clock() - t0
                pool.free_slots.append(inflight.pop(0)[0])

        def feeder():
            try:
                next_submit = next_upload = 0
                done = {}
                while next_upload < nb and not cancel.is_set():
                    reap(block=next_submit < nb and next_upload not in done and len(pool.outstanding) == 0)
                    while next_submit < nb and (len(batches[next_submit][0]) == 0 or pool.free_slots):
                        idx = batches[next_submit][0]
                        if len(idx) == 0:
                            done[next_submit] = None
                        else:
                            slot = pool.free_slots.pop()
                            pool.outstanding[(gen, next_submit)] = slot
                            pool.tasks.put((gen, next_submit, slot, epoch, np.asarray(idx), self._known(recipe, idx, epoch) if cached else None))
                        next_submit += 1
                    if next_upload in done:
                        item = done.pop(next_upload)
                        count = batches[next_upload][1]
                        if item is None:
                            ready.put((next_upload, None, 0, [], count, None))
                            next_upload += 1
                            continue
                        hslot, arrays, gts = item
                        t0 = clock()
                        while True:
                            try:
                                dslot, released = dev_free.get(timeout=0.2)
                                break
                            except queue.Empty:
                                if cancel.is_set():
                                    return
                        t1 = clock()
                        stats['slot_wait'] += t1 - t0
                        self._note_mosaics(stats, arrays)
                        if use_gpu:
                            slot_arr = pool.results.array_pool[hslot]
                            in_slot = all(isinstance(v, np.ndarray) and v.base is not None and
                                          (v.nbytes == 0 or slot_arr.ctypes.data <= v.ctypes.data < slot_arr.ctypes.data + slot_arr.nbytes)
                                          for v in arrays.values())
                            idx = batches[next_upload][0]
                            with torch.cuda.stream(fstream):
                                if released is not None:
                                    fstream.wait_event(released)
                                if in_slot:      # enqueue and move on: the consumer's stream waits for the event, not this thread
                                    images, labels = self._upload_async(ring, slot_arr, arrays, gts, dslot, recipe, idx)
                                else:            # a batch that did not fit its slot came through the pipe: the serial upload
                                    images, labels = self._upload(arrays, gts, dslot, ring, recipe, idx)
                                ev = torch.cuda.Event()
                                ev.record(fstream)
                            inflight.append((hslot, ev))
                        else:
                            images, labels = self._upload(arrays, gts, dslot)
                            ev = None
                            pool.free_slots.append(hslot)
                        stats['upload'] += clock() - t1
                        stats['batches'] += 1
                        ready.put((next_upload, dslot, len(gts), (images, labels, gts), count, ev))
                        next_upload += 1
                        continue
                    t0 = clock()
                    try:
                        tag, hslot, arrays, gts = pool.results.get(timeout=0.5)
                    except queue.Empty:
                        stats['worker_wait'] += clock() - t0
                        pool.check_alive()
                        continue
                    except WorkerError as e:
                        pool.outstanding.pop(e.tag, None)
                        if e.tag[0] != gen:
                            continue
                        raise
                    stats['worker_wait'] += clock() - t0
                    pool.outstanding.pop(tag, None)
                    if tag[0] != gen:                      # a batch of an abandoned epoch
                        pool.free_slots.append(hslot)
                        continue
                    done[tag[1]] = (hslot, arrays, gts)
            except BaseException as e:
                ready.put(e)
            finally:
                for hslot, ev in inflight:
                    if ev is not None:
                        try:
                            ev.synchronize()
                        except Exception:
                            pass
                del inflight[:]

        recipe.active = True
        th = threading.Thread(target=feeder, name='ssd-feeder-' + recipe.which, daemon=True)
        th.start()
        try:
            for k in range(nb):
                t0 = clock()
                item = ready.get()
                stats['consumer_wait'] += clock() - t0
                if isinstance(item, BaseException):
                    raise item
                seq, dslot, n, payload, count, ev = item
                assert seq == k
                if dslot is None:
                    self.global_count = count
                    yield None, None, []
                    continue
                images, labels, gts = payload
                if ev is not None:
                    torch.cuda.current_stream(dev).wait_event(ev)
                self.global_count = count
                yield images, labels, gts
                # the caller is back for the next batch: what it enqueued on its stream reads this slot
                released = None
                if use_gpu:
                    released = torch.cuda.Event()
                    released.record(torch.cuda.current_stream(dev))
                dev_free.put((dslot, released))
        finally:
            cancel.set()
            th.join()
            recipe.active = False
            # slots of results that were received but never uploaded go back; tasks still in flight are
            # recognised by their generation when they arrive
            while True:
                try:
                    item = ready.get_nowait()
                except queue.Empty:
                    break
            self._reclaim(pool, gen)

    @staticmethod
    def _reclaim(pool, gen):
        """After a generator ended (exhausted or abandoned): wait for the tasks of generation `gen` that are still with
        the workers and take their slots back."""
        while pool.outstanding:
            try:
                tag, hslot, _, _ = pool.results.get(timeout=5.0)
            except queue.Empty:
                pool.check_alive()
                continue
            except WorkerError as e:
                tag = e.tag
            pool.outstanding.pop(tag, None)
        pool.outstanding.clear()
        pool.free_slots = list(range(pool.nslots))
