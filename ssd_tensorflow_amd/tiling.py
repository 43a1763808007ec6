"""Tiled detection for large pictures: a picture is cut into overlapping windows, every window goes through the
network as an input of its own, and the windows' boxes are merged into one detection list per picture on the GPU
(ssd_merge_tiles_dev).  The decoded picture, the windows' network inputs, the per-window records and the merged detections all
stay in device memory; the host plans the windows and collects the (small) result.

  plan_tiles       the windows of a picture
  tile_plan        the network input of a window: an ImagePlan (crop + INTER_LINEAR resize) on the picture where it lies
  TiledDetector    planning, inference, decode and merge of a batch of pictures; the drivers' --tile
  source_batches   the drivers' pictures as device buffers, batch by batch
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import lib, check

Tile = namedtuple('Tile', ['x0', 'y0', 'w', 'h', 'interior'])

LEFT, RIGHT, TOP, BOTTOM = 1, 2, 4, 8


class TileStruct(C.Structure):
    """ssd_tile (include/ssdvgg_hip.h)"""
    _fields_ = [(n, C.c_int) for n in ('x0', 'y0', 'w', 'h', 'img_w', 'img_h', 'interior', 'image')]


def _windows(n, tile, overlap):
    """(start, length) of the windows along an axis of n pixels: the last one is shifted back, never clipped"""
    if n <= tile:
        return [(0, n)]
    stride = max(1, int(tile * (1 - overlap)))
    k = -(-(n - tile) // stride) + 1
    return [(min(i * stride, n - tile), tile) for i in range(k)]


def plan_tiles(w, h, tile, overlap=0.25, whole=True):
    """The windows of a w x h picture, row-major (y outer), in source pixels; with `whole` and more than one window the whole
    picture (the ordinary shrunk view, which keeps the large objects) comes last.  interior: which edges of a window lie inside
    the picture (LEFT 1, RIGHT 2, TOP 4, BOTTOM 8); the whole-picture view has none."""
    w, h, tile = int(w), int(h), int(tile)
    if w < 1 or h < 1:
        raise ValueError('a picture of %d x %d has no tiles' % (w, h))
    if tile < 32:
        raise ValueError('tile must be at least 32 pixels (got %d)' % tile)
    if not 0 <= overlap <= 0.9:
        raise ValueError('overlap must lie in 0 .. 0.9 (got %r)' % (overlap,))
    out = []
    for y0, th in _windows(h, tile, overlap):
        for x0, tw in _windows(w, tile, overlap):
            interior = (LEFT if x0 > 0 else 0) | (RIGHT if x0 + tw < w else 0) | (TOP if y0 > 0 else 0) | (BOTTOM if y0 + th < h else 0)
            out.append(Tile(x0, y0, tw, th, interior))
    if whole and len(out) > 1:
        out.append(Tile(0, 0, w, h, 0))
    return out


def tile_plan(source, t, net_w, net_h):
    """The network input of window t of `source` (a uint8 [H, W, 3] host array or a device triple (buffer, offset, (H, W))): what
    the existing path gives for that crop saved as a picture of its own -- the resize sees the window and nothing outside it."""
    from . import transforms as T
    plan = T.ImagePlan(source)
    plan.crop = (t.x0, t.y0, t.w, t.h)
    plan.resize = (int(net_w), int(net_h), T.INTER_LINEAR)
    return plan


def tile_structs(tiles):
    """ctypes array of ssd_tile for a list of (image, Tile, (W, H))"""
    arr = (TileStruct * max(len(tiles), 1))()
    for k, (image, t, (W, H)) in enumerate(tiles):
        arr[k].x0, arr[k].y0, arr[k].w, arr[k].h = int(t.x0), int(t.y0), int(t.w), int(t.h)
        arr[k].img_w, arr[k].img_h, arr[k].interior, arr[k].image = int(W), int(H), int(t.interior), int(image)
    return arr


def merge_limits():
    """(tiles per picture, tiles of a picture * tile_cap, candidates sorted in LDS) of ssd_merge_tiles"""
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    check(lib.ssd_merge_tiles_limits(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


class _TileDetections:
    """Ticket of TiledDetector.launch: get() waits for the pass's one event and yields one dict {conf, cls, idx, tile, box} per
    picture -- views of the pinned host copy of one of the detector's two output sets, valid until the second-next launch.
    count_dev / cls_dev / box_dev / out_cap: the device arrays annotate.annotate_batch draws from."""

    def __init__(self, owner, serial, dev, host, done, n_images, out_cap, tiles):
        self.owner, self.serial, self._dev, self._host, self.done = owner, serial, dev, host, done
        self.b, self.out_cap, self.tiles = n_images, out_cap, tiles
        self.count_dev, self.cls_dev, self.box_dev = dev['count'].data_ptr(), dev['cls'].data_ptr(), dev['box'].data_ptr()
        self.conf_dev = dev['conf'].data_ptr()

    def dev_slots(self):
        """(count, conf, cls, box, b, out_cap, stream) of the merged detections (average_precision.DeviceAPCalculator.add_pass)"""
        if self.owner._serial != self.serial:
            raise RuntimeError('the slots of these detections belong to an earlier pass: use them right after the launch')
        return (self.count_dev, self.conf_dev, self.cls_dev, self.box_dev, self.b, self.out_cap, getattr(self.owner.net, '_stream_ptr', 0))

    def get(self):
        if self.owner._serial - self.serial not in (0, 1):
            raise RuntimeError('these detections were overwritten: only the two most recent passes are kept')
        self.done.synchronize()
        h = {k: v.numpy() for k, v in self._host.items()}
        out = []
        for i in range(self.b):
            n = min(int(h['count'][i]), self.out_cap)
            out.append({k: h[k][i, :n] for k in ('conf', 'cls', 'idx', 'tile', 'box')})
        return out


class TiledDetector:
    """Detection on pictures cut into tiles.  launch(packed, offs, shapes) takes a batch of pictures where jpeg.decode_batch (or
    source_batches) left them, plans every picture's tiles, feeds them to net.infer_dev in picture order in batches of the
    handle's max_batch (a picture's tiles may span batches), decodes every batch's result with ssd_decode_nms_dev(nms = 0) into
    the tile lists and merges them with ONE ssd_merge_tiles_dev; everything is enqueued on the net's stream and nothing waits for
    the GPU between the batches.  Two output sets alternate, as in the handle: a caller may launch the next pictures before it
    collects these.
    decode='all' (DESIGN.md 28): every class of an anchor is a candidate.  ssd_detout_tiles_add_dev follows every infer_dev and one
    ssd_detout_tiles_merge_dev ends the pass: the same ticket and output sets, out_cap = keep_top_k, the detections in global
    confidence order.  tile_cap and max_out belong to 'argmax': other values than their defaults raise.
    soft_nms = 'linear' | 'gaussian' (decode='all' only): the merge's NMS per class becomes Soft-NMS
    (ssd_detout_tiles_merge_soft_dev); soft_nms_min_score None = threshold."""

    def __init__(self, net, tile, overlap=0.25, whole=True, edge_margin=2, threshold=0.5, tile_cap=200, max_out=200, decode='argmax',
                 nms_top_k=400, keep_top_k=200, soft_nms=None, soft_nms_iou=0.45, soft_nms_sigma=0.5, soft_nms_min_score=None):
        from .ssdutils import check_tile_decode, soft_nms_params
        self.soft = soft_nms_params(soft_nms, soft_nms_iou, soft_nms_sigma, soft_nms_min_score, threshold)
        if self.soft is not None and decode != 'all':
            raise ValueError("soft_nms needs decode='all': the argmax decode keeps the hard rule")
        plan_tiles(tile, tile, tile, overlap, whole)         # (validates tile and overlap)
        self.decode = check_tile_decode(decode, tile_cap, max_out)
        self.nms_top_k, self.keep_top_k = int(nms_top_k), int(keep_top_k)
        self.net, self.tile, self.overlap, self.whole = net, int(tile), float(overlap), bool(whole)
        self.edge_margin, self.threshold = int(edge_margin), float(threshold)
        self.tile_cap = int(tile_cap)
        self.max_out = None if max_out is None else int(max_out)
        if self.tile_cap < 1:
            raise ValueError('merge_tiles: tile_cap must be >= 1 (got %d)' % self.tile_cap)
        self._serial = 0
        self._sets = [None, None]
        self._lists = None
        self._anchors = None
        self._det_ws = None
        self._all_ws = None
        self._last = None

    # ---- planning ---------------------------------------------------------------------------------------
    def plan(self, shapes):
        """[(image, Tile, (W, H))] for pictures of shapes [(h, w)], in picture order"""
        out = []
        for i, (h, w) in enumerate(shapes):
            out += [(i, t, (int(w), int(h))) for t in plan_tiles(w, h, self.tile, self.overlap, self.whole)]
        return out

    def plans(self, packed, offs, shapes, tiles=None):
        """the ImagePlan of every tile"""
        size = self.net.preset.image_size
        tiles = self.plan(shapes) if tiles is None else tiles
        return [tile_plan((packed, int(offs[i]), tuple(shapes[i])), t, size.w, size.h) for i, t, _ in tiles]

    def batches(self, packed, offs, shapes, tiles=None):
        """the tiles' network inputs, batch by batch: float32 CUDA tensors [b <= max_batch, H, W, 3]"""
        from . import transforms as T
        size = self.net.preset.image_size
        plans = self.plans(packed, offs, shapes, tiles)
        mb = self.net.max_batch
        for k in range(0, len(plans), mb):
            yield T.augment_batch(plans[k:k + mb], size.w, size.h, device=self.net.device)

    # ---- device state ---------------------------------------------------------------------------------------
    def _stream(self, device):
        import torch
        ptr = getattr(self.net, '_stream_ptr', 0)
        return ptr, (torch.cuda.ExternalStream(ptr, device=device) if ptr else torch.cuda.default_stream(device))

    def _ensure(self, n_tiles, n_images, out_cap, dev, ptr):
        import torch
        net, cap = self.net, self.tile_cap
        i32 = dict(dtype=torch.int32, device=dev)
        if self._anchors is None:
            self._anchors = torch.empty((net.preset.num_anchors, 4), dtype=torch.float64, device=dev)
            check(lib.ssd_anchors_dev(net.preset.name.encode(), self._anchors.data_ptr(), None, ptr or None))
        if self._det_ws is None and self.decode == 'argmax':
            self._det_ws = torch.empty(max(int(lib.ssd_decode_nms_ws_bytes(net.preset.name.encode(), net.max_batch)), 16), dtype=torch.uint8,
                                       device=dev)
        if self.decode == 'all':
            # the per-class lists of every tile and picture live in one workspace, written and read in stream order
            ws_bytes = int(lib.ssd_detout_tiles_ws_bytes(net.preset.name.encode(), net.num_vars - 5, n_tiles, n_images, self.nms_top_k))
            if ws_bytes == 0:
                raise RuntimeError(_lib.last_error())
            if self._all_ws is None or self._all_ws.numel() < ws_bytes:
                self._all_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            return self._out_set(n_images, out_cap, dev)
        # the tile lists are written and read in stream order: one set serves every launch
        if self._lists is None or self._lists['count'].shape[0] < n_tiles:
            self._lists = dict(count=torch.zeros(n_tiles, **i32), conf=torch.zeros((n_tiles, cap), dtype=torch.float32, device=dev),
                               cls=torch.zeros((n_tiles, cap), **i32), idx=torch.zeros((n_tiles, cap), **i32),
                               box=torch.zeros((n_tiles, cap, 4), **i32), ws=None)
        ws_bytes = int(lib.ssd_merge_tiles_ws_bytes(n_tiles, cap))
        if ws_bytes == 0:
            raise RuntimeError(_lib.last_error())
        if self._lists['ws'] is None or self._lists['ws'].numel() < ws_bytes:
            self._lists['ws'] = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        return self._out_set(n_images, out_cap, dev)

    def _out_set(self, n_images, out_cap, dev):
        import torch
        which = self._serial & 1
        s = self._sets[which]
        if s is None or s[0]['count'].shape[0] != n_images or s[0]['cls'].shape[1] != out_cap:
            shapes = dict(count=(n_images,), conf=(n_images, out_cap), cls=(n_images, out_cap), idx=(n_images, out_cap),
                          tile=(n_images, out_cap), box=(n_images, out_cap, 4))
            d = {k: torch.zeros(v, dtype=torch.float32 if k == 'conf' else torch.int32, device=dev) for k, v in shapes.items()}
            h = {k: torch.zeros(v, dtype=torch.float32 if k == 'conf' else torch.int32, pin_memory=True) for k, v in shapes.items()}
            s = self._sets[which] = (d, h)
        return s

    # ---- the pass ---------------------------------------------------------------------------------------
    def launch(self, packed, offs, shapes):
        """Enqueue the whole pass for the pictures (packed uint8 CUDA tensor, byte offsets, [(h, w)]); returns the ticket."""
        import torch
        net, cap = self.net, self.tile_cap
        tiles = self.plan(shapes)
        n_tiles, n_images = len(tiles), len(shapes)
        if n_images < 1:
            raise ValueError('merge_tiles: no pictures')
        per_image = max(sum(1 for t in tiles if t[0] == i) for i in range(n_images))
        mo = -1 if self.max_out is None else self.max_out
        out_cap = max(mo, 1) if mo >= 0 else per_image * cap
        if self.decode == 'all':
            out_cap = max(self.keep_top_k, 1)
        dev = packed.device
        ptr, stream = self._stream(dev)
        pname = net.preset.name.encode()
        nfg = net.num_vars - 5
        with torch.cuda.stream(stream):
            self._serial += 1
            d, h = self._ensure(n_tiles, n_images, out_cap, dev, ptr)
            L = self._lists
            result = C.c_void_p()
            k = 0
            structs = C.cast(tile_structs(tiles), C.c_void_p)
            for x in self.batches(packed, offs, shapes, tiles):
                b = x.shape[0]
                net.infer_dev(x)
                check(lib.ssd_result_dev(net._h, C.byref(result)))
                if self.decode == 'all':
                    # the handle's result buffer is reused by the next batch: its tiles are decoded now
                    check(lib.ssd_detout_tiles_add_dev(pname, nfg, self._anchors.data_ptr(), result.value, structs, n_tiles, k, b,
                                                       self.threshold, self.nms_top_k, self.edge_margin, self._all_ws.data_ptr(),
                                                       self._all_ws.numel(), ptr or None))
                    k += b
                    continue
                check(lib.ssd_decode_nms_dev(pname, nfg, self._anchors.data_ptr(), result.value, b, self.threshold, cap, -1, cap, 0,
                                             L['count'][k:].data_ptr(), L['conf'][k:].data_ptr(), L['cls'][k:].data_ptr(),
                                             L['idx'][k:].data_ptr(), L['box'][k:].data_ptr(), self._det_ws.data_ptr(), ptr or None))
                k += b
            if self.decode == 'all':
                args = (nfg, structs, n_tiles, n_images, self.nms_top_k, self.keep_top_k, out_cap, d['count'].data_ptr(),
                        d['conf'].data_ptr(), d['cls'].data_ptr(), d['idx'].data_ptr(), d['tile'].data_ptr(), d['box'].data_ptr(),
                        self._all_ws.data_ptr(), self._all_ws.numel())
                if self.soft is None:
                    check(lib.ssd_detout_tiles_merge_dev(*args, ptr or None))
                else:
                    check(lib.ssd_detout_tiles_merge_soft_dev(*args, C.cast(C.pointer(self.soft), C.c_void_p), ptr or None))
            else:
                check(lib.ssd_merge_tiles_dev(structs, n_tiles, n_images, cap, L['count'].data_ptr(),
                                              L['conf'].data_ptr(), L['cls'].data_ptr(), L['idx'].data_ptr(), L['box'].data_ptr(),
                                              self.edge_margin, mo, out_cap, d['count'].data_ptr(), d['conf'].data_ptr(), d['cls'].data_ptr(),
                                              d['idx'].data_ptr(), d['tile'].data_ptr(), d['box'].data_ptr(), L['ws'].data_ptr(), ptr or None))
            for key in d:
                h[key].copy_(d[key], non_blocking=True)
            done = torch.cuda.Event()
            done.record(stream)
        self._last = _TileDetections(self, self._serial, d, h, done, n_images, out_cap, tiles)
        return self._last

    def annotate_last_launch(self, src, src_offs, src_shapes, style, dst_shapes=None, rgb_out=False, keep_device=False, to_host=True):
        """SSDVGG.annotate_last_launch for the pass launch() has just enqueued: the merged detections drawn on the original-size
        pictures, right behind the merge on the same stream (what annotate.GpuJpegWriter.launch calls)."""
        import torch
        from . import annotate as A
        from .ssdvgg import _Annotated
        t = self._last
        if t is None or t.serial != self._serial:
            raise RuntimeError('annotate_last_launch needs a launch right before it')
        if not 1 <= len(src_shapes) <= t.b:
            raise ValueError('%d images for a detection pass of %d' % (len(src_shapes), t.b))
        ptr, stream = self._stream(src.device)
        with torch.cuda.stream(stream):
            dst, offs, shapes = A.annotate_batch(src, src_offs, src_shapes, t.count_dev, t.cls_dev, t.box_dev, t.out_cap, style,
                                                 dst_shapes=dst_shapes, rgb_out=rgb_out, stream=ptr or None)
            host = None
            if to_host:
                host = torch.empty(dst.shape, dtype=dst.dtype, pin_memory=True)
                host.copy_(dst, non_blocking=True)
            done = torch.cuda.Event()
            done.record(stream)
        return _Annotated(host, done, offs, shapes, dst if keep_device else None, stream if keep_device else None)

    def calibrate_fp8(self, packed, offs, shapes, images=32):
        """--dtype fp8 without stored scales: the first `images` tiles of these pictures calibrate the net"""
        seen = 0
        for x in self.batches(packed, offs, shapes):
            take = min(x.shape[0], max(int(images), 1) - seen)
            self.net.calibrate_fp8(x[:take], accumulate=seen > 0)
            seen += take
            if seen >= images:
                break
        return seen


def add_arguments(parser):
    """the drivers' --tile flags"""
    from .utils import str2bool
    parser.add_argument('--tile', type=int, default=0, metavar='N',
                        help='detect in overlapping N x N windows of the source picture and merge their boxes on the GPU (0 = off: the '
                             'picture is shrunk to the network size in one piece)')
    parser.add_argument('--tile-overlap', type=float, default=0.25, help='--tile: overlap of neighbouring windows, 0 .. 0.9 of N')
    parser.add_argument('--tile-whole', type=str2bool, default='True', help='--tile: also detect on the whole shrunk picture (keeps the large objects)')
    parser.add_argument('--tile-edge-margin', type=int, default=2,
                        help='--tile: drop a box within this many thousandths of an interior window edge (the window cut it); -1 keeps all')
    parser.add_argument('--tile-decode', default='argmax', choices=['argmax', 'all'],
                        help="--tile: the decode of the windows (--decode names the untiled pass's decode and does not apply to --tile). "
                             "argmax: one candidate per anchor of a window; all: the SSD paper's DetectionOutput across the windows, every class "
                             'of an anchor above the threshold is a candidate, per class the best --nms-top-k of the picture go through one NMS '
                             'over all windows and the best --keep-top-k of the picture are kept, in confidence order (DESIGN.md 28)')


def check_arguments(parser, args):
    """--tile-decode all needs --tile and --nms-top-k / --keep-top-k in range"""
    if args.tile_decode == 'all':
        if not args.tile:
            parser.error('--tile-decode all needs --tile N (the untiled pass takes --decode all)')
        for name in ('nms_top_k', 'keep_top_k'):
            if not 1 <= getattr(args, name) <= 1024:
                parser.error('--%s must be in 1..1024' % name.replace('_', '-'))


def decode_keywords(args):
    """the decode keywords of TiledDetector for these arguments"""
    if args.tile_decode == 'all':
        from .infer import soft_nms_keywords
        return dict(decode='all', nms_top_k=args.nms_top_k, keep_top_k=args.keep_top_k, **soft_nms_keywords(args))
    return {}


def source_batches(files, batch_size, device=0, decoder='pillow', decoder_entropy='host'):
    """The drivers' pictures for TiledDetector.launch, batch by batch: (packed uint8 CUDA tensor, byte offsets, [(h, w)], indices).
    Baseline JPEGs are decoded on the GPU with decoder='gpu' (jpeg.decode_batch); anything else is loaded on the host and
    uploaded.  Tiling reads source pixels: float arrays (network-size inputs) are refused."""
    import torch
    from . import transforms as T
    from .annotate import pack_offsets
    from .infer import _has_jpeg_candidates
    for offset in range(0, len(files), batch_size):
        chunk = files[offset:offset + batch_size]
        idxs = list(range(offset, offset + len(chunk)))
        if decoder == 'gpu' and _has_jpeg_candidates(chunk):
            from . import jpeg
            packed, offs, shapes, _ = jpeg.decode_batch(chunk, device=device, entropy=decoder_entropy)
            yield packed, list(offs), [tuple(s) for s in shapes], idxs
            continue
        images = [f if isinstance(f, np.ndarray) else T.load_image_bgr(f) for f in chunk]
        for f, img in zip(chunk, images):
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                raise ValueError('%s: --tile needs uint8 [H, W, 3] pictures, got %s %s' % (f if isinstance(f, str) else 'array', img.dtype, img.shape))
        shapes = [(img.shape[0], img.shape[1]) for img in images]
        offs, total = pack_offsets(shapes, 1)
        host = np.zeros(max(total, 16), np.uint8)
        for o, img in zip(offs, images):
            host[o:o + img.size] = img.reshape(-1)
        yield torch.from_numpy(host).to(torch.device('cuda', device)), offs, shapes, idxs


def fp8_ready(detector, sources, calibration_file=None, calibrate_images=32):
    """fp8_batches for the tiled loop: an fp8 net has its scales before the first launch -- from calibration_file if it exists,
    else from the first tiles of `sources` (written to calibration_file if given).  Nothing to do for any other dtype."""
    net = detector.net
    if getattr(net, 'dtype', None) != 'fp8':
        return
    if calibration_file and os.path.exists(calibration_file):
        with np.load(calibration_file, allow_pickle=False) as f:
            net.fp8_scales = {k: float(f[k]) for k in f.files}
        print('[i] fp8 scales:         loaded from', calibration_file)
        return
    seen = detector.calibrate_fp8(*sources, images=calibrate_images)
    print('[i] fp8 scales:         calibrated on the first', seen, 'tiles')
    if calibration_file:
        with open(calibration_file, 'wb') as f:
            np.savez(f, **net.fp8_scales)
