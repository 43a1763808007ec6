"""cv2.imread for baseline JPEGs without the CPU decode (csrc/jpeg.hip): the library parses the file and decodes
its Huffman stream on host threads; dequantisation, the inverse DCT, chroma upsampling and YCbCr -> BGR run on the GPU and leave
packed [h][w][3] uint8 BGR pixels where `transforms.augment_batch` and `annotate` read them.  The pixels equal libjpeg-turbo's
default decode (what cv2.imread and Pillow produce) byte for byte.  With decode_batch(entropy='gpu') the Huffman streams are
decoded on the GPU as well (csrc/jpeg_huffdec.hip): the host parses the markers and copies the files' own bytes.

`encode_batch` is the way back, cv2.imwrite(<name>.jpg) without the CPU front half (csrc/jpeg_enc.hip): colour
conversion, chroma downsampling, the forward DCT and quantisation run on the GPU on the same packed layout, Huffman coding and the
file framing on host threads of the library; the files equal the ones libjpeg-turbo (cv2.imwrite, Pillow) writes byte for byte.
With entropy='gpu' Huffman coding and the framing run on the GPU as well (csrc/jpeg_huff.hip) and only the files'
own bytes come to the host; the bytes are the same.

A file outside the supported class (progressive, CMYK, unusual sampling, ...: status UNSUPPORTED), a non-JPEG file or a .npy array
is loaded by `transforms.load_image_bgr` and copied into the same packed buffer.  A corrupt JPEG raises JpegError.
"""
import ctypes as C
import os

import numpy as np

from ._lib import lib, last_error

OK, UNSUPPORTED, ERROR, TO_HOST = 0, 1, 2, 3       # TO_HOST (SSD_JPEG_TO_HOST) never leaves decode_batch
MAX_L1 = 15000                   # SSD_JPEG_MAX_L1


class JpegError(RuntimeError):
    pass


class Desc(C.Structure):
    """ssd_jpeg_desc (include/ssdvgg_hip.h)"""
    _fields_ = [('width', C.c_int), ('height', C.c_int), ('components', C.c_int), ('hs', C.c_int), ('vs', C.c_int),
                ('mcus_x', C.c_int), ('mcus_y', C.c_int), ('max_l1', C.c_int),
                ('coef_off', C.c_ulonglong * 3), ('dst_off', C.c_ulonglong), ('qt', (C.c_ushort * 64) * 3)]


def _buf(data):
    """(keep-alive object, address, length) of a bytes-like or uint8 array without copying"""
    a = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8).reshape(-1)
    return a, a.ctypes.data, a.size


def info(data):
    """(width, height, components, luma sampling hs * 16 + vs, status) from the header alone; JpegError for a corrupt header"""
    a, ptr, n = _buf(data)
    w, h, c, s, st = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    if lib.ssd_jpeg_info(ptr, n, w, h, c, s, st) != 0:
        raise JpegError(last_error())
    return w.value, h.value, c.value, s.value, st.value


def entropy_decode(data):
    """Host only: (status, Desc, int16 coefficient array) of one file; the array is None unless the status is OK or the file
    was refused by the 32-bit range guard.  JpegError for corrupt input."""
    a, ptr, n = _buf(data)
    nbytes = lib.ssd_jpeg_coef_bytes(ptr, n)
    coef = np.zeros(max(nbytes // 2, 8), np.int16)
    d, st = Desc(), C.c_int()
    if lib.ssd_jpeg_entropy_decode(ptr, n, coef.ctypes.data, nbytes, C.byref(d), st) != 0:
        raise JpegError(last_error())
    return st.value, d, (coef if nbytes else None)


def entropy_decode_batch(datas, threads=None, coef=None):
    """Host only: (int16 coefficient array, byte offsets [n + 1], Desc array, statuses, error text) of a list of bytes-likes, on up
    to `threads` host threads (default min(8, n); never derived from the machine's core count).  coef: a function
    nbytes -> writable int16 numpy array to decode into (pinned memory), default numpy's own."""
    n = len(datas)
    threads = min(8, max(n, 1)) if threads is None else int(threads)
    keep = [_buf(d) for d in datas]
    ptrs = (C.c_void_p * n)(*[k[1] for k in keep])
    sizes = (C.c_size_t * n)(*[k[2] for k in keep])
    offsets = (C.c_ulonglong * (n + 1))()
    for i in range(n):
        offsets[i + 1] = offsets[i] + lib.ssd_jpeg_coef_bytes(ptrs[i], sizes[i])
    total = int(offsets[n])
    buf = (coef or (lambda nbytes: np.empty(nbytes // 2, np.int16)))(max(total, 16))
    descs = (Desc * n)()
    status = (C.c_int * n)()
    if lib.ssd_jpeg_entropy_decode_batch(ptrs, sizes, n, threads, buf.ctypes.data, offsets, descs, status) != 0:
        raise RuntimeError(last_error())
    st = list(status)
    return buf, list(offsets), descs, st, (last_error() if ERROR in st else '')


class HuffTable(C.Structure):
    """ssd_jpeg_huff_table (include/ssdvgg_hip.h)"""
    _fields_ = [('fast_len', C.c_ubyte * 512), ('fast_val', C.c_ubyte * 512), ('maxcode', C.c_int * 17), ('mincode', C.c_int * 17),
                ('valptr', C.c_int * 17), ('vals', C.c_ubyte * 256)]


class Segment(C.Structure):
    """ssd_jpeg_segment"""
    _fields_ = [('begin', C.c_uint), ('end', C.c_uint)]


class Plan(C.Structure):
    """ssd_jpeg_plan"""
    _fields_ = [('file_off', C.c_ulonglong), ('file_bytes', C.c_ulonglong), ('scan_pos', C.c_ulonglong), ('restart_interval', C.c_int),
                ('segments', C.c_int), ('seg', C.POINTER(Segment)), ('seg_cap', C.c_int), ('dc_sel', C.c_int * 3), ('ac_sel', C.c_int * 3),
                ('dc', HuffTable * 2), ('ac', HuffTable * 2)]


class HuffdecRec(C.Structure):
    """ssd_jpeg_huffdec_rec"""
    _fields_ = [('status', C.c_int), ('max_l1', C.c_int)]


def scan_plan(data, plan=None):
    """Host only, no bit decoded: (status, Desc, Plan) of one file; the Plan (segment ranges in plan.seg[0 .. plan.segments), the
    selected Huffman tables) is usable when the status is OK.  TO_HOST: entropy_decode decides.  JpegError for a corrupt header.
    plan: a Plan to fill (an element of a Plan array), default a new one."""
    a, ptr, n = _buf(data)
    cap = lib.ssd_jpeg_scan_segments(ptr, n)
    segs = (Segment * max(cap, 1))()
    plan = Plan() if plan is None else plan
    plan.seg, plan.seg_cap = segs, max(cap, 1)
    plan._segs = segs                                            # (keeps the array alive with the plan)
    d, st = Desc(), C.c_int()
    if lib.ssd_jpeg_scan_plan(ptr, n, C.byref(d), C.byref(plan), st) != 0:
        raise JpegError(last_error())
    return st.value, d, plan


def _read(item):
    """bytes of a file that may be a JPEG, else None (arrays, .npy files, files with a .npy beside them: load_image_bgr's rules)"""
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    if isinstance(item, np.ndarray) or item.endswith('.npy') or os.path.exists(item + '.npy'):
        return None
    with open(item, 'rb') as f:
        return f.read()


def _fallback(item, data):
    from . import transforms as T
    if isinstance(item, np.ndarray):
        img = item
    elif isinstance(item, str):
        img = T.load_image_bgr(item)
    else:
        import io
        from PIL import Image
        with Image.open(io.BytesIO(data)) as im:
            img = np.asarray(im.convert('RGB'))[:, :, ::-1]
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError('decode_batch packs uint8 [H, W, 3] BGR images, got %s %s' % (img.dtype, img.shape))
    return img


def _huffdec_gpu(datas, dev, max_rounds):
    """The Huffman stage of decode_batch(entropy='gpu') for a list of bytes: plans on the calling thread, one pinned copy of the
    files' bytes, the launches, one copy of the records, one wait.  Returns (device int16 coefficient tensor or None, Desc array,
    statuses, messages): status OK with the descriptor complete (coef_off inside the tensor, max_l1), UNSUPPORTED, or ERROR with
    the host stage's message; files the device stage hands over have been through entropy_decode and uploaded."""
    import torch
    n = len(datas)
    descs, plans, keep = (Desc * n)(), (Plan * n)(), []
    status, msgs = [ERROR] * n, [''] * n
    for k, data in enumerate(datas):
        try:
            status[k], d, plan = scan_plan(data, plans[k])
            keep.append(plan._segs)                              # (the segment arrays live until the launches have copied them)
            C.memmove(C.byref(descs[k]), C.byref(d), C.sizeof(Desc))
        except JpegError as e:
            msgs[k] = str(e)
    run = [k for k in range(n) if status[k] == OK]
    host = [k for k in range(n) if status[k] == TO_HOST]
    coef_off, total = {}, 0
    for k in run + host:
        coef_off[k] = total
        total += lib.ssd_jpeg_coef_bytes(*_buf(datas[k])[1:])
    if not total:
        return None, descs, status, msgs
    s = torch.cuda.current_stream(dev)
    coef_dev = torch.empty((total // 2,), dtype=torch.int16, device=dev)
    if run:
        file_off, fbytes = [], 0
        for k in run:
            file_off.append(fbytes)
            fbytes += (len(datas[k]) + 15) // 16 * 16
        stage = torch.empty((fbytes,), dtype=torch.uint8, pin_memory=True)
        view = stage.numpy()
        rp, rd = (Plan * len(run))(), (Desc * len(run))()
        for j, k in enumerate(run):
            view[file_off[j]:file_off[j] + len(datas[k])] = np.frombuffer(datas[k], np.uint8)
            C.memmove(C.byref(rp[j]), C.byref(plans[k]), C.sizeof(Plan))
            C.memmove(C.byref(rd[j]), C.byref(descs[k]), C.sizeof(Desc))
            rp[j].file_off = file_off[j]
            for c in range(3):
                rd[j].coef_off[c] += coef_off[k] // 2
        files_dev = stage.to(dev, non_blocking=True)
        ws_bytes = lib.ssd_jpeg_huffdec_ws_bytes(rp, rd, len(run))
        if ws_bytes == 0:
            raise RuntimeError(last_error())
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        recs_dev = torch.empty((len(run) * C.sizeof(HuffdecRec),), dtype=torch.uint8, device=dev)
        if lib.ssd_jpeg_huffdec_batch_dev(files_dev.data_ptr(), files_dev.numel(), rp, rd, len(run), coef_dev.data_ptr(), total,
                                          recs_dev.data_ptr(), ws.data_ptr(), ws_bytes, int(max_rounds), s.cuda_stream) != 0:
            raise RuntimeError(last_error())
        recs_host = torch.empty((len(run) * C.sizeof(HuffdecRec),), dtype=torch.uint8, pin_memory=True)
        recs_host.copy_(recs_dev, non_blocking=True)
        s.synchronize()                                          # the one wait
        recs = (HuffdecRec * len(run)).from_buffer_copy(recs_host.numpy().tobytes())
        for j, k in enumerate(run):
            if recs[j].status == OK:
                C.memmove(C.byref(descs[k]), C.byref(rd[j]), C.sizeof(Desc))
                descs[k].max_l1 = recs[j].max_l1
                if recs[j].max_l1 > MAX_L1:
                    status[k] = UNSUPPORTED                      # the range guard: the caller's fallback decodes it
            else:
                status[k] = TO_HOST
                host.append(k)
    for k in sorted(host):                                       # the host stage decides: status, message, coefficients
        try:
            status[k], d, coef = entropy_decode(datas[k])
        except JpegError as e:
            status[k], msgs[k] = ERROR, str(e)
            continue
        if status[k] == OK:
            C.memmove(C.byref(descs[k]), C.byref(d), C.sizeof(Desc))
            for c in range(3):
                descs[k].coef_off[c] += coef_off[k] // 2
            nel = lib.ssd_jpeg_coef_bytes(*_buf(datas[k])[1:]) // 2
            up = torch.empty((nel,), dtype=torch.int16, pin_memory=True)
            up.numpy()[:] = coef[:nel]
            coef_dev[coef_off[k] // 2:coef_off[k] // 2 + nel].copy_(up, non_blocking=True)
    return coef_dev, descs, status, msgs


def decode_batch(files_or_bytes, device=0, threads=None, stream=None, entropy='host', _max_rounds=0):
    """Decode a batch onto the GPU: (packed uint8 device tensor, byte offsets, [(h, w)], fallbacks).  Image i lies at
    offsets[i] (a multiple of 16; ascending unless there are fallbacks, which lie behind the decoded images) as [h][w][3] BGR;
    the bytes between images hold nothing.  One pinned staging buffer, one
    host-to-device copy, two kernel launches, all on `stream` (default: torch's current stream of `device`).  `fallbacks`: indices
    of the items the library did not decode (unsupported JPEGs, other formats, arrays): loaded as load_image_bgr does and copied in.
    entropy='gpu': the Huffman stage runs on the GPU too (csrc/jpeg_huffdec.hip): the files' own bytes are copied
    instead of the coefficients, and the call waits once for one small record per file; a file whose decode the device stage
    cannot certify goes through the host stage.  The same return value and the same exceptions; `threads` is not used."""
    if entropy not in ENTROPY:
        raise ValueError("entropy must be 'host' or 'gpu' (got %r)" % (entropy,))
    import torch
    items = list(files_or_bytes)
    n = len(items)
    dev = torch.device('cuda', device)
    datas = [_read(it) for it in items]
    cand = [i for i in range(n) if datas[i] is not None and datas[i][:2] == b'\xff\xd8']
    pinned = []

    def alloc(nbytes):
        t = torch.empty((nbytes // 2,), dtype=torch.int16, pin_memory=True)
        pinned.append(t)
        return t.numpy()

    gpu, descs, coef_dev = [], None, None
    if cand and entropy == 'gpu':
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            coef_dev, descs, status, msgs = _huffdec_gpu([datas[i] for i in cand], dev, _max_rounds)
        for k, i in enumerate(cand):                             # (the host path names the first bad file of the list, as "file k")
            if status[k] == ERROR:
                raise JpegError('%s: file %d: %s' % (items[i] if isinstance(items[i], str) else 'item %d' % i, k, msgs[k]))
        gpu = [(k, i) for k, i in enumerate(cand) if status[k] == OK]
    elif cand:
        coef, coef_offs, descs, status, err = entropy_decode_batch([datas[i] for i in cand], threads, alloc)
        for k, i in enumerate(cand):
            if status[k] == ERROR:
                raise JpegError('%s: %s' % (items[i] if isinstance(items[i], str) else 'item %d' % i, err))
        gpu = [(k, i) for k, i in enumerate(cand) if status[k] == OK]
    on_gpu = {i for _, i in gpu}
    fallbacks = [i for i in range(n) if i not in on_gpu]
    loaded = {i: _fallback(items[i], datas[i]) for i in fallbacks}
    sizes, offsets, off = [None] * n, [0] * n, 0
    for k, i in gpu:
        sizes[i] = (descs[k].height, descs[k].width)
    for i in fallbacks:
        sizes[i] = loaded[i].shape[:2]
    for i in sorted(on_gpu) + fallbacks:            # the fallbacks lie behind the decoded images, in one run: one copy
        offsets[i] = off
        off += (sizes[i][0] * sizes[i][1] * 3 + 15) // 16 * 16
    tail = offsets[fallbacks[0]] if fallbacks else off
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        s = torch.cuda.current_stream(dev).cuda_stream
        dst = torch.empty((max(off, 16),), dtype=torch.uint8, device=dev)
        if fallbacks:
            stage = torch.empty((off - tail,), dtype=torch.uint8, pin_memory=True)
            host = stage.numpy()
            for i in fallbacks:
                host[offsets[i] - tail:offsets[i] - tail + loaded[i].size] = loaded[i].reshape(-1)
            dst[tail:].copy_(stage, non_blocking=True)
        if gpu:
            run = (Desc * len(gpu))()
            for j, (k, i) in enumerate(gpu):
                C.memmove(C.byref(run[j]), C.byref(descs[k]), C.sizeof(Desc))
                run[j].dst_off = offsets[i]
            if coef_dev is None:
                coef_dev = pinned[0].to(dev, non_blocking=True)
            ws_bytes = lib.ssd_jpeg_ws_bytes(run, len(gpu))
            if ws_bytes == 0:
                raise RuntimeError(last_error())
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
            if lib.ssd_jpeg_decode_batch_dev(coef_dev.data_ptr(), coef_dev.numel() * 2, run, len(gpu), dst.data_ptr(), dst.numel(),
                                             ws.data_ptr(), ws_bytes, s) != 0:
                raise RuntimeError(last_error())
            # coef_dev and ws are released in stream order by torch's allocator; the descriptors were copied by the call
    return dst, offsets, sizes, fallbacks


def decode(file_or_bytes, device=0, entropy='host'):
    """One image as a uint8 [h, w, 3] BGR numpy array (through the GPU)."""
    dst, offs, sizes, _ = decode_batch([file_or_bytes], device=device, threads=1, entropy=entropy)
    h, w = sizes[0]
    return dst[offs[0]:offs[0] + h * w * 3].cpu().numpy().reshape(h, w, 3)


# ------------------------------------------------------------------------------------------------ encoding
SAMPLING = {'4:4:4': 0x11, '4:2:2': 0x21, '4:2:0': 0x22}


def quant_tables(quality):
    """(luma, chroma) uint16 [64] quantisation tables of a libjpeg quality 1..100, natural order"""
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    if lib.ssd_jpeg_quant_tables(int(quality), luma.ctypes.data, chroma.ctypes.data) != 0:
        raise JpegError(last_error())
    return luma, chroma


def entropy_encode(coef, desc):
    """Host only: the JFIF file (bytes) of one image's int16 coefficients and Desc (coef_off relative to `coef`)."""
    coef = np.ascontiguousarray(coef, np.int16)
    cap = lib.ssd_jpeg_file_bound(C.byref(desc))
    if cap == 0:
        raise JpegError(last_error())
    out, size = np.empty(cap, np.uint8), C.c_size_t()
    if lib.ssd_jpeg_entropy_encode(coef.ctypes.data, coef.nbytes, C.byref(desc), out.ctypes.data, cap, C.byref(size)) != 0:
        raise JpegError(last_error())
    return out[:size.value].tobytes()


def entropy_encode_batch(coef, descs, threads=None):
    """Host only: the JFIF files (list of bytes) of n images on up to `threads` host threads (default min(8, n); never derived from
    the machine's core count).  coef: int16 numpy array; descs: Desc array with coef_off relative to `coef`."""
    n = len(descs)
    threads = min(8, max(n, 1)) if threads is None else int(threads)
    offsets = (C.c_ulonglong * (n + 1))()
    for i in range(n):
        cap = lib.ssd_jpeg_file_bound(C.byref(descs[i]))
        if cap == 0:
            raise JpegError('image %d: %s' % (i, last_error()))
        offsets[i + 1] = offsets[i] + cap
    out = np.empty(max(int(offsets[n]), 16), np.uint8)               # (an upper bound: the pages behind a file are never touched)
    sizes = (C.c_ulonglong * n)()
    if lib.ssd_jpeg_entropy_encode_batch(coef.ctypes.data, coef.nbytes, descs, n, threads, out.ctypes.data, out.size, offsets, sizes) != 0:
        raise JpegError(last_error())
    return [out[offsets[i]:offsets[i] + sizes[i]].tobytes() for i in range(n)]


class FileRec(C.Structure):
    """ssd_jpeg_file_rec (include/ssdvgg_hip.h)"""
    _fields_ = [('offset', C.c_ulonglong), ('size', C.c_ulonglong), ('status', C.c_int), ('reserved', C.c_int)]


ENTROPY = ('host', 'gpu')
HUFF_REFUSALS = {1: 'jpeg: a DC difference needs more than 11 bits, baseline Huffman codes 11',
                 2: 'jpeg: an AC coefficient needs more than 10 bits, baseline Huffman codes 10'}
_copy_streams = {}


def file_header(desc):
    """Host only: the 623 bytes in front of the scan (SOI ... SOS) of the file of this Desc"""
    out = np.empty(623, np.uint8)
    if lib.ssd_jpeg_file_header(C.byref(desc), out.ctypes.data) != 0:
        raise JpegError(last_error())
    return out.tobytes()


class _Encoding:
    """Ticket of encode_launch: the device stage and the copy of its coefficients are in flight."""
    def __init__(self, host, descs, done, threads, keep):
        self.host, self.descs, self.done, self.threads, self._keep = host, descs, done, threads, keep

    def get(self):
        """list of bytes, one JFIF file per image (waits for the copy, then runs the host stage)"""
        self.done.synchronize()
        self._keep = None
        return entropy_encode_batch(self.host.numpy(), self.descs, self.threads)


class _DeviceEncoding:
    """Ticket of encode_launch(entropy='gpu'): both device stages and the copy of the file records are in flight."""
    def __init__(self, recs, out, done, keep):
        self.recs, self.out, self.done, self._keep = recs, out, done, keep

    def get(self):
        """list of bytes, one JFIF file per image: waits for the records, then copies exactly the files' bytes, on a stream of
        its own (the caller's stream may hold the next batch's kernels by now)"""
        import torch
        self.done.synchronize()
        n = self.recs.numel() // C.sizeof(FileRec)
        recs = (FileRec * n).from_buffer_copy(self.recs.numpy().tobytes())
        for i in range(n):
            if recs[i].status != 0:
                self._keep = self.out = None
                raise JpegError('image %d: %s' % (i, HUFF_REFUSALS.get(recs[i].status, 'jpeg: status %d' % recs[i].status)))
        total = int(recs[n - 1].offset + recs[n - 1].size)
        dev = self.out.device
        if dev.index not in _copy_streams:
            _copy_streams[dev.index] = torch.cuda.Stream(dev)
        side = _copy_streams[dev.index]
        host = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
        with torch.cuda.stream(side):
            host.copy_(self.out[:total], non_blocking=True)
        side.synchronize()
        self._keep = self.out = None
        data = host.numpy()
        return [data[r.offset:r.offset + r.size].tobytes() for r in recs]


def encode_launch(src, offs=None, shapes=None, quality=95, subsampling='4:2:0', threads=None, stream=None, device=0, entropy='host'):
    """Enqueue the device stage of encode_batch and the device-to-host copy of the coefficients (into pinned memory) on `stream`
    (a torch stream; default the current one); returns a ticket whose get() runs the host stage.  entropy='gpu': the Huffman
    stage is enqueued behind the device stage, with a copy of the n file records; get() fetches the files' bytes (`threads` is
    not used)."""
    import torch
    if subsampling not in SAMPLING:
        raise ValueError('subsampling must be one of 4:4:4, 4:2:2, 4:2:0 (got %r)' % (subsampling,))
    if entropy not in ENTROPY:
        raise ValueError("entropy must be 'host' or 'gpu' (got %r)" % (entropy,))
    if not hasattr(src, 'data_ptr'):                                  # host arrays: packed at 16-byte aligned offsets and uploaded
        imgs = [np.ascontiguousarray(a) for a in src]
        for a in imgs:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError('encode_batch takes uint8 [H, W, 3] BGR images, got %s %s' % (a.dtype, a.shape))
        shapes, offs, total = [a.shape[:2] for a in imgs], [], 0
        for a in imgs:
            offs.append(total)
            total += (a.size + 15) // 16 * 16
        stage = torch.empty((max(total, 16),), dtype=torch.uint8, pin_memory=True)
        host = stage.numpy()
        for a, o in zip(imgs, offs):
            host[o:o + a.size] = a.reshape(-1)
        dev = torch.device('cuda', device)
    else:
        if src.dtype != torch.uint8 or not src.is_contiguous():
            raise ValueError('encode_batch takes a contiguous uint8 device tensor, got %s' % (src.dtype,))
        stage, dev = None, src.device
    n = len(shapes)
    if n < 1 or len(offs) != n:
        raise ValueError('one offset per image and at least one image')
    threads = min(8, n) if threads is None else int(threads)
    shp = (C.c_int * (2 * n))(*[int(v) for hw in shapes for v in hw[:2]])
    src_offs = (C.c_ulonglong * n)(*[int(o) for o in offs])
    sampling = SAMPLING[subsampling]
    coef_bytes, ws_bytes = lib.ssd_jpeg_enc_coef_bytes(shp, n, sampling), lib.ssd_jpeg_enc_ws_bytes(shp, n, sampling)
    if coef_bytes == 0 or ws_bytes == 0:
        raise JpegError(last_error())
    descs = (Desc * n)()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        cur = torch.cuda.current_stream(dev)
        if stage is not None:
            src = stage.to(dev, non_blocking=True)
        coef_dev = torch.empty((coef_bytes // 2,), dtype=torch.int16, device=dev)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        if lib.ssd_jpeg_encode_batch_dev(src.data_ptr(), src.numel(), src_offs, shp, n, int(quality), sampling, coef_dev.data_ptr(),
                                         coef_bytes, descs, ws.data_ptr(), ws_bytes, cur.cuda_stream) != 0:
            raise JpegError(last_error())
        if entropy == 'gpu':
            huff_ws_bytes, out_bytes = lib.ssd_jpeg_huff_ws_bytes(descs, n), lib.ssd_jpeg_huff_out_bytes(descs, n)
            if huff_ws_bytes == 0 or out_bytes == 0:
                raise JpegError(last_error())
            huff_ws = torch.empty((huff_ws_bytes,), dtype=torch.uint8, device=dev)
            out = torch.empty((out_bytes,), dtype=torch.uint8, device=dev)
            recs_dev = torch.empty((n * C.sizeof(FileRec),), dtype=torch.uint8, device=dev)
            if lib.ssd_jpeg_huffman_batch_dev(coef_dev.data_ptr(), coef_bytes, descs, n, out.data_ptr(), out_bytes, recs_dev.data_ptr(),
                                              huff_ws.data_ptr(), huff_ws_bytes, cur.cuda_stream) != 0:
                raise JpegError(last_error())
            recs = torch.empty((n * C.sizeof(FileRec),), dtype=torch.uint8, pin_memory=True)
            recs.copy_(recs_dev, non_blocking=True)
            done = torch.cuda.Event()
            done.record(cur)
            return _DeviceEncoding(recs, out, done, (src, coef_dev, ws, stage, huff_ws, recs_dev))
        host = torch.empty((coef_bytes // 2,), dtype=torch.int16, pin_memory=True)
        host.copy_(coef_dev, non_blocking=True)
        done = torch.cuda.Event()
        done.record(cur)
    # (src, coef_dev and ws stay referenced until the copy has finished: another stream's allocations cannot take them before)
    return _Encoding(host, descs, done, threads, (src, coef_dev, ws, stage))


def encode_batch(src, offs=None, shapes=None, quality=95, subsampling='4:2:0', threads=None, stream=None, device=0, entropy='host'):
    """cv2.imwrite's JPEG bytes of a batch: list of bytes, one JFIF file per image.  src: a uint8 device tensor that holds image i as
    [h][w][3] BGR at byte offset offs[i] (shapes[i] = (h, w); the layout annotate_batch and decode_batch write), or a list of
    uint8 [h, w, 3] BGR host arrays, which are uploaded.  Device stage (one launch), one device-to-host copy of the int16
    coefficients into pinned memory, then the host stage on up to `threads` threads (default min(8, n)).  quality 95 and 4:2:0
    are cv2.imwrite's defaults.  entropy='gpu': Huffman coding and the framing on the GPU too (seven more launches), then one copy
    of the n file records and one of the files' own bytes; the same files."""
    return encode_launch(src, offs, shapes, quality, subsampling, threads, stream, device, entropy).get()


def encode(image, quality=95, subsampling='4:2:0', device=0, entropy='host'):
    """One uint8 [h, w, 3] BGR picture as the bytes of a JFIF file (through the GPU)."""
    return encode_batch([image], quality=quality, subsampling=subsampling, threads=1, device=device, entropy=entropy)[0]
