"""cv2.imread for baseline JPEGs without the CPU decode (csrc/jpeg.hip): the library parses the file and decodes
its Huffman stream on host threads; dequantisation, the inverse DCT, chroma upsampling and YCbCr -> BGR run on the GPU and leave
packed [h][w][3] uint8 BGR pixels where `transforms.augment_batch` and `annotate` read them.  The pixels equal libjpeg-turbo's
default decode (what cv2.imread and Pillow produce) byte for byte.

A file outside the supported class (progressive, CMYK, unusual sampling, ...: status UNSUPPORTED), a non-JPEG file or a .npy array
is loaded by `transforms.load_image_bgr` and copied into the same packed buffer.  A corrupt JPEG raises JpegError.
"""
import ctypes as C
import os

import numpy as np

from ._lib import lib, last_error

OK, UNSUPPORTED, ERROR = 0, 1, 2
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


def decode_batch(files_or_bytes, device=0, threads=None, stream=None):
    """Decode a batch onto the GPU: (packed uint8 device tensor, byte offsets, [(h, w)], fallbacks).  Image i lies at
    offsets[i] (a multiple of 16; ascending unless there are fallbacks, which lie behind the decoded images) as [h][w][3] BGR;
    the bytes between images hold nothing.  One pinned staging buffer, one
    host-to-device copy, two kernel launches, all on `stream` (default: torch's current stream of `device`).  `fallbacks`: indices
    of the items the library did not decode (unsupported JPEGs, other formats, arrays): loaded as load_image_bgr does and copied in."""
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

    gpu, descs = [], None
    if cand:
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


def decode(file_or_bytes, device=0):
    """One image as a uint8 [h, w, 3] BGR numpy array (through the GPU)."""
    dst, offs, sizes, _ = decode_batch([file_or_bytes], device=device, threads=1)
    h, w = sizes[0]
    return dst[offs[0]:offs[0] + h * w * 3].cpu().numpy().reshape(h, w, 3)
