"""Drawing detections through the HIP library (include/ssdvgg_hip.h "drawing detections"): the counterpart of the
reference's utils.draw_box (utils.py:138-148) and of what its callers do with it.  The pixels and the boxes stay on the GPU:
`annotate_batch` takes a packed device buffer of images and detection arrays laid out like ssd_detect_last_dev's.  There is no
CPU fallback; the only host-side code here is packing arguments and encoding the finished image files."""
import ctypes as C
import os
import struct
import zlib

import numpy as np

from ._lib import lib, check, np_ptr

MAX_LABEL = 31


class _Image(C.Structure):
    """ssd_annotate_image (include/ssdvgg_hip.h)"""
    _fields_ = [('src_off', C.c_ulonglong), ('src_w', C.c_int), ('src_h', C.c_int),
                ('dst_off', C.c_ulonglong), ('dst_w', C.c_int), ('dst_h', C.c_int)]


def glyph(ch):
    """The 7 rows of a character of the built-in 5 x 7 font (5 bits per row, column 0 = bit 4)."""
    rows = (C.c_ubyte * 7)()
    check(lib.ssd_annotate_glyph(int(ch), rows))
    return list(rows)


def rect_on_image(box1000, w, h):
    """(xmin, xmax, ymin, ymax) in pixels of a w x h image for an integer box on the 1000 grid."""
    src = (C.c_int * 4)(*[int(v) for v in box1000]); out = (C.c_int * 4)()
    check(lib.ssd_annotate_rect(src, int(w), int(h), out))
    return tuple(out)


def pack_names(names):
    """[num_classes][32] NUL-terminated bytes; a name is cut at 31 characters, non-ASCII characters are drawn as '?'."""
    out = np.zeros((len(names), 32), np.uint8)
    for i, n in enumerate(names):
        raw = str(n).encode('ascii', 'replace')[:MAX_LABEL].replace(b'\0', b'?')
        out[i, :len(raw)] = np.frombuffer(raw, np.uint8)
    return out


class Style:
    """Class colours (BGR) and names on one GPU, uploaded once (ssd_annotate_style_create)."""

    def __init__(self, colors_bgr, names, device=0):
        colors = np.ascontiguousarray(np.asarray(colors_bgr).reshape(-1, 3), np.uint8)
        if len(colors) != len(names):
            raise ValueError('one colour per class name')
        self.names = [str(n) for n in names]
        self.colors = colors
        self.device = int(device)
        h = C.c_void_p()
        check(lib.ssd_annotate_style_create(self.device, len(names), np_ptr(colors), np_ptr(pack_names(names)), C.byref(h)))
        self._h = h

    def close(self):
        if self._h is not None:
            lib.ssd_annotate_style_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_offsets(shapes, itemsize):
    """Byte offsets of [h][w][3] images packed at 16-byte aligned offsets (as transforms.plan_params packs sources) + the total."""
    offs, off = [], 0
    for h, w in shapes:
        offs.append(off)
        off += (h * w * 3 * itemsize + 15) // 16 * 16
    return offs, off


def annotate_batch(src, src_offs, src_shapes, count, cls, box, out_cap, style, dst_shapes=None, boxes_on_1000_grid=True,
                   rgb_out=False, dst_float=False, stream=None):
    """Enqueue the drawing of a batch.  src: torch uint8 or float32 CUDA tensor (any shape) that holds image i as [h][w][3] at byte
    offset src_offs[i]; count / cls / box: torch int32 CUDA tensors or raw device addresses laid out [b] / [b, out_cap] /
    [b, out_cap, 4].  Returns (dst tensor, dst_offs, dst_shapes): a packed torch tensor (uint8, or float32 with dst_float) on
    the same device.  Asynchronous on `stream` (a raw hipStream_t; default torch's current stream)."""
    import torch
    b = len(src_shapes)
    dst_shapes = list(src_shapes) if dst_shapes is None else list(dst_shapes)
    src_f32 = src.dtype == torch.float32
    if not src_f32 and src.dtype != torch.uint8:
        raise ValueError('images must be uint8 or float32, got %s' % (src.dtype,))
    dst_offs, total = pack_offsets(dst_shapes, 4 if dst_float else 1)
    dev = src.device
    dst = torch.empty(max(total, 16) // (4 if dst_float else 1), dtype=torch.float32 if dst_float else torch.uint8, device=dev)
    arr = (_Image * max(b, 1))()
    for i in range(b):
        arr[i].src_off = int(src_offs[i]); arr[i].src_h, arr[i].src_w = int(src_shapes[i][0]), int(src_shapes[i][1])
        arr[i].dst_off = dst_offs[i]; arr[i].dst_h, arr[i].dst_w = int(dst_shapes[i][0]), int(dst_shapes[i][1])
    ws = torch.empty(max(int(lib.ssd_annotate_ws_bytes(b, out_cap)), 16), dtype=torch.uint8, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream

    def addr(t):
        return t.data_ptr() if hasattr(t, 'data_ptr') else t
    check(lib.ssd_annotate_batch_dev(src.data_ptr(), int(src_f32), C.cast(arr, C.c_void_p), b, addr(count), addr(cls), addr(box),
                                     int(out_cap), int(bool(boxes_on_1000_grid)), style._h, int(bool(rgb_out)), dst.data_ptr(),
                                     int(bool(dst_float)), ws.data_ptr(), stream))
    # (the scratch is released in stream order by torch's allocator; the structs were copied by the call)
    return dst, dst_offs, dst_shapes


def unpack(host, offs, shapes):
    """Per-image [h, w, 3] views of a packed host array (numpy, the dtype of the images)."""
    flat = host.reshape(-1)
    item = flat.dtype.itemsize
    return [flat[o // item:o // item + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(offs, shapes)]


# ------------------------------------------------------------------------------------------------ image files
def png_bytes(rgb):
    """A [h, w, 3] uint8 RGB array as an 8-bit truecolour PNG (stdlib zlib, filter-0 rows)."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]

    def chunk(kind, data):
        return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, w * 3)], 1).tobytes()
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(raw, 6))
            + chunk(b'IEND', b''))


def write_image(path, bgr):
    """cv2.imwrite(path, bgr) without OpenCV: Pillow when it is importable and writes the extension, else `<path>.png` from the
    built-in writer (a path that already ends in .png keeps its name).  Returns the path written."""
    bgr = np.asarray(bgr, np.uint8)
    rgb = bgr[:, :, ::-1]
    ext = os.path.splitext(path)[1].lower()
    if ext != '.png':
        try:
            from PIL import Image
            if ext in Image.registered_extensions():
                Image.fromarray(np.ascontiguousarray(rgb)).save(path)
                return path
        except Exception:
            pass
        path = path + '.png'
    with open(path, 'wb') as f:
        f.write(png_bytes(rgb))
    return path


def is_jpeg_name(path):
    return os.path.splitext(path)[1].lower() in ('.jpg', '.jpeg')


class GpuJpegWriter:
    """The drivers' --encoder gpu: annotated pictures whose output name ends in .jpg / .jpeg are encoded from the annotation
    launch's device buffer by jpeg.encode_launch and never reach the host as pixels; the other names of a batch go
    through write_image as before.  launch() right behind annotate_last_launch, write() where the batch is collected."""

    def __init__(self, quality=95, entropy='host'):
        self.quality, self.entropy = int(quality), entropy

    def launch(self, net, sources, style, paths):
        """paths: the output path of every image of the batch.  Returns the ticket write() takes."""
        jpg = [i for i, p in enumerate(paths) if is_jpeg_name(p)]
        drawn = net.annotate_last_launch(*sources, style, keep_device=bool(jpg), to_host=len(jpg) < len(paths))
        enc = None
        if jpg:
            from . import jpeg
            enc = jpeg.encode_launch(drawn.dev, [drawn.offs[i] for i in jpg], [drawn.shapes[i] for i in jpg], quality=self.quality,
                                     stream=drawn.stream, entropy=self.entropy)
        return drawn, enc, jpg, list(paths)

    def write(self, ticket):
        drawn, enc, jpg, paths = ticket
        if enc is not None:
            for i, data in zip(jpg, enc.get()):
                with open(paths[i], 'wb') as f:
                    f.write(data)
        if len(jpg) < len(paths):
            images = drawn.get()
            for i in sorted(set(range(len(paths))) - set(jpg)):
                write_image(paths[i], images[i])
