"""GPU: the drawing kernel (csrc/annotate.hip) through the C ABI against the numpy yardstick (tests/annotate_ref.py), for exact
equality: integer coverage and separately rounded float32 arithmetic on both sides.  Ordinary runs only."""
import ctypes as C

import numpy as np
import pytest
import torch

import annotate_ref as R
from gpu_util import DEV, dev
from ssd_tensorflow_amd import annotate as A
from ssd_tensorflow_amd import utils as ut
from ssd_tensorflow_amd._lib import lib, last_error

pytestmark = pytest.mark.gpu

NAMES = ['aeroplane', 'b', 'a label of exactly 31 characters', 'a label that is longer than thirty-one characters', 'dog {~}']
COLORS = [(0, 0, 255), (10, 200, 30), (255, 128, 0), (1, 2, 3), (250, 250, 250)]
SIZES = [(1, 1), (23, 37), (375, 500), (1080, 1920)]      # (h, w)


def pack(images):
    shapes = [im.shape[:2] for im in images]
    offs, total = A.pack_offsets(shapes, images[0].dtype.itemsize)
    buf = np.zeros(max(total, 16), np.uint8)
    for o, im in zip(offs, images):
        buf[o:o + im.nbytes] = np.frombuffer(im.tobytes(), np.uint8)
    t = dev(buf)
    return (t.view(torch.float32) if images[0].dtype == np.float32 else t), offs, shapes


def slot(rects, classes, out_cap, counts=None):
    """count / cls / box arrays laid out like ssd_detect_last_dev's outputs"""
    b = len(rects)
    count = np.array([len(r) for r in rects] if counts is None else counts, np.int32)
    cls = np.zeros((b, out_cap), np.int32); box = np.zeros((b, out_cap, 4), np.int32)
    for i in range(b):
        n = min(len(rects[i]), out_cap)
        cls[i, :n] = classes[i][:n]; box[i, :n] = np.asarray(rects[i], np.int64).reshape(-1, 4)[:n]
    return dev(count), dev(cls), dev(box)


def run(images, rects, classes, out_cap, grid1000=False, dst_shapes=None, rgb_out=False, dst_float=False, counts=None):
    style = A.Style(COLORS, NAMES, 0)
    try:
        src, offs, shapes = pack(images)
        count, cls, box = slot(rects, classes, out_cap, counts)
        dst, doffs, dshapes = A.annotate_batch(src, offs, shapes, count, cls, box, out_cap, style, dst_shapes=dst_shapes,
                                               boxes_on_1000_grid=grid1000, rgb_out=rgb_out, dst_float=dst_float)
        torch.cuda.synchronize()
        return [a.copy() for a in A.unpack(dst.cpu().numpy(), doffs, dshapes)]
    finally:
        style.close()


def want(img, rects, classes, out_cap, grid1000=False, count=None):
    n = min(len(rects) if count is None else count, out_cap, len(rects))
    h, w = img.shape[:2]
    px = [R.rect1000(r, w, h) if grid1000 else r for r in rects[:n]]
    return R.draw(img, R.style_boxes(px, classes[:n], COLORS, NAMES))


def random_rects(rng, n, h, w, spread=0.3):
    """boxes around the image: partly and wholly outside included"""
    x = np.sort(rng.integers(int(-spread * w) - 30, int((1 + spread) * w) + 30, (n, 2)), 1)
    y = np.sort(rng.integers(int(-spread * h) - 30, int((1 + spread) * h) + 30, (n, 2)), 1)
    return [tuple(int(v) for v in (x[i, 0], x[i, 1], y[i, 0], y[i, 1])) for i in range(n)]


def special_rects(h, w):
    return [(w // 3, w // 3, h // 4, h // 2),              # zero width
            (w // 2, w // 2 + 40, 5, h // 2),              # tag cut by the top edge
            (w - 60, w - 10, h // 2, h // 2 + 30),         # text running past the right edge
            (-500, -300, -400, -200),                      # wholly outside
            (w + 40, w + 90, 10, 50),
            (5, 9, h - 3, h + 30),                         # partly outside, bottom
            (-10, w + 10, -10, h + 10)]                    # around the whole image


def test_uint8_pixel_rects_against_the_yardstick():
    rng = np.random.default_rng(11)
    images = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
    rects, classes = [], []
    for i, (h, w) in enumerate(SIZES):
        r = special_rects(h, w) + random_rects(rng, 14, h, w)
        c = [int(v) for v in rng.integers(0, len(NAMES), len(r))]
        c[0], c[1], c[2], c[3] = 2, 3, 0, 7            # the 31-character label, the longer one, ..., a class id out of range
        c[-1] = -1
        rects.append(r); classes.append(c)
    rects[1] = []                                          # 0 boxes: the output equals the input
    out_cap = 24
    got = run(images, rects, classes, out_cap)
    assert np.array_equal(got[1], images[1])
    for i in range(len(SIZES)):
        assert np.array_equal(got[i], want(images[i], rects[i], classes[i], out_cap)), SIZES[i]
    # two launches on the same inputs give identical bytes
    again = run(images, rects, classes, out_cap)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_many_overlapping_boxes_and_count_above_out_cap():
    rng = np.random.default_rng(12)
    h, w = 375, 500
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    cx = rng.integers(200, 300, 200); cy = rng.integers(150, 230, 200); sx = rng.integers(20, 180, 200); sy = rng.integers(20, 140, 200)
    rects = [tuple(int(v) for v in (cx[k] - sx[k], cx[k] + sx[k], cy[k] - sy[k], cy[k] + sy[k])) for k in range(200)]
    classes = [int(v) for v in rng.integers(0, len(NAMES), 200)]
    got = run([img, img], [rects, rects], [classes, classes], 200)
    ref = want(img, rects, classes, 200)
    assert np.array_equal(got[0], ref) and np.array_equal(got[1], ref)
    assert not np.array_equal(ref, want(img, rects[::-1], classes[::-1], 200))      # the order matters
    # count > out_cap: min(count, out_cap) boxes are drawn
    got = run([img], [rects], [classes], 40, counts=[200])
    assert np.array_equal(got[0], want(img, rects, classes, 40))


def test_boxes_on_the_1000_grid():
    rng = np.random.default_rng(13)
    images = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
    rects, classes = [], []
    for h, w in SIZES:
        x = np.sort(rng.integers(0, 1000, (20, 2)), 1); y = np.sort(rng.integers(0, 1000, (20, 2)), 1)
        r = [tuple(int(v) for v in (x[k, 0], x[k, 1], y[k, 0], y[k, 1])) for k in range(20)]
        r[0] = (r[0][0], r[0][0], r[0][2], r[0][3]); r[1] = (0, 999, 0, 999)
        rects.append(r); classes.append([int(v) for v in rng.integers(0, len(NAMES) + 1, 20)])
    got = run(images, rects, classes, 20, grid1000=True)
    for i in range(len(SIZES)):
        assert np.array_equal(got[i], want(images[i], rects[i], classes[i], 20, grid1000=True)), SIZES[i]


def test_float32_paths():
    rng = np.random.default_rng(14)
    imgs = [rng.uniform(-40, 300, (300, 300, 3)).astype(np.float32) for _ in range(3)]      # fractional, out of range
    imgs[2] = np.rint(imgs[2]).astype(np.float32)
    rects = [random_rects(rng, 20, 1000, 1000, 0.0) for _ in imgs]
    rects = [[tuple(int(np.clip(v, 0, 999)) for v in r) for r in rr] for rr in rects]
    classes = [[int(v) for v in rng.integers(0, len(NAMES), 20)] for _ in imgs]
    # without a resize, BGR out, float destination: the unclamped floats bit for bit
    got = run(imgs, rects, classes, 20, grid1000=True, dst_float=True)
    for i in range(3):
        ref = want(imgs[i], rects[i], classes[i], 20, grid1000=True)
        assert got[i].dtype == np.float32 and np.array_equal(got[i].view(np.uint32), ref.view(np.uint32))
    # without a resize, uint8 destination: clamped and truncated after the last box
    got = run(imgs, rects, classes, 20, grid1000=True)
    for i in range(3):
        assert np.array_equal(got[i], R.to_u8(want(imgs[i], rects[i], classes[i], 20, grid1000=True)))
    # 300 x 300 -> 512 x 512, RGB out (what the image summaries ask for)
    got = run(imgs, rects, classes, 20, grid1000=True, dst_shapes=[(512, 512)] * 3, rgb_out=True)
    for i in range(3):
        big = R.resize_linear(imgs[i], 512, 512)
        assert np.array_equal(got[i], R.to_u8(want(big, rects[i], classes[i], 20, grid1000=True))[:, :, ::-1]), i
    got = run(imgs[:1], [[]], [[]], 4, dst_shapes=[(512, 512)], dst_float=True)
    assert np.array_equal(got[0].view(np.uint32), R.resize_linear(imgs[0], 512, 512).view(np.uint32))


def test_draw_box_in_place():
    rng = np.random.default_rng(15)
    box = ut.Box('person', 14, ut.Point(0.41, 0.52), ut.Size(0.33, 0.47))
    for dtype in (np.uint8, np.float32):
        img = rng.integers(0, 256, (211, 317, 3)).astype(dtype)
        if dtype == np.float32:
            img = img * np.float32(1.3) - np.float32(20.25)
        ref = R.draw(img, [(ut.prop2abs(box.center, box.size, ut.Size(317, 211)), (30, 200, 90), 'person')])
        ut.draw_box(img, box, (30, 200, 90))
        assert img.dtype == dtype and np.array_equal(img.view(np.uint32) if dtype == np.float32 else img, ref.view(np.uint32) if dtype == np.float32 else ref)
        assert not np.array_equal(img, np.zeros_like(img))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_from_a_real_detection_slot(dtype):
    from oracle import boxes as ob, ssdvgg_ref as ref
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    b = 3
    preset = ob.get_preset('vgg300')
    rng = np.random.default_rng(2)
    x, _, _ = ref.synth_batch(rng, b, preset)
    names = ['class_%d' % i for i in range(20)]
    colors = [ut.default_colors(names)[n] for n in names]
    sizes = [(300, 300), (211, 317), (375, 500)]
    images = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 20, max_batch=b, training=False, weights=ref.init_params(preset, 20, seed=1, alive=True), dtype=dtype)
        result = net.infer(torch.from_numpy(x).to(DEV))
        thr = float(np.quantile(result[:, :, :20].max(-1), 0.999))
        style = A.Style(colors, names, 0)
        try:
            src, offs, shapes = pack(images)
            ticket = net.detect_last_launch(b, thr, None, 200)
            drawn = net.annotate_last_launch(src, offs, shapes, style)
            dets = [{k: v.copy() for k, v in d.items()} for d in ticket.get()]
            got = drawn.get()
        finally:
            style.close()
    assert sum(len(d['cls']) for d in dets) > 0
    for i, (h, w) in enumerate(sizes):
        px = [R.rect1000(bx, w, h) for bx in dets[i]['box']]
        assert np.array_equal(got[i], R.draw(images[i], R.style_boxes(px, dets[i]['cls'], colors, names))), i


def test_error_paths_leave_the_process_usable():
    style = A.Style(COLORS, NAMES, 0)
    img = np.zeros((8, 8, 3), np.uint8)
    src, offs, shapes = pack([img])
    count, cls, box = slot([[]], [[]], 4)
    dst = torch.empty(1024, dtype=torch.uint8, device=DEV); ws = torch.empty(4096, dtype=torch.uint8, device=DEV)

    def call(b=1, w=8, h=8, dw=8, dh=8, src_f32=0, dst_f32=0, srcp=None, st=style):
        arr = (A._Image * 1)()
        arr[0].src_off = 0; arr[0].src_w = w; arr[0].src_h = h; arr[0].dst_off = 0; arr[0].dst_w = dw; arr[0].dst_h = dh
        return lib.ssd_annotate_batch_dev(src.data_ptr() if srcp is None else srcp, src_f32, C.cast(arr, C.c_void_p), b, count.data_ptr(),
                                          cls.data_ptr(), box.data_ptr(), 4, 0, st._h if st is not None else None, 0, dst.data_ptr(), dst_f32,
                                          ws.data_ptr(), None)
    assert call(b=0) != 0 and 'batch' in last_error()
    assert call(dw=16, dh=16) != 0 and 'resize' in last_error()
    assert call(w=0, dw=0) != 0 and 'zero size' in last_error()
    assert call(srcp=0) != 0 and 'null' in last_error()
    assert call(st=None) != 0 and 'null' in last_error()
    assert call(dst_f32=1) != 0 and 'float32' in last_error()
    h = C.c_void_p()
    for nc in (0, 128):
        assert lib.ssd_annotate_style_create(0, nc, src.data_ptr(), src.data_ptr(), C.byref(h)) != 0 and 'num_classes must be in 1..127' in last_error()
    assert lib.ssd_annotate_style_create(0, 2, None, None, C.byref(h)) != 0 and 'null' in last_error()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(dst[:192].cpu().numpy(), img.reshape(-1))
    style.close()
