"""CPU: the host half of the drawing feature (include/ssdvgg_hip.h "drawing detections"): the shared geometry function and the
font table through their host entry points, the numpy yardstick (tests/annotate_ref.py) against hand-counted cases and against
the oracle's float64 resize, the built-in PNG writer, the Python surface."""
import struct
import zlib

import numpy as np

import annotate_ref as R
from ssd_tensorflow_amd import annotate as A
from ssd_tensorflow_amd import utils as ut


def test_rect_equals_the_reference_functions():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 1000, (10000, 2)); b = rng.integers(0, 1000, (10000, 2))
    boxes = np.stack([a.min(1), a.max(1), b.min(1), b.max(1)], 1)
    boxes[:200, 1] = boxes[:200, 0]                      # x0 == x1
    boxes[200:400, 0] = 0; boxes[400:600, 1] = 999       # touching 0 and 999
    boxes[600:700, 2] = 0; boxes[700:800, 3] = 999
    for w, h in ((1, 1), (37, 23), (300, 300), (500, 375), (1920, 1080)):
        for bx in boxes:
            want = ut.prop2abs(*ut.abs2prop(int(bx[0]), int(bx[1]), int(bx[2]), int(bx[3]), ut.Size(1000, 1000)), ut.Size(w, h))
            assert A.rect_on_image(bx, w, h) == want, (bx, w, h)


def test_font_table():
    glyphs = {ch: tuple(A.glyph(ch)) for ch in range(32, 127)}
    assert all(len(g) == 7 and all(0 <= r < 32 for r in g) for g in glyphs.values())
    assert not any(glyphs[32])
    assert all(any(glyphs[ch]) for ch in range(33, 127))
    assert len(set(glyphs.values())) == 95
    for ch in (0, 10, 31, 127, 200, 255):
        assert tuple(A.glyph(ch)) == glyphs[ord('?')]


def test_yardstick_hand_counted():
    img = np.full((80, 100, 3), 100, np.uint8)
    # a box well inside, no label: ring = 53 x 33 outer minus 47 x 27 inner; tag = 53 x 21 rows 10..30, of which rows 29, 30 are ring too
    rect = (20, 70, 30, 60)
    cov, txt = R.coverage(img.shape[:2], rect, '')
    assert not txt.any()
    assert cov.sum() == (53 * 33 - 47 * 27) + 53 * 21 - 53 * 2
    # the tag cut by the top edge: ymin = 5 -> tag rows 0..5 of -15..5
    cov2, _ = R.coverage(img.shape[:2], (20, 70, 5, 60), '')
    assert cov2[:4].sum() == 53 * 4 and cov2[0, 19] and not cov2[0, 18] and cov2[0, 71] and not cov2[0, 72]
    # text: one '!' = six lit font pixels of 2 x 2, white; character 1 starts 12 pixels further right
    cov3, txt3 = R.coverage(img.shape[:2], rect, '!!')
    assert txt3.sum() == 2 * 6 * 4 and txt3[30 - 18, 20 + 5 + 4] and txt3[30 - 18, 20 + 5 + 12 + 4] and not txt3[30 - 18, 20 + 5]
    # one blended value: v = 100, d = 200 -> 0.8 * 200 + 0.2 * 100 = 180
    out = R.draw(img, [(rect, (200, 200, 200), '')])
    assert out[30, 20, 0] == 180 and out[45, 45, 0] == 100 and (out[cov] == 180).all() and (out[~cov] == 100).all()
    # float: kept in float, unclamped
    outf = R.draw(np.full((80, 100, 3), 300, np.float32), [(rect, (200, 255, 0), '!')])
    assert outf.dtype == np.float32 and outf[30, 20, 1] == np.float32(0.8) * np.float32(255) + np.float32(0.2) * np.float32(300)
    # a label is cut at 31 characters
    assert R.coverage((40, 500), (2, 400, 25, 35), 'M' * 40)[1].sum() == R.coverage((40, 500), (2, 400, 25, 35), 'M' * 31)[1].sum()


def test_yardstick_resize_against_the_oracle():
    from oracle import augment as oa
    rng = np.random.default_rng(3)
    total = differ = 0
    for k in range(8):
        integer = k % 2 == 1
        img = rng.integers(0, 256, (300, 300, 3)).astype(np.float32) if integer else rng.uniform(-20, 280, (300, 300, 3)).astype(np.float32)
        got = R.to_u8(R.resize_linear(img, 512, 512))
        want = R.to_u8(oa.resize(img, 512, 512, oa.INTER_LINEAR))
        diff = np.abs(got.astype(int) - want.astype(int))
        assert diff.max() <= 1
        if integer:
            assert not diff.any()
        total += diff.size; differ += int((diff != 0).sum())
    print('resize: %d of %d bytes differ' % (differ, total))
    assert differ <= 1e-4 * total


def _decode_png(data):
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, size = 8, b'', None
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff
        if kind == b'IHDR':
            w, h, depth, ctype = struct.unpack('>IIBB', body[:10])
            assert (depth, ctype) == (8, 2)
            size = (h, w)
        elif kind == b'IDAT':
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(size[0], 1 + size[1] * 3)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(size[0], size[1], 3)


def test_png_writer_round_trips(tmp_path):
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (23, 37, 3)).astype(np.uint8)
    assert np.array_equal(_decode_png(A.png_bytes(rgb)), rgb)
    path = A.write_image(str(tmp_path / 'x.npy'), rgb[:, :, ::-1])
    assert path.endswith('x.npy.png') and np.array_equal(_decode_png(open(path, 'rb').read()), rgb)


def test_surface():
    from ssd_tensorflow_amd import source_pascal_voc as voc
    assert callable(ut.draw_box) and callable(ut.default_colors)
    assert ut.default_colors(voc.VOC_NAMES) == voc.PascalVOCSource().colors
    other = ut.default_colors(['a', 'b', 'c'])
    assert list(other) == ['a', 'b', 'c'] and len(set(other.values())) == 3 and other == ut.default_colors(['a', 'b', 'c'])
    assert A.pack_names(['x' * 40, 'ok']).shape == (2, 32) and A.pack_names(['x' * 40])[0, 30] == ord('x') and A.pack_names(['x' * 40])[0, 31] == 0
