#!/usr/bin/env python3
"""Writes tests/golden/j1_jpeg.npz: JPEG bytes and the BGR pixels Pillow (libjpeg-turbo) decodes them to, for tests/test_jpeg.py
and tests/test_gpu_jpeg.py.  Needs Pillow; the tests do not.

    python tools/make_jpeg_golden.py [--voc DIR]     # DIR: two VOC pictures 000032.jpg / 000232.jpg, stored as bytes + checksums

Keys: ok_names / ok_<i>_jpg / ok_<i>_bgr (supported files), voc_<name>_jpg / _shape / _sha256 / _rowsums, unsup_names /
unsup_<i>_jpg, bad_names / bad_<i>_jpg, guard_inside_jpg / guard_beyond_jpg (one crafted block each, test 8).
"""
import argparse
import hashlib
import io
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [('444', 0), ('422', 1), ('420', 2), ('gray', None)]
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def picture(rng, w, h, kind='scene'):
    """a colourful test picture: gradients, a few hard-edged shapes and mild noise (chroma detail at every sampling)"""
    if kind == 'flat':
        return np.full((h, w, 3), (90, 140, 200), np.uint8)
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / 7.0 + y / 13.0), 255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1)], -1)
    for _ in range(4):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        x1, y1 = x0 + int(rng.integers(1, w // 2 + 2)), y0 + int(rng.integers(1, h // 2 + 2))
        img[y0:y1, x0:x1] = rng.integers(0, 256, 3)
    img += rng.normal(0, 6, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(rgb, mode, quality=75, optimize=False, restarts=0, **kw):
    im = Image.fromarray(rgb)
    if mode[1] is None:
        im = im.convert('L')
    else:
        kw['subsampling'] = mode[1]
    if restarts:
        kw['restart_marker_blocks'] = restarts
    buf = io.BytesIO()
    im.save(buf, 'JPEG', quality=quality, optimize=optimize, **kw)
    return buf.getvalue()


def pillow_bgr(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


def segments(data):
    """[(marker, offset of its 0xFF, total length incl. marker)] up to and including SOS"""
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        L = (data[p + 2] << 8) | data[p + 3]
        out.append((m, p, L + 2))
        p += L + 2
        if m == 0xDA:
            return out, p


def find(data, marker):
    return next(s for s in segments(data)[0] if s[0] == marker)


def patched(data, marker, rel, value):
    _, off, _ = find(data, marker)
    b = bytearray(data)
    b[off + rel] = value
    return bytes(b)


def huffman_codes(data, tc, th):
    """{symbol: (code, length)} of table (tc, th) of a JPEG's DHT segments"""
    for m, off, L in segments(data)[0]:
        if m != 0xC4:
            continue
        seg = data[off + 4:off + L]
        s = 0
        while s < len(seg):
            c, h = seg[s] >> 4, seg[s] & 15
            counts = list(seg[s + 1:s + 17])
            vals = list(seg[s + 17:s + 17 + sum(counts)])
            s += 17 + sum(counts)
            if (c, h) == (tc, th):
                codes, code, k = {}, 0, 0
                for l in range(1, 17):
                    for _ in range(counts[l - 1]):
                        codes[vals[k]] = (code, l)
                        code += 1
                        k += 1
                    code <<= 1
                return codes
    raise KeyError((tc, th))


def crafted_block(template, coefs):
    """An 8 x 8 greyscale JPEG whose single block holds `coefs` (natural order, all 63 AC values non-zero) with an all-ones
    quantisation table: the template's headers and Huffman tables, the scan re-encoded here."""
    segs, scan = segments(template)
    dc, ac = huffman_codes(template, 0, 0), huffman_codes(template, 1, 0)
    head = bytearray(template[:scan])
    _, off, L = find(template, 0xDB)
    assert L == 2 + 2 + 65 and head[off + 4] == 0            # one 8-bit table
    head[off + 5:off + 69] = bytes([1] * 64)
    bits = []

    def put(code, length):
        bits.extend((code >> (length - 1 - i)) & 1 for i in range(length))

    def value(v):
        t = int(abs(v)).bit_length()
        return t, (v if v >= 0 else v + (1 << t) - 1)

    t, v = value(coefs[0])
    put(*dc[t]); put(v, t)
    for k in range(1, 64):
        t, v = value(coefs[ZIGZAG[k]])
        assert t > 0
        put(*ac[t]); put(v, t)
    bits.extend([1] * (-len(bits) % 8))
    body = bytearray()
    for i in range(0, len(bits), 8):
        byte = int(''.join(map(str, bits[i:i + 8])), 2)
        body.append(byte)
        if byte == 0xFF:
            body.append(0)
    return bytes(head) + bytes(body) + b'\xff\xd9'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--voc', default=None, help='directory with 000032.jpg and 000232.jpg')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'j1_jpeg.npz'))
    args = ap.parse_args()
    rng = np.random.default_rng(20261016)
    out, ok = {}, []

    # every sampling x quality x table kind x restart setting, walking through sizes whose remainders mod 16 are 0, 1, 8, 15
    sizes = [(64, 48), (17, 33), (49, 40), (72, 31), (95, 65), (33, 17), (104, 88), (47, 63), (80, 81), (31, 15), (144, 96), (56, 24)]
    k = 0
    for mode in MODES:
        for q in (30, 75, 95):
            for opt in (False, True):
                for rst in (0, 3):
                    w, h = sizes[k % len(sizes)]
                    k += 1
                    ok.append(('%s_q%d_%s_%s_%dx%d' % (mode[0], q, 'opt' if opt else 'std', 'rst3' if rst else 'norst', w, h),
                               encode(picture(rng, w, h), mode, q, opt, rst)))
    for mode in MODES:
        for w, h in ((1, 1), (8, 8), (16, 16), (17, 33)):
            ok.append(('%s_small_%dx%d' % (mode[0], w, h), encode(picture(rng, w, h), mode, 85)))
        ok.append(('%s_noise_40x24' % mode[0], encode(picture(rng, 40, 24, 'noise'), mode, 95)))      # all 63 AC positions
        ok.append(('%s_flat_40x24' % mode[0], encode(picture(rng, 40, 24, 'flat'), mode, 75)))        # DC only
    out['ok_names'] = np.array([n for n, _ in ok])
    for i, (_, data) in enumerate(ok):
        out['ok_%d_jpg' % i] = np.frombuffer(data, np.uint8)
        out['ok_%d_bgr' % i] = pillow_bgr(data)

    if args.voc:
        for name in ('000032', '000232'):
            data = open(os.path.join(args.voc, name + '.jpg'), 'rb').read()
            px = pillow_bgr(data)
            out['voc_%s_jpg' % name] = np.frombuffer(data, np.uint8)
            out['voc_%s_shape' % name] = np.array(px.shape[:2])
            out['voc_%s_sha256' % name] = np.array(hashlib.sha256(px.tobytes()).hexdigest())
            out['voc_%s_rowsums' % name] = px.astype(np.int64).sum(1).astype(np.int32)      # [h, 3]
        out['voc_names'] = np.array(['000032', '000232'])

    base = encode(picture(rng, 64, 48), MODES[2], 80)                       # a good 4:2:0 file to patch
    sof = find(base, 0xC0)[1]
    app0 = find(base, 0xE0)
    adobe = b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00'           # transform 0 and no JFIF marker: RGB to libjpeg
    cmyk = io.BytesIO()
    Image.fromarray(picture(rng, 32, 32)).convert('CMYK').save(cmyk, 'JPEG')
    unsup = [('progressive', encode(picture(rng, 48, 48), MODES[2], 80, progressive=True)),
             ('cmyk', cmyk.getvalue()),
             ('luma_1x2', patched(base, 0xC0, 11, 0x12)),
             ('luma_4x1', patched(base, 0xC0, 11, 0x41)),
             ('chroma_2x1', patched(base, 0xC0, 14, 0x21)),
             ('precision_12', patched(base, 0xC0, 4, 12)),
             ('arithmetic_sof9', base[:sof + 1] + b'\xc9' + base[sof + 2:]),
             ('adobe_transform_0', base[:app0[1]] + adobe + base[app0[1] + app0[2]:])]
    out['unsup_names'] = np.array([n for n, _ in unsup])
    for i, (_, data) in enumerate(unsup):
        out['unsup_%d_jpg' % i] = np.frombuffer(data, np.uint8)

    good = encode(picture(rng, 96, 80, 'noise'), MODES[2], 95, False, 2)    # restarts and stuffed bytes in the scan
    segs, scan = segments(good)
    dht, dqt, sofs = find(good, 0xC4), find(good, 0xDB), find(good, 0xC0)
    b = bytearray(good)
    b[dht[1] + 5:dht[1] + 9] = b'\xff\xff\xff\xff'
    dht_bad = bytes(b)
    b = bytearray(good)
    b[dqt[1] + 2:dqt[1] + 4] = b'\xff\xff'
    len_bad = bytes(b)
    sos_first = good[:sofs[1]] + good[sofs[1] + sofs[2]:scan] + good[sofs[1]:sofs[1] + sofs[2]] + good[scan:]
    st = next(i for i in range(scan, len(good) - 2) if good[i] == 0xFF and good[i + 1] == 0 and good[i + 2] not in (0, 0xFF))
    unstuffed = good[:st + 1] + good[st + 2:]
    rs = next(i for i in range(scan, len(good) - 1) if good[i] == 0xFF and 0xD0 <= good[i + 1] <= 0xD7)
    b = bytearray(good)
    b[rs + 1] = 0xD0 + ((good[rs + 1] - 0xD0 + 3) & 7)
    rst_bad = bytes(b)
    bad = [('truncated_10', good[:len(good) // 10]), ('truncated_50', good[:len(good) // 2]), ('truncated_99', good[:len(good) * 99 // 100]),
           ('dht_counts_past_256', dht_bad), ('sos_before_sof', sos_first), ('segment_length_past_end', len_bad),
           ('stuffing_removed', unstuffed), ('restart_wrong_index', rst_bad)]
    out['bad_names'] = np.array([n for n, _ in bad])
    out['bad_source_jpg'] = np.frombuffer(good, np.uint8)
    for i, (_, data) in enumerate(bad):
        out['bad_%d_jpg' % i] = np.frombuffer(data, np.uint8)

    # test 8: one block, coefficients of alternating sign in all 64 positions, L1 norm exactly at / one past the guard (q = 1)
    template = encode(picture(rng, 8, 8), MODES[3], 75)
    for name, dcv in (('inside', 258), ('beyond', 259)):
        coefs = [234 * (1 if i % 2 == 0 else -1) for i in range(64)]
        coefs[0] = dcv
        assert sum(abs(c) for c in coefs) == 15000 + (name == 'beyond')
        out['guard_%s_jpg' % name] = np.frombuffer(crafted_block(template, coefs), np.uint8)
        out['guard_%s_coefs' % name] = np.array(coefs, np.int16)

    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes;', len(ok), 'supported,', len(unsup), 'unsupported,', len(bad), 'corrupt')


if __name__ == '__main__':
    main()
