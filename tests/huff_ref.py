"""What the two Huffman-stage test files share (tests/test_jpeg_huffman.py, tests/test_gpu_jpeg_huffman.py): a pure-Python counter
of the bits of a scan that takes its code lengths from the DHT segments of the host stage's own file, descriptors for crafted
coefficients, and the seeded family of small images.  The host stage (jpeg.entropy_encode) is byte-identical to libjpeg-turbo on
the whole fixture (tests/test_jpeg_encode.py), so it is the oracle of the files; scan_bits is independent of its bit writer."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
HEADER = 623


def dht_lengths(data):
    """{table class * 16 + id: {symbol: code length}} from the DHT segments in front of the scan"""
    out, p = {}, 2
    while data[p + 1] != 0xDA:
        seg = data[p + 4:p + 2 + (data[p + 2] << 8 | data[p + 3])]
        if data[p + 1] == 0xC4:
            syms = iter(seg[17:])
            out[seg[0]] = {next(syms): l + 1 for l in range(16) for _ in range(seg[1 + l])}
        p += 2 + (data[p + 2] << 8 | data[p + 3])
    return out


def scan_bits(coef, d, lengths=None):
    """bits of the scan of coefficients `coef` (int16, natural order) under descriptor d; lengths: dht_lengths of a host-stage
    file (default: of this image's own)"""
    if lengths is None:
        from ssd_tensorflow_amd import jpeg
        lengths = dht_lengths(jpeg.entropy_encode(coef, d))
    bits, pred = 0, [0, 0, 0]
    for my in range(d.mcus_y):
        for mx in range(d.mcus_x):
            for c in range(3):
                h, v = (d.hs, d.vs) if c == 0 else (1, 1)
                dc, ac = lengths[0x00 + (c > 0)], lengths[0x10 + (c > 0)]
                for by in range(v):
                    for bx in range(h):
                        o = int(d.coef_off[c]) + ((my * v + by) * d.mcus_x * h + mx * h + bx) * 64
                        blk = [int(coef[o + ZIGZAG[k]]) for k in range(64)]
                        nb = abs(blk[0] - pred[c]).bit_length()
                        pred[c] = blk[0]
                        bits += dc[nb] + nb
                        run = 0
                        for x in blk[1:]:
                            if x == 0:
                                run += 1
                                continue
                            bits += (run >> 4) * ac[0xF0] + ac[(run & 15) << 4 | abs(x).bit_length()] + abs(x).bit_length()
                            run = 0
                        bits += ac[0] if run else 0
    return bits


def make_desc(width, height, hs=1, vs=1, quality=95, base=0):
    """(Desc, int16 elements of its coefficients): planes one after the other from element `base`, tables of `quality`"""
    from ssd_tensorflow_amd import jpeg
    d = jpeg.Desc()
    d.width, d.height, d.components, d.hs, d.vs = width, height, 3, hs, vs
    d.mcus_x, d.mcus_y = (width + 8 * hs - 1) // (8 * hs), (height + 8 * vs - 1) // (8 * vs)
    luma, chroma = jpeg.quant_tables(quality)
    off = base
    for c in range(3):
        d.coef_off[c] = off
        off += d.mcus_x * d.mcus_y * (hs * vs if c == 0 else 1) * 64
        for k in range(64):
            d.qt[c][k] = int((chroma if c else luma)[k])
    return d, off - base


def family(count, seed=11):
    """[int16 [192]]: 8 x 8 4:4:4 images (three blocks); per block a DC in +-1023 and 1..39 nonzero AC coefficients of categories
    1..10, either sign, at random zigzag positions"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        coef = np.zeros(192, np.int16)
        for b in range(3):
            coef[b * 64] = rng.integers(-1023, 1024)
            k = int(rng.integers(1, 40))
            for pos in rng.choice(np.arange(1, 64), k, replace=False):
                cat = int(rng.integers(1, 11))
                mag = int(rng.integers(1 << (cat - 1), 1 << cat))
                coef[b * 64 + ZIGZAG[pos]] = mag if rng.integers(0, 2) else -mag
        out.append(coef)
    return out
