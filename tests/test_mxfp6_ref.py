"""CPU: the mxfp6 oracle (tests/mxfp6_ref.py) against the format's definition: the decode table, round to nearest
even with its ties, the packing, and the scale rule on bits against the rule by exact arithmetic."""
from fractions import Fraction

import numpy as np

import mxfp6_ref as m6


def bits(u):
    return np.array(u, np.uint32).view(np.float32)


def test_decode_table_is_the_definition():
    assert m6.DECODE.shape == (64,)
    mags = [0.0] + [i / 8 for i in range(1, 8)] + [1 + i / 8 for i in range(8)] + [2 + i / 4 for i in range(8)] + [4 + i / 2 for i in range(8)]
    assert m6.DECODE[:32].tolist() == mags and m6.DECODE[32:].tolist() == [-v for v in mags]
    for c in range(64):
        s, e, m = c >> 5, (c >> 3) & 3, c & 7
        v = Fraction(m, 8) if e == 0 else (1 + Fraction(m, 8)) * Fraction(2) ** (e - 1)
        assert Fraction(m6.DECODE[c]) == (-v if s else v)
    assert m6.DECODE[31] == 7.5 and m6.DECODE[8] == 1.0 and m6.DECODE[1] == 0.125
    assert np.all(np.isfinite(m6.DECODE))                                          # no Inf / NaN codes


def test_encode_rounds_to_nearest_even_and_saturates():
    d = lambda v: m6.decode(m6.encode(np.array(v, np.float64))).tolist()
    # the named ties: halfway between two codes, the one with the even mantissa wins
    assert d([0.0625, 0.1875, 1.0625, 1.1875, 7.25]) == [0.0, 0.25, 1.0, 1.25, 7.0]
    assert d([-0.0625, -0.1875, -7.25, 6.75, 3.875, 1.9375]) == [-0.0, -0.25, -7.0, 7.0, 4.0, 2.0]
    assert d([7.5, 7.75, 100.0, -1e30, 7.4999]) == [7.5, 7.5, 7.5, -7.5, 7.5]
    assert np.array_equal(m6.encode(m6.DECODE), np.arange(64, dtype=np.uint8))      # every value is its own code
    # against the nearest grid value by exact search, off ties
    rng = np.random.default_rng(61)
    v = rng.uniform(-8, 8, 4000)
    near = m6.DECODE[:32][np.abs(np.abs(v)[:, None] - m6.DECODE[None, :32]).argmin(1)] * np.sign(v)
    assert np.array_equal(m6.decode(m6.encode(v)), near)


def test_pack_round_trip_and_bit_order():
    rng = np.random.default_rng(62)
    codes = rng.integers(0, 64, (5, 7, 96)).astype(np.uint8)
    p = m6.pack(codes)
    assert p.shape == (5, 7, 3, 24) and p.dtype == np.uint8
    assert np.array_equal(m6.unpack(p), codes)
    # code j in bits 6 j ... 6 j + 5 of the little-endian 24-byte string
    for j in (0, 1, 5, 21, 31):
        one = np.zeros(32, np.uint8)
        one[j] = 63
        n = int.from_bytes(m6.pack(one).reshape(24).tobytes(), 'little')
        assert n == 63 << (6 * j)
    n = int.from_bytes(p[2, 3, 1].tobytes(), 'little')
    assert [(n >> (6 * j)) & 63 for j in range(32)] == codes[2, 3, 32:64].tolist()


def test_scale_bytes_at_the_named_points():
    sb = lambda a: int(m6.scale_exponent(np.array([a], np.float32))[0]) + 127
    assert sb(7.5) == 127 and sb(7.5 * 32) == 132 and sb(7.5 / 512) == 118 and sb(1.875) == 125
    assert sb(np.nextafter(np.float32(1.875), np.float32(2))) == 126                # the next fp32 value ...
    assert sb(bits([(np.float32(1.875).view(np.uint32) + 0x10000)])[0]) == 126      # ... and the next bf16 value (1.8828125)
    assert float(bits([(np.float32(1.875).view(np.uint32) + 0x10000)])[0]) == 1.8828125
    assert sb(np.nextafter(np.float32(7.5), np.float32(8))) == 128 and sb(np.nextafter(np.float32(7.5), np.float32(0))) == 127
    assert sb(1.0) == 125 and sb(2.0) == 126 and sb(4.0) == 127 and sb(8.0) == 128
    z = np.zeros((1, 32), np.float32)
    p, s = m6.quantize(z)
    assert s[0, 0] == 0 and not p.any()                                              # an all-zero block: byte 0
    big = np.full((1, 32), np.finfo(np.float32).max, np.float32)
    p, s = m6.quantize(big)
    assert s[0, 0] == 127 + 126 and s.max() < 255                                    # never byte 255


def test_rule_equals_definition_over_all_exponents():
    out = []
    for k in range(-126, 128):
        base = np.float32(np.ldexp(1.875, k)).view(np.uint32)                        # (7.5 * 2^k is 1.875 * 2^(k + 2))
        one = np.float32(np.ldexp(1.0, k)).view(np.uint32)
        out += [base - 1, base, base + 1, one, one + 1]
    v = bits(out)
    v = v[np.isfinite(v)]
    assert v.size > 1200
    assert np.array_equal(m6.scale_exponent(v), m6.scale_exponent_by_definition(v))
    rng = np.random.default_rng(63)
    r = bits(rng.integers(0x00800000, 0x7F800000, 5000, dtype=np.uint32))
    assert np.array_equal(m6.scale_exponent(r), m6.scale_exponent_by_definition(r))


def test_every_block_uses_its_range():
    rng = np.random.default_rng(64)
    v = (rng.normal(0, 1, (500, 64)) * np.exp2(rng.integers(-20, 20, (500, 2)).repeat(32, 1))).astype(np.float32)
    codes, scales = m6.quantize_codes(v)
    top = np.abs(m6.decode(codes)).reshape(500, 2, 32).max(-1)
    assert np.all(top >= 3.75) and np.all(top <= 7.5)
    p, s = m6.quantize(v)
    assert np.array_equal(s, scales) and np.array_equal(m6.unpack(p), codes)
    back = m6.dequantize(p, s)
    assert np.all(np.abs(back - v) <= np.repeat(m6.scale_values(s), 32, -1) * m6.e2m3_step(m6.decode(codes)) / 2)


def test_identity_on_small_integer_blocks_and_filters():
    rng = np.random.default_rng(65)
    i = rng.integers(0, 8, (300, 96))
    i[:, ::32] = 7
    s = rng.integers(-40, 40, (300, 3)).repeat(32, 1)
    v = np.ldexp(i.astype(np.float32), s).astype(np.float32)
    v[5] = 0
    for sign in (1, -1):
        p, sc = m6.quantize(sign * v)
        assert np.array_equal(m6.dequantize(p, sc), sign * v.astype(np.float64))
    # filters: blocks along Ci, [tap][Co][Ci / 32][24]
    w = np.ldexp(rng.integers(-3, 4, (3, 3, 64, 40)).astype(np.float32), rng.integers(-5, 5, (3, 3, 2, 40)).repeat(32, 2)).astype(np.float32)
    w6, ws = m6.quantize_filter(w)
    assert w6.shape == (9, 40, 2, 24) and ws.shape == (9, 40, 2)
    assert np.array_equal(m6.dequantize_filter(w6, ws, 3, 3), w.astype(np.float64))


def test_conv_values_and_bound():
    rng = np.random.default_rng(66)
    x = rng.integers(-3, 4, (1, 4, 5, 32)).astype(np.float64)
    w = rng.integers(-2, 3, (3, 3, 32, 8)).astype(np.float64)
    acc, absacc = m6.conv_values(x, w, 1, 1, 'SAME')
    assert acc.shape == (1, 4, 5, 8) and np.all(absacc >= np.abs(acc))
    want = sum(x[0, 1 + dh, 2 + dw] @ w[1 + dh, 1 + dw] for dh in (-1, 0, 1) for dw in (-1, 0, 1))
    assert np.array_equal(acc[0, 1, 2], want)
    rows, _ = m6.conv_values_rows(x, w, 1, 1, 3)
    assert np.array_equal(rows, acc[:, 1:3])
    assert np.array_equal(m6.accumulation_bound(absacc, 288), 288 * 2.0 ** -23 * absacc)
    assert np.array_equal(m6.epilogue(acc, np.ones(8), True), np.maximum(acc + 1, 0))


def test_pool_requantises_per_block():
    codes = np.zeros((1, 2, 2, 32), np.uint8)
    scales = np.array([127, 130, 120, 127], np.uint8).reshape(1, 2, 2, 1)
    codes[0, 0, 0, :] = m6.encode(np.full(32, 3.0))                 # 3
    codes[0, 0, 1, :] = m6.encode(np.full(32, 1.0))                 # 8: the window's maximum
    codes[0, 1, 0, :] = m6.encode(np.full(32, 7.5))                 # 7.5 / 128
    codes[0, 1, 1, 0] = m6.encode(np.array([5.0]))[0]               # channel 0: 5 < 8
    codes[0, 1, 1, 1] = m6.encode(np.array([-5.0]))[0]
    y6, ys = m6.maxpool(m6.pack(codes), scales, 2, 2)
    assert y6.shape == (1, 1, 1, 1, 24) and ys.shape == (1, 1, 1, 1)
    got = m6.dequantize(y6, ys)[0, 0, 0]
    assert np.all(got == 8.0) and ys[0, 0, 0, 0] == 128
