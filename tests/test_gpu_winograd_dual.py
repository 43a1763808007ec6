"""-m gpu: backward's transforms of dy as ONE kernel (csrc/winograd.hip launch_in: wino_in_kernel<true, true> reads dy once and writes
Yt = B^T dy B for the data gradient and Ya = A dy A^T for the weight gradient) against the two single launches the step ran before
(flags bit 4 of ssd_op_wino_bwd_transform), through the C ABI.  Every output value is the same expression in the same order, so the
assertion is BITWISE equality of Yt and of Ya between the forms; the pad columns (Co ... kpad(Co) - 1) are zeros in both and the guard
words around the buffers keep their pattern.  The buffers start as NaNs: a word that a form did not write would show."""
import zlib
import numpy as np
import pytest
import torch

from gpu_util import lib, check, dev, ptr

pytestmark = pytest.mark.gpu
REF, TWO = 8, 16      # flags bit 3: the reference geometry; bit 4: two launches
GUARD = 64            # words in front of and behind each buffer (a multiple of 4: the kernel stores 16-byte vectors)
PATTERN = 0x7FC0BEEF  # a quiet NaN

# (name, h, w, co, b, dilation): the smallest shapes at which each thing can go wrong
CASES = [
    ('3x3 co4 b1: one tile per image, one quad', 3, 3, 4, 1, 1),
    ('5x7 co32 b3: ragged in both axes', 5, 7, 32, 3, 1),
    ('6x10 co100 b2: pad to 128, the head', 6, 10, 100, 2, 1),
    ('19x19 co152 b1: pad to 160', 19, 19, 152, 1, 1),
    ('7x7 co32 b2 dilation 2', 7, 7, 32, 2, 2),
    ('19x19 co32 b1 dilation 6: residue-class tiles, mod_conv6', 19, 19, 32, 1, 6),
    ('32x32 co64 b4: 32 workgroups, the XCD remap permutes them', 32, 32, 64, 4, 1),
    ('9x9 co36 b5: T Cp / 4 = 720, a partly empty last workgroup', 9, 9, 36, 5, 1),
]


def tiles_1d(n, dil):
    return dil * -(-(-(-n // dil)) // 4)


def transform(dy_, b, h, w, co, dil, flags):
    """-> (Yt, Ya) as uint32 [36][tiles][kpad(co)] on the host, after the guards were checked"""
    cp = (co + 31) // 32 * 32
    tiles = b * tiles_1d(h, dil) * tiles_1d(w, dil)
    n = 36 * tiles * cp
    out = []
    bufs = [torch.full((GUARD + n + GUARD,), PATTERN, dtype=torch.int32, device='cuda') for _ in range(2)]
    check(lib.ssd_op_wino_bwd_transform(ptr(dy_), bufs[0].data_ptr() + 4 * GUARD, bufs[1].data_ptr() + 4 * GUARD, b, h, w, co, dil, flags, None))
    torch.cuda.synchronize()
    for what, buf in zip(('Yt', 'Ya'), bufs):
        raw = buf.cpu().numpy().view(np.uint32)
        assert np.all(raw[:GUARD] == PATTERN) and np.all(raw[GUARD + n:] == PATTERN), f'{what}: guard words overwritten (flags {flags})'
        out.append(raw[GUARD:GUARD + n].reshape(36, tiles, cp))
    return out


def run_case(name, h, w, co, b, dil, extra=0):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    dy = rng.normal(0, 1, (b, h, w, co)).astype(np.float32)
    dy_ = dev(dy)
    dual = transform(dy_, b, h, w, co, dil, extra)
    two = transform(dy_, b, h, w, co, dil, extra | TWO)
    for what, a, t in zip(('Yt', 'Ya'), dual, two):
        assert np.array_equal(a, t), f'{name}: {what} differs between the forms in {np.count_nonzero(a != t)} of {a.size} words'
        for form, v in (('dual', a), ('two launches', t)):
            assert not np.any(v[:, :, co:]), f'{name}: {what} ({form}): pad columns not zero'
            f = v.view(np.float32)
            assert np.all(np.isfinite(f)), f'{name}: {what} ({form}): words left unwritten'
            assert np.count_nonzero(f[:, :, :co]) > 0.5 * f[:, :, :co].size
    return dual


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_dual_bit_identical_to_two_launches(case):
    run_case(*case)


def test_dual_reference_geometry():
    # raster-order workgroups in both forms, and the same bits as the default order
    case = CASES[6]
    ref = run_case(*case, extra=REF)
    default = run_case(*case)
    for what, a, t in zip(('Yt', 'Ya'), ref, default):
        assert np.array_equal(a, t), f'{what}: the reference geometry differs from the default one'


def test_dual_values():
    # equal is not yet right: the transforms of one tile against their definitions in float64
    name, h, w, co, b = 'values 5x7 co32 b3', 5, 7, 32, 3
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    dy = rng.normal(0, 1, (b, h, w, co)).astype(np.float32)
    yt, ya = [v.view(np.float32) for v in transform(dev(dy), b, h, w, co, 1, 0)]
    bt = np.array([[1.265625, 0, -2.8125, 0, 1, 0], [0, -1.6875, -2.25, 0.75, 1, 0], [0, 1.6875, -2.25, -0.75, 1, 0],
                   [0, -0.84375, -0.5625, 1.5, 1, 0], [0, 0.84375, -0.5625, -1.5, 1, 0], [0, 1.265625, 0, -2.8125, 0, 1]])
    am = np.array([[1, 0, 0, 0], [1, 0.75, 0.5625, 0.421875], [1, -0.75, 0.5625, -0.421875], [1, 1.5, 2.25, 3.375],
                   [1, -1.5, 2.25, -3.375], [0, 0, 0, 1]])
    th, tw = 2, 2
    padded = np.zeros((b, 4 * th + 2, 4 * tw + 2, co))
    padded[:, 1:1 + h, 1:1 + w] = dy
    for bi, i, j in ((0, 0, 0), (1, 1, 1), (2, 0, 1)):
        t = (bi * th + i) * tw + j
        patch = padded[bi, 4 * i:4 * i + 6, 4 * j:4 * j + 6]                     # [6][6][co], from pixel (4i - 1, 4j - 1)
        want_t = np.einsum('kr,rsc,ls->klc', bt, patch, bt).reshape(36, co)
        want_a = np.einsum('kr,rsc,ls->klc', am, patch[1:5, 1:5], am).reshape(36, co)
        assert np.abs(yt[:, t, :co] - want_t).max() < 1e-5 * np.abs(want_t).max()
        assert np.abs(ya[:, t, :co] - want_a).max() < 1e-5 * np.abs(want_a).max()
