"""-m gpu: the Winograd GEMM + output transform in one kernel (csrc/winograd.hip wino_gemm_out_kernel: conv1_2 / conv2_1-like channel
counts) against the two-launch path (flags bit 2 of ssd_op_conv2d_wino_fwd / _dgrad), through the C ABI, in all four forms of the output
transform: forward, forward + 2x2 pool with its record, data gradient (plain, accumulate + fp32 mask, accumulate + mask bits), data
gradient un-pooled through a record.
The fused kernel feeds the k slots of its 16x16x4 MFMAs in the order the GEMM kernel's 32x32x2 chain visits k, and the transform is the
same device code, so the assertion is BITWISE equality of values, pooled tensors and records."""
import zlib
import numpy as np
import pytest
import torch

from gpu_util import lib, check, dev, ptr, host, max_rel

pytestmark = pytest.mark.gpu
TWO = 4      # flags bit 2: GEMM and output transform as two launches

# (name, b, h, w, ci, co, the selection rule sends the forward / the data gradient to the fused kernel)
CASES = [
    ('conv1_2-like 64->64, 37x41: ragged last tile row and column, 220 tiles (not a multiple of 32)', 2, 37, 41, 64, 64, True, True),
    ('conv2_1-like 64->128, 30x26 b3', 3, 30, 26, 64, 128, True, True),
    ('128->64, 21x10 b2 (forward k = 128, data gradient n = 128)', 2, 21, 10, 128, 64, True, True),
    ('batch 1, odd 15x13 64->64', 1, 15, 13, 64, 64, True, True),
    ('batch 1, odd 75x75 64->128 (pool3-like ceil)', 1, 75, 75, 64, 128, True, True),
    ('exact tiles 16x32 64->64 b2 (64 tiles)', 2, 16, 32, 64, 64, True, True),
    ('one tile 3x2 64->64 b1', 1, 3, 2, 64, 64, True, True),
    ('conv2_2-like 128->128 12x9: two launches by rule', 2, 12, 9, 128, 128, False, False),
    ('32->64 9x11: k = 32 forward, n = 32 data gradient: two launches by rule', 2, 9, 11, 32, 64, False, False),
    ('64->256 10x10: n = 256 forward: two launches by rule', 1, 10, 10, 64, 256, False, False),
]


def raw(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint8 if t.dtype != torch.float32 else np.uint32)


def same(a, b, what):
    ra, rb = raw(a), raw(b)
    if not np.array_equal(ra, rb):
        if a.dtype == torch.float32:
            print(f'{what}: fused vs two-launch max-rel {max_rel(host(a), host(b)):.3e}, {np.count_nonzero(ra != rb)} of {ra.size} differ')
        raise AssertionError(f'{what}: the fused kernel and the two-launch path differ')


def m_floats_written(call, nws):
    """how many floats of a fresh workspace the forward call with these flags leaves untouched: the two paths differ by M, 36 T Co"""
    SENT = 0x7FC12345
    ws = torch.full((nws,), SENT, dtype=torch.int32, device='cuda')
    call(ws.view(torch.float32))
    torch.cuda.synchronize()
    return int((ws == SENT).sum().item())


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_fused_output_transform_bit_identical_to_two_launches(case):
    name, b, h, w, ci, co, fwd_fused, _ = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = np.maximum(rng.normal(0, 1, (b, h, w, ci)), 0).astype(np.float32)
    wt = (rng.normal(0, 1, (3, 3, ci, co)) / np.sqrt(9 * ci)).astype(np.float32)
    bias = rng.normal(0, 0.3, (co,)).astype(np.float32)
    dy = rng.normal(0, 1, (b, h, w, co)).astype(np.float32)
    geom = (b, h, w, ci, h, w, co, 3, 3, 1, 1, 1, 1)
    x_, w_, b_, dy_ = dev(x), dev(wt), dev(bias), dev(dy)
    ws_ = torch.empty((lib.ssd_op_conv2d_wino_ws_floats(*geom),), dtype=torch.float32, device='cuda')
    bits_ = torch.full((lib.ssd_op_conv2d_wino_bits_words(*geom),), -1, dtype=torch.int64, device='cuda')

    def out(shape, fill, dtype=torch.float32):
        return [torch.full(shape, fill, dtype=dtype, device='cuda') for _ in range(2)]

    # the rule: the fused forward leaves M's 36 T Co floats of the workspace untouched; where the rule says two launches the flag is a no-op
    y0 = torch.empty((b, h, w, co), dtype=torch.float32, device='cuda')
    left = [m_floats_written(lambda ws: check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), ptr(b_), ptr(y0), None, None, None, ptr(ws), fl,
                                                                          *geom, 1, None)), ws_.numel()) for fl in (0, TWO)]
    tiles = b * ((h + 3) // 4) * ((w + 3) // 4)
    assert left[0] - left[1] == (36 * tiles * co if fwd_fused else 0), f'{name}: {left}'

    # ---- forward: bias + relu, bias alone, no bias
    for relu, bp in ((1, ptr(b_)), (0, ptr(b_)), (1, None)):
        y = out((b, h, w, co), 7.0)
        check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), bp, ptr(y[0]), None, None, ptr(bits_), ptr(ws_), 0, *geom, relu, None))
        check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), bp, ptr(y[1]), None, None, None, ptr(ws_), 1 | TWO, *geom, relu, None))
        same(y[0], y[1], f'{name}: forward relu={relu} bias={bp is not None}')
    assert np.count_nonzero(host(y[0])) > 0.2 * y[0].numel()

    # ---- forward + pool: pooled tensor and record, and without a record
    ph, pw = (h + 1) // 2, (w + 1) // 2
    p, r = out((b, ph, pw, co), 9.0), out((b, ph, pw, co // 4), -2, torch.int16)
    check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), ptr(b_), None, ptr(p[0]), ptr(r[0]), None, ptr(ws_), 1, *geom, 1, None))
    check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), ptr(b_), None, ptr(p[1]), ptr(r[1]), None, ptr(ws_), 1 | TWO, *geom, 1, None))
    same(p[0], p[1], f'{name}: pooled tensor')
    same(r[0], r[1], f'{name}: pool record')
    p2 = torch.full((b, ph, pw, co), 9.0, dtype=torch.float32, device='cuda')
    check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), ptr(b_), None, ptr(p2), None, None, ptr(ws_), 1, *geom, 1, None))
    same(p2, p[1], f'{name}: pooled tensor without a record')

    # ---- data gradient: plain, accumulate + fp32 mask, accumulate + mask bits
    prev = rng.normal(0, 1, x.shape).astype(np.float32)
    g = out((b, h, w, ci), 3.0)
    check(lib.ssd_op_conv2d_wino_dgrad(ptr(dy_), ptr(w_), ptr(g[0]), None, None, 0, None, 0, 0, ptr(ws_), 1, *geom, None))
    check(lib.ssd_op_conv2d_wino_dgrad(ptr(dy_), ptr(w_), ptr(g[1]), None, None, 0, None, 0, 0, ptr(ws_), 1 | TWO, *geom, None))
    same(g[0], g[1], f'{name}: data gradient')
    assert np.count_nonzero(host(g[0])) > 0.9 * g[0].numel()
    for mb in (None, ptr(bits_)):
        g = [dev(prev), dev(prev)]
        check(lib.ssd_op_conv2d_wino_dgrad(ptr(dy_), ptr(w_), ptr(g[0]), ptr(x_), mb, 1, None, 0, 0, ptr(ws_), 1, *geom, None))
        check(lib.ssd_op_conv2d_wino_dgrad(ptr(dy_), ptr(w_), ptr(g[1]), ptr(x_), mb, 1, None, 0, 0, ptr(ws_), 1 | TWO, *geom, None))
        same(g[0], g[1], f'{name}: data gradient, accumulate + mask ({"bits" if mb else "fp32"})')
        zeros = np.count_nonzero(host(g[0]) == 0)
        assert 0.2 * g[0].numel() < zeros < 0.8 * g[0].numel()

    # ---- data gradient un-pooled through a record: this layer's input is the pool of a (uh x uw) tensor, both parities of each
    for uh, uw in ((2 * h, 2 * w), (2 * h - 1, 2 * w - 1)):
        src = dev(rng.normal(0, 1, (b, uh, uw, ci)).astype(np.float32))
        pooled = torch.empty((b, h, w, ci), dtype=torch.float32, device='cuda')
        rec = torch.full((b, h, w, ci // 4), -1, dtype=torch.int16, device='cuda')
        check(lib.ssd_op_maxpool_rec_fwd(ptr(src), ptr(pooled), ptr(rec), 0, b, uh, uw, ci, None))
        u = out((b, uh, uw, ci), 6.0)
        check(lib.ssd_op_conv2d_wino_dgrad(ptr(dy_), ptr(w_), ptr(u[0]), None, None, 0, ptr(rec), uh, uw, ptr(ws_), 1, *geom, None))
        check(lib.ssd_op_conv2d_wino_dgrad(ptr(dy_), ptr(w_), ptr(u[1]), None, None, 0, ptr(rec), uh, uw, ptr(ws_), 1 | TWO, *geom, None))
        same(u[0], u[1], f'{name}: un-pooled data gradient into {uh}x{uw}')
        assert np.count_nonzero(host(u[0])) > 0.02 * u[0].numel()
