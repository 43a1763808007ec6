"""-m gpu: the launch geometry of the Winograd input transform and of the weight gradient's reduce (csrc/winograd.hip: wino_in_kernel's
workgroups as one contiguous run of the tile raster per XCD, wino_wgrad_reduce36_kernel's one thread per position) against the reference
geometry (flags bit 3 of ssd_op_conv2d_wino_fwd / _dgrad / _wgrad: raster-order workgroups, one thread per (ci, 4 co)), through the C ABI.
Only which thread handles which (tile, quad) or which position changes: every load, sum and store is the same expression in the same
order, so the assertion is BITWISE equality of y, pooled y and record, relu bits, dx, dw, dbias -- and of the whole workspace, which
holds the transforms themselves.  One case also goes against the CPU oracle at test_gpu_winograd.py's bound: equal is not yet right."""
import zlib
import numpy as np
import pytest
import torch

from gpu_util import lib, check, dev, ptr, host, max_rel
from test_gpu_kernels import oracle_conv

pytestmark = pytest.mark.gpu
REF = 8      # flags bit 3: the reference geometry
TOL = 1e-3   # test_gpu_winograd.py's (BASELINE.json north_star)

# (name, b, h, w, ci, co, dilation): the smallest shapes that reach each edge of the mapping.  A workgroup of the input transform is
# 256 threads = 256 / (C / 4) tiles; the reduce's is 16 (ci, 4 co) elements x 36 positions, after cdiv(co / 4, 32) bias workgroups.
CASES = [
    ('ragged tile grid 10x7 32->32 b2: 12 tiles, 1 workgroup (fewer than 8)', 2, 10, 7, 32, 32, 1),
    ('9x13 64->64 b3: 36 tiles, 3 workgroups (not a multiple of 8), T c4n = 576 (not of 256)', 3, 9, 13, 64, 64, 1),
    ('one tile per image 4x4 64->128 b1', 1, 4, 4, 64, 128, 1),
    ('head padding 38x38 128->104 b2: the data gradient k 104 -> 128', 2, 38, 38, 128, 104, 1),
    ('head padding 19x19 64->152 b2: the data gradient k 152 -> 160', 2, 19, 19, 64, 152, 1),
    ('dilation 6 19x19 64->64 b2: every residue class one tile', 2, 19, 19, 64, 64, 6),
    ('dilation 2 12x12 64->64 b2', 2, 12, 12, 64, 64, 2),
    ('21x21 512->64 b2: 2 tiles per workgroup', 2, 21, 21, 512, 64, 1),
    ('8x8 1024->32 b1: 1 tile per workgroup, wider than the tile row', 1, 8, 8, 1024, 32, 1),
]


def raw(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint8 if t.dtype != torch.float32 else np.uint32)


def same(a, b, what):
    ra, rb = raw(a), raw(b)
    if not np.array_equal(ra, rb):
        raise AssertionError(f'{what}: the two geometries differ in {np.count_nonzero(ra != rb)} of {ra.size} words')


def tiles_1d(n, dil):
    return dil * -(-(-(-n // dil)) // 4)


def wgrad_splits(geom):
    """slabs the weight-gradient GEMM of this shape writes (winograd.hip tn_splits, then wino_wgrad's rounding), from the workspace size"""
    b, h, w, ci, _, _, co, _, _, _, dil, _, _ = geom
    cop = (co + 31) // 32 * 32
    tiles = b * tiles_1d(h, dil) * tiles_1d(w, dil)
    fixed = 2 * 36 * ci * cop + 36 * tiles * (ci + max(ci, cop) + 2 * cop)
    planned, rest = divmod(lib.ssd_op_conv2d_wino_ws_floats(*geom) - fixed, 36 * ci * co + 16 * co)
    assert rest == 0 and planned >= 1
    chunk = -(-(-(-tiles // planned)) // 32) * 32
    return -(-tiles // chunk)


def both(shape, fill, dtype=torch.float32):
    return [torch.full(shape, fill, dtype=dtype, device='cuda') for _ in range(2)]


def run_both_geometries(name, b, h, w, ci, co, dil, pools=True):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = np.maximum(rng.normal(0, 1, (b, h, w, ci)), 0).astype(np.float32)
    wt = (rng.normal(0, 1, (3, 3, ci, co)) / np.sqrt(9 * ci)).astype(np.float32)
    bias = rng.normal(0, 0.3, (co,)).astype(np.float32)
    dy = rng.normal(0, 1, (b, h, w, co)).astype(np.float32)
    prev = rng.normal(0, 1, x.shape).astype(np.float32)
    geom = (b, h, w, ci, h, w, co, 3, 3, 1, dil, dil, dil)
    x_, w_, b_, dy_ = dev(x), dev(wt), dev(bias), dev(dy)
    nws = lib.ssd_op_conv2d_wino_ws_floats(*geom)
    assert nws > 0
    # [0]: the default geometry, [1]: the reference; each with a workspace of its own, so every transform is its own geometry's
    ws = both((nws,), 0.0)
    fl = (0, REF)

    # ---- forward with relu bits
    y = both((b, h, w, co), 7.0)
    bits = both((lib.ssd_op_conv2d_wino_bits_words(*geom),), -1, torch.int64)
    for g in (0, 1):
        check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), ptr(b_), ptr(y[g]), None, None, ptr(bits[g]), ptr(ws[g]), fl[g], *geom, 1, None))
    same(y[0], y[1], f'{name}: forward')
    same(bits[0], bits[1], f'{name}: relu bits')
    same(ws[0], ws[1], f'{name}: workspace after the forward (V, M)')
    assert np.count_nonzero(host(y[0])) > 0.2 * y[0].numel()

    # ---- forward + pool: pooled tensor and record
    if pools and dil == 1:
        ph, pw = (h + 1) // 2, (w + 1) // 2
        p, r = both((b, ph, pw, co), 9.0), both((b, ph, pw, co // 4), -2, torch.int16)
        for g in (0, 1):
            check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), ptr(b_), None, ptr(p[g]), ptr(r[g]), None, ptr(ws[g]), 1 | fl[g], *geom, 1, None))
        same(p[0], p[1], f'{name}: pooled tensor')
        same(r[0], r[1], f'{name}: pool record')

    # ---- weight gradient (the call transforms x and dy itself), with weight decay
    gw, gb = both((3, 3, ci, co), 7.0), both((co,), 7.0)
    for g in (0, 1):
        check(lib.ssd_op_conv2d_wino_wgrad(ptr(x_), ptr(dy_), ptr(gw[g]), ptr(gb[g]), ptr(w_), 0.0005, ptr(ws[g]), 1 | fl[g], *geom, None))
    same(gw[0], gw[1], f'{name}: dw')
    same(gb[0], gb[1], f'{name}: dbias')
    same(ws[0], ws[1], f'{name}: workspace after the weight gradient (V, Ya, slabs)')
    assert np.count_nonzero(host(gw[0])) > 0.9 * gw[0].numel() and np.count_nonzero(host(gb[0])) == co

    # ---- data gradient: plain, accumulate + fp32 mask, accumulate + mask bits
    gx = both((b, h, w, ci), 3.0)
    for g in (0, 1):
        check(lib.ssd_op_conv2d_wino_dgrad(ptr(dy_), ptr(w_), ptr(gx[g]), None, None, 0, None, 0, 0, ptr(ws[g]), 1 | fl[g], *geom, None))
    same(gx[0], gx[1], f'{name}: data gradient')
    same(ws[0], ws[1], f'{name}: workspace after the data gradient (Yt, M)')
    assert np.count_nonzero(host(gx[0])) > 0.9 * gx[0].numel()
    for mb in (None, bits):
        ga = [dev(prev), dev(prev)]
        for g in (0, 1):
            check(lib.ssd_op_conv2d_wino_dgrad(ptr(dy_), ptr(w_), ptr(ga[g]), ptr(x_), ptr(mb[g]) if mb else None, 1, None, 0, 0, ptr(ws[g]),
                                               1 | fl[g], *geom, None))
        same(ga[0], ga[1], f'{name}: data gradient, accumulate + mask ({"bits" if mb else "fp32"})')
        zeros = np.count_nonzero(host(ga[0]) == 0)
        assert 0.2 * ga[0].numel() < zeros < 0.8 * ga[0].numel()

    # ---- data gradient un-pooled through a record
    if pools and dil == 1:
        uh, uw = 2 * h - 1, 2 * w
        src = dev(rng.normal(0, 1, (b, uh, uw, ci)).astype(np.float32))
        pooled = torch.empty((b, h, w, ci), dtype=torch.float32, device='cuda')
        rec = torch.full((b, h, w, ci // 4), -1, dtype=torch.int16, device='cuda')
        check(lib.ssd_op_maxpool_rec_fwd(ptr(src), ptr(pooled), ptr(rec), 0, b, uh, uw, ci, None))
        u = both((b, uh, uw, ci), 6.0)
        for g in (0, 1):
            check(lib.ssd_op_conv2d_wino_dgrad(ptr(dy_), ptr(w_), ptr(u[g]), None, None, 0, ptr(rec), uh, uw, ptr(ws[g]), 1 | fl[g], *geom, None))
        same(u[0], u[1], f'{name}: un-pooled data gradient')
        assert np.count_nonzero(host(u[0])) > 0.02 * u[0].numel()
    return geom


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_geometry_bit_identical_to_the_reference(case):
    run_both_geometries(*case)


def test_wgrad_reduce_more_than_four_slabs():
    # 64 -> 64 at 76x76, batch 4: 1444 tiles; the cost model splits them into more than the reduce's 4-slab unroll
    geom = (4, 76, 76, 64, 76, 76, 64, 3, 3, 1, 1, 1, 1)
    assert wgrad_splits(geom) > 4, wgrad_splits(geom)
    run_both_geometries('wgrad split 76x76 64->64 b4', 4, 76, 76, 64, 64, 1, pools=False)


def test_wgrad_reduce_one_slab():
    geom = (3, 9, 13, 64, 9, 13, 64, 3, 3, 1, 1, 1, 1)
    assert wgrad_splits(geom) == 1
    # (its bits against the reference: the 9x13 case above)
    assert wgrad_splits((2, 21, 21, 512, 21, 21, 64, 3, 3, 1, 1, 1, 1)) == 1


def test_default_geometry_against_the_cpu_oracle():
    name, b, h, w, ci, co = 'oracle 9x13 64->64 b3', 3, 9, 13, 64, 64
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = np.maximum(rng.normal(0, 1, (b, h, w, ci)), 0).astype(np.float32)
    wt = (rng.normal(0, 1, (3, 3, ci, co)) / np.sqrt(9 * ci)).astype(np.float32)
    bias = rng.normal(0, 0.1, (co,)).astype(np.float32)
    dy = rng.normal(0, 1, (b, h, w, co)).astype(np.float32)
    xt, wtt, bt, pre, y_ref = oracle_conv(x, wt, bias, 1, 1, 'SAME', True)
    gpre = torch.tensor(dy).permute(0, 3, 1, 2) * (pre > 0).float()
    pre.backward(gpre)
    dx_ref = xt.grad.permute(0, 2, 3, 1).numpy()
    dw_ref, db_ref = wtt.grad.numpy(), bt.grad.numpy()

    geom = (b, h, w, ci, h, w, co, 3, 3, 1, 1, 1, 1)
    ws_ = torch.zeros((lib.ssd_op_conv2d_wino_ws_floats(*geom),), dtype=torch.float32, device='cuda')
    x_, w_, b_, gdy_ = dev(x), dev(wt), dev(bias), dev(gpre.permute(0, 2, 3, 1).contiguous().numpy())
    y_ = torch.full((b, h, w, co), 7.0, dtype=torch.float32, device='cuda')
    check(lib.ssd_op_conv2d_wino_fwd(ptr(x_), ptr(w_), ptr(b_), ptr(y_), None, None, None, ptr(ws_), 0, *geom, 1, None))
    e_f = max_rel(host(y_), y_ref.detach().permute(0, 2, 3, 1).numpy())
    wd = 0.0005
    gw_ = torch.full((3, 3, ci, co), 7.0, dtype=torch.float32, device='cuda')
    gb_ = torch.full((co,), 7.0, dtype=torch.float32, device='cuda')
    check(lib.ssd_op_conv2d_wino_wgrad(ptr(x_), ptr(gdy_), ptr(gw_), ptr(gb_), ptr(w_), wd, ptr(ws_), 1, *geom, None))
    e_w, e_b = max_rel(host(gw_), dw_ref + wd * wt), max_rel(host(gb_), db_ref)
    gx_ = torch.full((b, h, w, ci), 3.0, dtype=torch.float32, device='cuda')
    check(lib.ssd_op_conv2d_wino_dgrad(ptr(gdy_), ptr(w_), ptr(gx_), None, None, 0, None, 0, 0, ptr(ws_), 1, *geom, None))
    e_d = max_rel(host(gx_), dx_ref)
    print(f'{name}: fwd {e_f:.2e} wgrad {e_w:.2e} bias {e_b:.2e} dgrad {e_d:.2e}')
    assert e_f < TOL and e_w < TOL and e_b < TOL and e_d < TOL
