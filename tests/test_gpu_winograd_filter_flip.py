"""-m gpu: the data gradients' filter transform U' through LDS (csrc/winograd.hip wino_filter_flip_lds_kernel: a 32 ci x 32 co tile of the
nine taps per workgroup, whole lines of w in and of U' out) against the kernel it replaced, kept behind flags bit 0 of
ssd_op_wino_filter_flip_plan (lanes along ci, no staging).  The same g6 arithmetic on the same values: BITWISE equality, over one plan of
three layers as a step launches them -- 32 x 4 (one ragged tile), 64 x 100 (a ragged last co tile; rows 100 ... 127 of every position are
the caller's zeros and stay so), 128 x 64 (eight full tiles).  One layer is also checked against G g' G^T in float64."""
import ctypes as C
import numpy as np
import pytest
import torch

from gpu_util import lib, check, dev

pytestmark = pytest.mark.gpu
LAYERS = [(32, 4), (64, 100), (128, 64)]      # (ci, co)
GUARD, PATTERN = 64, 0x7FC0BEEF


def run(ws, flags):
    """-> per layer U' as uint32 [36][kpad(co)][ci]"""
    n = len(LAYERS)
    bufs = []
    for ci, co in LAYERS:
        cop = (co + 31) // 32 * 32
        t = torch.full((GUARD + 36 * cop * ci + GUARD,), PATTERN, dtype=torch.int32, device='cuda')
        t[GUARD:-GUARD] = 0      # (the step clears U' once: the pad rows)
        bufs.append(t)
    wp = (C.c_void_p * n)(*[w.data_ptr() for w in ws])
    up = (C.c_void_p * n)(*[b.data_ptr() + 4 * GUARD for b in bufs])
    cis = (C.c_int * n)(*[ci for ci, _ in LAYERS])
    cos = (C.c_int * n)(*[co for _, co in LAYERS])
    check(lib.ssd_op_wino_filter_flip_plan(wp, up, cis, cos, n, flags, None))
    torch.cuda.synchronize()
    out = []
    for (ci, co), b in zip(LAYERS, bufs):
        raw = b.cpu().numpy().view(np.uint32)
        assert np.all(raw[:GUARD] == PATTERN) and np.all(raw[-GUARD:] == PATTERN), f'{ci}x{co}: guard words overwritten (flags {flags})'
        out.append(raw[GUARD:-GUARD].reshape(36, (co + 31) // 32 * 32, ci))
    return out


def test_filter_flip_lds_bit_identical_to_the_lanes_along_ci_kernel():
    rng = np.random.default_rng(41)
    w = [rng.normal(0, 1, (3, 3, ci, co)).astype(np.float32) for ci, co in LAYERS]
    ws = [dev(x) for x in w]
    lds, old = run(ws, 0), run(ws, 1)
    for (ci, co), a, b in zip(LAYERS, lds, old):
        assert np.array_equal(a, b), f'{ci}x{co}: U\' differs in {np.count_nonzero(a != b)} of {a.size} words'
        for v in (a, b):
            assert not np.any(v[:, co:, :]), f'{ci}x{co}: pad rows written'
            assert np.count_nonzero(v[:, :co, :]) == 36 * co * ci
    # equal is not yet right: U'[(k, l)][co][ci] = (G g' G^T)_(k, l) with g' the filter rotated by 180 degrees
    G = np.array([[64 / 81, 0, 0], [-128 / 243, -32 / 81, -8 / 27], [-128 / 243, 32 / 81, -8 / 27],
                  [32 / 243, 16 / 81, 8 / 27], [32 / 243, -16 / 81, 8 / 27], [0, 0, 1]])
    ci, co = LAYERS[1]
    g = w[1][::-1, ::-1].astype(np.float64)                                  # [3][3][ci][co]
    want = np.einsum('ka,abio,lb->kloi', G, g, G).reshape(36, co, ci)
    got = lds[1].view(np.float32)[:, :co, :]
    assert np.abs(got - want).max() < 1e-5 * np.abs(want).max()
