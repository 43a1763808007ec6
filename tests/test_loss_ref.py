"""CPU: tests/loss_ref.py, the two-stage float64 oracle of the multibox loss kernels, against oracle.ssdvgg_ref.loss_numpy on
tie-free input; and why the op-level tests (test_gpu_loss.py) judge the selection on the kernel's own fp32 cross entropies:
on palette inputs with saturated rows the float64 oracle picks a different set than the fp32 rule."""
import ctypes as C

import numpy as np

import loss_ref as lr
from oracle import ssdvgg_ref as ref


def test_two_stages_agree_with_loss_numpy_on_tie_free_input():
    rng = np.random.default_rng(11)
    for C_, A, pos_counts in ((20, 700, [5, 0, 120, 400]), (3, 64, [1, 20, 63])):
        out, y = lr.continuous_batch(rng, A, C_, pos_counts)
        a, b, d = lr.full_chain(out, y, C_)
        assert len(np.unique(a['ce'])) == a['ce'].size                      # tie-free
        conf, loc, d_ref, selmask = ref.loss_numpy(out, y, C_)
        assert abs(b['losses'][2] - conf) <= 1e-13 * abs(conf) and abs(b['losses'][1] - loc) <= 1e-13 * abs(loc)
        assert np.array_equal(b['sel'].astype(bool), a['pos'] | selmask)
        assert np.array_equal(b['picked'] & ~a['pos'], selmask)
        assert np.abs(d - d_ref).max() <= 1e-15 + 1e-13 * np.abs(d_ref).max()
        assert list(b['k']) == [min(A - p, 3 * p) for p in pos_counts]
        assert np.array_equal(b['sample'][:, 3], pos_counts) and not b['sample'][np.array(pos_counts) == 0].any()
        # bnorm only rescales: the weight and the two means
        b2 = lr.stage_b(a['ce'], a['pos'], a['sl1'], bnorm=2.5, sumsq=8.0, weight_decay=0.5)
        B = len(pos_counts)
        assert np.allclose(b2['sample'][:, 2] * 2.5, b['sample'][:, 2] * B, rtol=1e-15)
        assert np.allclose(b2['losses'][1:3] * 2.5, b['losses'][1:3] * B, rtol=1e-14) and b2['losses'][3] == 2.0
        assert np.isclose(b2['losses'][0], b2['losses'][1:].sum(), rtol=1e-15)


def test_pack_heads_round_trip_and_layout():
    lay = lr.layout(*lr.PRESET_LAYOUTS['vgg300'], 20)
    assert lay['A'] == 8732 and lay['ld'] == [104, 152, 152, 152, 104, 104] and lay['off'][1] == 5776
    assert lr.layout(*lr.PRESET_LAYOUTS['vgg512'], 20)['A'] == 24564
    lay = lr.layout([9, 4, 1], [4, 6, 8], 3)
    rng = np.random.default_rng(0)
    out = rng.normal(0, 1, (2, lay['A'], lay['nv'])).astype(np.float32)
    bufs = lr.pack_heads(out, lay, pad_value=7.0)
    assert [b.shape for b in bufs] == [(18, 32), (8, 48), (2, 64)]
    # anchor (map 1, type 2, cell 3) of image 1: row 1 * 4 + 3, columns 2 * 8 ..
    assert np.array_equal(bufs[1][7, 16:24], out[1, lay['off'][1] + 2 * 4 + 3])
    back, pads = lr.unpack_heads(bufs, lay, 2)
    assert np.array_equal(back, out) and all((p == 7.0).all() for p in pads) and pads[2].shape == (2, 0)


def test_library_layout_matches_restated_layout():
    """the C ABI's workspace query reports the anchor count of the layout the entry builds (host only, no GPU)"""
    from ssd_tensorflow_amd._lib import lib, last_error
    for hw, nj in (lr.PRESET_LAYOUTS['vgg300'], lr.PRESET_LAYOUTS['vgg512'], ([9, 4, 1], [4, 6, 8])):
        n = len(hw)
        a = C.c_int(); offs = (C.c_size_t * 6)()
        nbytes = lib.ssd_op_multibox_loss_ws_bytes(n, (C.c_int * n)(*hw), (C.c_int * n)(*nj), 5, offs, a)
        A = lr.layout(hw, nj, 20)['A']
        assert a.value == A and nbytes > 0
        o = list(offs)
        assert o[0] == 0 and o[1] == 5 * A * 4 and o[2] == 2 * o[1] and o[3] - o[2] >= 5 * A and o[4] - o[3] >= 5 * A
        assert o[5] - o[4] >= 5 * 16 and o[5] + 16 <= nbytes and all(v % 16 == 0 for v in o)
    assert lib.ssd_op_multibox_loss_ws_bytes(9, (C.c_int * 9)(*[1] * 9), (C.c_int * 9)(*[1] * 9), 1, None, None) == 0
    assert 'feature maps' in last_error()


def test_float64_oracle_cannot_judge_the_selection_on_saturated_input():
    """3 samples of 8732 anchors, rows from a 12-row palette, 40 / 1500 / 2900 positives (seed fixed).
    Samples 0 and 1: more entries equal the threshold T > 0 than are taken.  Sample 2: k == neg_n and T == 0, the zeros of
    the positives compete with the zero-loss negatives.  There loss_numpy, whose float64 cross entropy of a saturated row is
    ~1e-13 and not 0, picks a different set than the rule applied to fp32 cross entropies."""
    rng = np.random.default_rng(20260)
    A, C_, pos_counts = 8732, 20, [40, 1500, 2900]
    out, y = lr.palette_batch(rng, A, C_, pos_counts)
    ce32 = lr.ce_fp32(out, y, C_)
    a = lr.stage_a(out, y, C_)
    neg = ~a['pos']
    # fp32 saturates all three kinds of rows to 0; float64 keeps the row that leads by 30 at ~1e-13 (the others are 0 there too)
    sat64 = a['ce'][neg][ce32[neg] == 0]
    assert (ce32[neg] == 0).sum() > 1000 and sat64.max() < 1e-11 and ((sat64 > 0).sum() > 300) and (sat64 == 0).sum() > 300
    b32 = lr.stage_b(ce32, a['pos'], a['sl1'])
    assert list(b32['k']) == [120, 4500, A - 2900]
    for s in (0, 1):
        assert b32['T'][s] > 0 and b32['n_eq'][s] > b32['n_eq_taken'][s] > 0, (s, b32['T'][s], b32['n_eq'][s], b32['n_eq_taken'][s])
    assert b32['T'][2] == 0 and b32['k'][2] == neg[2].sum() and b32['n_eq'][2] > b32['n_eq_taken'][2] > 0
    zeros = np.flatnonzero(np.where(a['pos'][2], 0.0, ce32[2]) == 0)
    taken = zeros[:b32['n_eq_taken'][2]]
    assert a['pos'][2][taken].any() and (neg[2][zeros] & ~b32['picked'][2][zeros]).any()      # positives took slots of negatives
    print('entries equal to T / taken:', [(int(b32['n_eq'][s]), int(b32['n_eq_taken'][s])) for s in range(3)])
    _, _, _, selmask = ref.loss_numpy(out, y, C_)
    want = b32['picked'] & neg
    assert np.array_equal(selmask[0], want[0]) and np.array_equal(selmask[1], want[1])          # exact ties survive float64
    ndiff = int((selmask[2] != want[2]).sum())
    print('sample 2: the float64 oracle differs from the fp32 rule at', ndiff, 'anchors')
    assert ndiff > 0
    # ... while the confidence loss hardly moves: the 1e-3 bar of the model tests cannot see a selection that is off
    conf64 = ref.loss_numpy(out, y, C_)[0]
    assert abs(b32['losses'][2] - conf64) < 1e-6 * conf64
