"""-m gpu: the multibox loss kernels in isolation (csrc/ops.hip: heads_kernel<true> / heads_wide_kernel<true>, loss_sample_kernel<9|24|32>,
loss_grad_kernel<float|bf16_t>, sumsq_partial_kernel) through ssd_op_multibox_loss / ssd_op_multibox_loss_grad, against the two-stage
float64 oracle of tests/loss_ref.py (ssdvgg.py:375-580), on the inputs whole-model steps never produce: exact ties at the
hard-negative threshold, saturated rows (cross entropy exactly 0, threshold 0, the positives' zeros competing for slots),
k == neg_n, samples without positives, A from 64 to 32256, 1..127 classes, forward lanes, bf16 gradient buffers.

Bounds and where they come from:
  pos                      exact
  result, ce, sl1          stage A, scale-aware max-rel < 1e-3 (BASELINE.json north_star); the measured errors are printed
  sel                      stage B on the kernel's OWN ce: byte for byte (the assertion that catches a wrong tie rule)
  sample, losses           stage B on the kernel's own ce / sl1 in float64, 1e-5 relative: the fp32 tree sum of <= 32768 non-negative
                           terms at <= 32 per thread rounds by about (32 + log2 1024) * 2^-24 = 3e-6
  gradient                 stage B's formula on the kernel's own result and sample weight: 1e-6 of the largest magnitude (three
                           fp32 roundings); against the full float64 chain from the raw logits: 1e-3, tie-free cases only
  bf16 gradient            the bits of round-to-nearest-even of the fp32 run's gradient
Every case asserts the precondition of the path it is there for on the kernel's own ce before anything else."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import loss_ref as lr
from gpu_util import lib, check, dev, host, max_rel

pytestmark = pytest.mark.gpu
TOL = 1e-3              # result, ce, sl1 against stage A; the tie-free gradient against the full chain
TOL_SUMS = 1e-5         # sample, losses against stage B
TOL_GRAD = 1e-6         # gradient against stage B on the kernel's own result and weight
SENTINEL = 7.0

VGG300, VGG512 = lr.PRESET_LAYOUTS['vgg300'], lr.PRESET_LAYOUTS['vgg512']
BIG32 = ([64 * 64, 32 * 32, 16 * 16], [6, 6, 6])                     # A = 32256: loss_sample_kernel<32>
TINY = ([9, 4, 1], [4, 6, 4])                                        # A = 64: most threads hold no anchor
A1024 = ([128], [8])                                                 # every thread holds exactly one anchor; nj = 8
A1025 = ([128, 1], [8, 1])                                           # ... and thread 0 a second one
MID = ([361, 100, 25, 9, 1], [4, 6, 8, 6, 4])                        # A = 2302, ragged cell chunks, nj = 8 on one map


def _ints(v):
    return (C.c_int * len(v))(*v)


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class LossOp:
    """device buffers of one step of B samples on a layout, and the calls in lanes"""

    def __init__(self, hw, nj, num_classes, out, labels, bf16=False):
        self.lay = lay = lr.layout(hw, nj, num_classes)
        self.C, self.B, self.bf16 = num_classes, out.shape[0], bf16
        self.hw_, self.nj_ = _ints(lay['hw']), _ints(lay['nj'])
        a = C.c_int(); offs = (C.c_size_t * 6)()
        self.nbytes = lib.ssd_op_multibox_loss_ws_bytes(lay['nmaps'], self.hw_, self.nj_, self.B, offs, a)
        assert self.nbytes > 0 and a.value == lay['A'] == out.shape[1]
        self.offs = list(offs)
        self.ws = torch.zeros((self.nbytes,), dtype=torch.uint8, device='cuda')             # zero before first use
        self.heads = [dev(b) for b in lr.pack_heads(out, lay, pad_value=1e30)]              # pad columns: never consumed
        self.labels = dev(labels)
        self.result = torch.full(labels.shape, SENTINEL, dtype=torch.float32, device='cuda')
        self.grads = [torch.full(h.shape, SENTINEL, dtype=torch.bfloat16 if bf16 else torch.float32, device='cuda') for h in self.heads]

    def _lane(self, tensors, b_off):
        return [t[b_off * hw:] for t, hw in zip(tensors, self.lay['hw'])]

    def forward(self, b=None, b_off=0, bnorm=0.0, filters=None, wd=0.0):
        b = self.B if b is None else b
        lay = self.lay
        check(lib.ssd_op_multibox_loss(lay['nmaps'], self.hw_, self.nj_, self.C, _ptrs(self._lane(self.heads, b_off)),
                                       self.labels[b_off:].data_ptr(), self.result[b_off:].data_ptr(), self.ws.data_ptr(), b, b_off,
                                       self.B, bnorm, None if filters is None else filters.data_ptr(),
                                       0 if filters is None else filters.numel(), wd, None))

    def backward(self, b=None, b_off=0):
        b = self.B if b is None else b
        lay = self.lay
        check(lib.ssd_op_multibox_loss_grad(lay['nmaps'], self.hw_, self.nj_, self.C, _ptrs(self._lane(self.grads, b_off)),
                                            int(self.bf16), self.labels[b_off:].data_ptr(), self.result[b_off:].data_ptr(),
                                            self.ws.data_ptr(), b, b_off, self.B, None))

    def read(self):
        """every intermediate, on the host"""
        ws = host(self.ws)
        n = self.B * self.lay['A']
        o = self.offs

        def part(i, count, dt):
            return ws[o[i]:o[i] + count * np.dtype(dt).itemsize].view(dt).copy()
        r = dict(ce=part(0, n, np.float32), sl1=part(1, n, np.float32), pos=part(2, n, np.uint8), sel=part(3, n, np.uint8))
        r = {k: v.reshape(self.B, -1) for k, v in r.items()}
        r['sample'] = part(4, self.B * 4, np.float32).reshape(self.B, 4)
        r['losses'] = part(5, 4, np.float32)
        r['result'] = host(self.result)
        return r

    def read_grads(self):
        """(d_out [B,A,nv] in anchor order, pad columns per map) -- bf16 buffers as their uint16 bit patterns"""
        if self.bf16:
            bufs = [host(g.view(torch.int16)).view(np.uint16) for g in self.grads]
        else:
            bufs = [host(g) for g in self.grads]
        return lr.unpack_heads(bufs, self.lay, self.B)


def _close(got, want, tol):
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= tol * np.abs(want)).all())          # an exact 0 must come out as 0


def _rel(got, want):
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == want, 0.0, np.inf))
    return float(r.max())


def verify(name, op, out, labels, got, bnorm=0.0, sumsq=0.0, wd=0.0, tie_free=False, expect=None):
    """all assertions of one finished forward + backward; expect: per sample one of 'ties' (more entries equal T > 0 than are
    taken), 'zero' (T == 0 and positives take slots below zero-loss negatives), 'kmax' (k == neg_n), 'nopos', None"""
    C_ = op.C
    a = lr.stage_a(out, labels, C_)
    sb = lr.stage_b(got['ce'], got['pos'], got['sl1'], bnorm, sumsq, wd)
    gpos = got['pos'].astype(bool)
    neg = ~gpos
    # ---- preconditions first, on the kernel's own cross entropies and mask: a case that misses its path fails
    for s, e in enumerate(expect or []):
        what = f'{name}: sample {s} misses its precondition {e!r}: T {sb["T"][s]}, {sb["n_eq"][s]} equal, {sb["n_eq_taken"][s]} taken, k {sb["k"][s]}'
        for e1 in (e or '').split('+'):
            if e1 == 'ties':
                assert sb['T'][s] > 0 and sb['n_eq'][s] > sb['n_eq_taken'][s] > 0, what
            elif e1 == 'zero':
                assert sb['T'][s] == 0 and sb['n_eq'][s] > sb['n_eq_taken'][s] > 0, what
                zeros = np.flatnonzero(np.where(gpos[s], 0.0, got['ce'][s]) == 0)
                assert gpos[s][zeros[:sb['n_eq_taken'][s]]].any() and (neg[s][zeros] & ~sb['picked'][s][zeros]).any(), what
            elif e1 == 'kmax':
                assert sb['k'][s] == neg[s].sum() > 0, what
            elif e1 == 'nopos':
                assert not gpos[s].any() and gpos[:s].any() and gpos[s + 1:].any(), what
            else:
                assert e1 == '', e1
    assert np.array_equal(got['pos'].astype(bool), a['pos']), f'{name}: positive mask'
    if tie_free:        # nothing else equals the threshold: the selection does not depend on a tie rule (fp32 values of thousands of
        # continuous draws do collide somewhere; only a collision AT the threshold would matter)
        assert all(sb['n_eq'][s] == sb['n_eq_taken'][s] == 1 for s in range(op.B) if sb['k'][s]), f'{name}: the control ties at T: {sb["n_eq"]}'
    # ---- stage A
    e_r, e_c, e_s = max_rel(got['result'], a['result']), max_rel(got['ce'], a['ce']), max_rel(got['sl1'], a['sl1'])
    # ---- stage B on the kernel's own ce
    e_sample, e_loss = _rel(got['sample'], sb['sample']), _rel(got['losses'], sb['losses'])
    nsel_diff = int((got['sel'] != sb['sel']).sum())
    # ---- gradient
    d_out, pads = op.read_grads()
    e_g = e_full = float('nan')
    if not op.bf16:
        d_ref = lr.grad(got['result'], labels, got['sel'], got['pos'], got['sample'][:, 2], C_)
        e_g = float(np.abs(d_out - d_ref).max() / max(np.abs(d_ref).max(), 1e-300))
        if tie_free:
            e_full = max_rel(d_out, lr.full_chain(out, labels, C_, bnorm)[2])
    print(f'{name}: A {op.lay["A"]} C {C_} result {e_r:.2e} ce {e_c:.2e} sl1 {e_s:.2e} sample {e_sample:.2e} losses {e_loss:.2e} '
          f'grad {e_g:.2e} grad-vs-float64-chain {e_full:.2e} sel-diff {nsel_diff} '
          f'[T, equal, taken, k] {[(float(sb["T"][s]), int(sb["n_eq"][s]), int(sb["n_eq_taken"][s]), int(sb["k"][s])) for s in range(op.B)]}')
    assert e_r < TOL and e_c < TOL and e_s < TOL, f'{name}: result {e_r:.3e} ce {e_c:.3e} sl1 {e_s:.3e}'
    assert nsel_diff == 0, f'{name}: selection differs from the rule at {nsel_diff} anchors'
    assert np.array_equal(got['sample'][:, 3], sb['sample'][:, 3]), f'{name}: pos_n'
    assert _close(got['sample'], sb['sample'], TOL_SUMS), f'{name}: sample rel {e_sample:.3e}'
    assert _close(got['losses'], sb['losses'], TOL_SUMS), f'{name}: losses rel {e_loss:.3e}'
    for p in pads:
        assert not p.any(), f'{name}: gradient pad columns are not zero'
    if not op.bf16:
        assert e_g <= TOL_GRAD, f'{name}: gradient {e_g:.3e}'
        if tie_free:
            assert e_full < TOL, f'{name}: gradient against the float64 chain {e_full:.3e}'
    return sb, d_out


def run_case(name, layout, C_, pos_counts, expect=None, kind='palette', zero_frac=0.25, **kw):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    A = lr.layout(*layout, C_)['A']
    gen = lr.palette_batch if kind == 'palette' else lr.continuous_batch
    out, y = gen(rng, A, C_, pos_counts, zero_frac) if kind == 'palette' else gen(rng, A, C_, pos_counts)
    op = LossOp(*layout, C_, out, y)
    op.forward(**kw)
    op.backward()
    got = op.read()
    verify(name, op, out, y, got, bnorm=kw.get('bnorm', 0.0), tie_free=kind != 'palette', expect=expect)
    return op, out, y, got


# (name, layout, classes, positives per sample, expected path per sample)
CASES = [
    ('vgg300 three tie regimes around a sample without positives', VGG300, 20, [40, 1500, 0, 2900], ['ties', 'ties', 'nopos', 'zero+kmax']),
    ('vgg512 (template 24)', VGG512, 20, [60, 0, 3000, 7000], ['ties', 'nopos', 'ties', 'zero+kmax']),
    ('A 32256 (template 32)', BIG32, 20, [100, 5000, 9000], ['ties', 'ties', 'zero+kmax']),
    ('tiny A 64', TINY, 20, [3, 0, 20, 1], [None, 'nopos', 'kmax', None]),
    ('A 1024 nj 8', A1024, 20, [10, 100, 300], ['ties', 'ties', 'zero+kmax']),
    ('A 1025', A1025, 20, [10, 100, 300], ['ties', 'ties', 'zero+kmax']),
    ('1 class', MID, 1, [20, 300, 700], ['ties', 'ties', 'zero+kmax']),
    ('27 classes (last of heads_kernel)', MID, 27, [20, 300, 700], ['ties', 'ties', 'zero+kmax']),
    ('28 classes (first of heads_wide_kernel)', MID, 28, [20, 300, 700], ['ties', 'ties', 'zero+kmax']),
    ('80 classes', MID, 80, [20, 300, 700], ['ties', 'ties', 'zero+kmax']),
    ('127 classes', MID, 127, [20, 300, 700], ['ties', 'ties', 'zero+kmax']),
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_loss_palette(case):
    run_case(*case)


CONTROLS = [
    ('control vgg300', VGG300, 20, [40, 7, 300]),
    ('control 28 classes', MID, 28, [20, 1, 700]),
    ('control tiny', TINY, 3, [3, 20, 1]),
]


@pytest.mark.parametrize('case', CONTROLS, ids=[c[0] for c in CONTROLS])
def test_loss_tie_free_control(case):
    run_case(*case, kind='continuous')


def test_loss_every_negative_saturated():
    """every negative has a cross entropy of 0: the whole sample ties at T == 0 and the anchor index alone decides (a threshold
    of 0 always has a surplus: the positives' zeros are never all taken, k <= neg_n)"""
    op, out, y, got = run_case('all negatives saturated', MID, 20, [700, 300], ['zero+kmax', 'zero'], zero_frac=1.0)
    assert (got['ce'][~got['pos'].astype(bool)] == 0).all() and not got['sel'].all()


def _bits(got):
    return {k: got[k].view(np.uint8 if got[k].dtype == np.uint8 else np.uint32).copy() for k in ('sel', 'sample', 'losses', 'ce', 'sl1', 'pos')}


def test_loss_lanes_and_ticket():
    """one call over 5 samples == two calls (3 at 0, 2 at 3) of a step of 5, bit for bit; and again on the same workspace"""
    name = 'lanes vgg300'
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pos_counts = [40, 1500, 0, 2900, 500]
    out, y = lr.palette_batch(rng, 8732, 20, pos_counts)
    w = rng.normal(0, 0.05, (4100,)).astype(np.float32)
    sumsq = float((w.astype(np.float64) ** 2).sum())
    w_ = dev(w)
    one = LossOp(*VGG300, 20, out, y)
    one.forward(filters=w_, wd=0.0005)
    one.backward()
    g1 = one.read()
    verify(name, one, out, y, g1, sumsq=sumsq, wd=0.0005, expect=['ties', 'ties', 'nopos', 'zero+kmax', 'ties'])
    d1 = one.read_grads()[0]
    two = LossOp(*VGG300, 20, out, y)
    for rep in range(2):                     # the second round runs on the workspace the first one left: the ticket reset itself
        if rep:
            two.ws[two.offs[5]:two.offs[5] + 16].zero_()           # losses only: they must be written again
            for g in two.grads:
                g.fill_(SENTINEL)
        two.forward(b=3, b_off=0, filters=w_, wd=0.0005)
        if not rep:
            assert not host(two.ws[two.offs[5]:two.offs[5] + 16]).any(), 'losses written before the step completed'
        two.forward(b=2, b_off=3, wd=0.0005)
        two.backward(b=3, b_off=0)
        two.backward(b=2, b_off=3)
        g2 = two.read()
        b1, b2 = _bits(g1), _bits(g2)
        for k in b1:
            assert np.array_equal(b1[k], b2[k]), f'{name}: {k} differs between one call and two lanes (round {rep})'
        assert np.array_equal(g1['result'].view(np.uint32), g2['result'].view(np.uint32))
        assert np.array_equal(d1.view(np.uint32), two.read_grads()[0].view(np.uint32)), f'{name}: gradient differs (round {rep})'
    # the same single call again on its own workspace
    one.forward(filters=w_, wd=0.0005)
    b1, b3 = _bits(g1), _bits(one.read())
    for k in b1:
        assert np.array_equal(b1[k], b3[k]), f'{name}: {k} differs on the second call'


def test_loss_bnorm():
    """bnorm = 2.5 against the default (the step's own 4): sums and selection keep their bits, weight and losses rescale"""
    name = 'bnorm vgg300'
    op, out, y, g0 = run_case(name, VGG300, 20, [40, 1500, 0, 2900], ['ties', 'ties', 'nopos', 'zero+kmax'])
    d0 = op.read_grads()[0]
    op2 = LossOp(*VGG300, 20, out, y)
    op2.forward(bnorm=2.5)
    op2.backward()
    g1 = op2.read()
    sb, d1 = verify(name + ' 2.5', op2, out, y, g1, bnorm=2.5)
    for k in ('sel', 'ce'):
        assert np.array_equal(g0[k], g1[k])
    assert np.array_equal(g0['sample'][:, [0, 1, 3]].view(np.uint32), g1['sample'][:, [0, 1, 3]].view(np.uint32))
    # fp32 roundings apart: the weight is one division, a loss one division, a gradient value the weight times a difference
    f64 = lambda v: np.asarray(v, np.float64)
    assert _close(f64(g1['sample'][:, 2]) * 2.5, f64(g0['sample'][:, 2]) * 4, 3e-7)
    assert _close(f64(g1['losses'][1:3]) * 2.5, f64(g0['losses'][1:3]) * 4, 3e-7)
    assert max_rel(f64(d1) * 2.5, f64(d0) * 4) < 3e-7


def bf16_rne_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


@pytest.mark.parametrize('layout,C_', [(VGG300, 20), (MID, 80)], ids=['vgg300', 'mid 80 classes'])
def test_loss_grad_bf16(layout, C_):
    """bf16 gradient buffers hold round-to-nearest-even of the fp32 run's gradient, pad columns zero in both"""
    name = f'bf16 grads {C_}'
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    A = lr.layout(*layout, C_)['A']
    pos_counts = [A // 200, 0, A // 6, A // 3]
    out, y = lr.palette_batch(rng, A, C_, pos_counts)
    f = LossOp(*layout, C_, out, y)
    f.forward(); f.backward()
    gf = f.read()
    _, d32 = verify(name + ' (fp32 run)', f, out, y, gf, expect=['ties', 'nopos', 'ties', 'zero+kmax'])
    h = LossOp(*layout, C_, out, y, bf16=True)
    h.forward(); h.backward()
    gh = h.read()
    verify(name, h, out, y, gh)
    d16, pads = h.read_grads()
    assert all(not p.any() for p in pads) and d16.dtype == np.uint16
    assert np.count_nonzero(d32) > 1000
    assert np.array_equal(d16, bf16_rne_bits(d32)), f'{name}: {(d16 != bf16_rne_bits(d32)).sum()} values differ from RNE'


@pytest.mark.parametrize('n', [4, 1024 * 4 + 4, 26_000_000], ids=['4', '4100', '26M'])
def test_loss_l2_term(n):
    """sumsq_partial_kernel + the last workgroup's float64 sum of the partials, against float64"""
    name = f'l2 term over {n} floats'
    rng = np.random.default_rng(n)
    w = rng.normal(0, 0.05, (n,)).astype(np.float32)
    sumsq = float(np.square(w, dtype=np.float64).sum())
    out, y = lr.palette_batch(rng, 64, 20, [3, 20])
    op = LossOp(*TINY, 20, out, y)
    op.forward(filters=dev(w), wd=0.0005)
    op.backward()
    got = op.read()
    sb, _ = verify(name, op, out, y, got, sumsq=sumsq, wd=0.0005)
    assert sb['losses'][3] > 0 and _close(got['losses'][3], 0.0005 * 0.5 * sumsq, TOL_SUMS)
    # a call without filters keeps the partial sums; a fresh workspace has none
    op.forward(wd=0.0005)
    assert op.read()['losses'][3] == got['losses'][3]
    op2 = LossOp(*TINY, 20, out, y)
    op2.forward(wd=0.0005)
    assert op2.read()['losses'][3] == 0.0
