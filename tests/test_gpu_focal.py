"""-m gpu: the focal-loss kernels in isolation (csrc/ops.hip: focal_sample_kernel<9|24|32>, focal_grad_kernel<float|bf16_t, narrow|wide>
behind the unchanged heads_kernel<true> / heads_wide_kernel<true>) through ssd_op_multibox_loss_ex / ssd_op_multibox_loss_grad_ex,
against the float64 oracle of tests/focal_ref.py, on the inputs of tests/focal_cases.py: saturated rows (cross entropy exactly 0),
nearly saturated ones (1e-6), samples without positives and with nothing else, A from 64 to 32256, 1..127 classes, gamma 0, 0.5, 1,
2, 5, forward lanes, bf16 gradient buffers.

Bounds and where they come from (eps = 2^-24, one fp32 rounding; the device expm1f, expf and powf are documented at 1 ulp = 2 eps
in the HIP math API's accuracy table):
  pos, result, ce, sl1     bit for bit what a mining call leaves on the same input (the head kernels are shared)
  sel                      all ones
  sample, losses           stage F on the kernel's OWN ce / sl1 in float64.  A term alpha_t * q^gamma * ce: q = -expm1f(-ce) 2 eps,
                           raised to gamma (gamma * 2 eps; powf another 2 eps, q * q one, gamma 0 and 1 none), 1 - alpha and the two
                           products 3 eps: (gamma + 1) * 2 eps + 3 eps <= 5.4e-7 at gamma <= 2, 9e-7 at gamma 5.  All terms are
                           >= 0, so the sum inherits that; the tree sum of <= 32768 of them (32 per thread, 6 shuffle levels, 16
                           waves in turn) adds 54 eps = 3.2e-6, the divisions and the sum over samples 6 eps:
                               BOUND_SUMS(gamma) = 3.2e-6 + (2 gamma + 11) eps  <= 4.5e-6, under the cap of 1e-5 (TOL_SUMS)
  gradient                 focal_ref.grad on the kernel's own result, ce and sample weight, relative to the largest magnitude.
                           kappa = alpha_t * q^gamma * (1 + gamma * p * ce / q): q^gamma as above (gamma + 1) * 2 eps; the bracket's
                           second term p = expf(-ce) 2 eps, q 2 eps, the division and two products 3 eps, weighing < 1 in the sum,
                           whose own rounding is 1 eps: 8 eps; alpha_t and its two products 3 eps, times the weight, the difference
                           softmax - label and the last product 3 eps:
                               BOUND_GRAD(gamma) = (2 gamma + 16) eps  <= 1.6e-6, under the cap of 1e-5
                           against the full float64 chain from the raw logits: 1e-3 (BASELINE.json north_star)
  bf16 gradient            the bits of round-to-nearest-even of the fp32 run's gradient
  finite, pad columns 0    everywhere
Per-anchor focal terms are never compared relatively (at gamma 5 they reach subnormals): sums only.  The measured errors are
printed by every case."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import focal_cases as fc
import focal_ref as fr
import loss_ref as lr
from gpu_util import lib, check, dev, host, max_rel
from ssd_tensorflow_amd.ssdvgg import LossConfig

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
TOL = 1e-3              # the gradient against the full float64 chain
CAP = 1e-5              # the issue's cap on both derived bounds
SENTINEL = 7.0


def bound_sums(gamma):
    return min(CAP, 3.2e-6 + (2 * gamma + 11) * EPS)


def bound_grad(gamma):
    return min(CAP, (2 * gamma + 16) * EPS)


def _ints(v):
    return (C.c_int * len(v))(*v)


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class LossOp:
    """device buffers of one step of B samples on a layout, and the calls in lanes (test_gpu_loss.py's helper, restated, with the
    configuration: cfg None = the entry points without one, otherwise the _ex ones)"""

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

    def forward(self, cfg=None, b=None, b_off=0, bnorm=0.0, filters=None, wd=0.0):
        b = self.B if b is None else b
        lay = self.lay
        args = (lay['nmaps'], self.hw_, self.nj_, self.C, _ptrs(self._lane(self.heads, b_off)), self.labels[b_off:].data_ptr(),
                self.result[b_off:].data_ptr(), self.ws.data_ptr(), b, b_off, self.B, bnorm,
                None if filters is None else filters.data_ptr(), 0 if filters is None else filters.numel(), wd)
        if cfg is None:
            check(lib.ssd_op_multibox_loss(*args, None))
        else:
            check(lib.ssd_op_multibox_loss_ex(*args, C.byref(cfg), None))

    def backward(self, cfg=None, b=None, b_off=0):
        b = self.B if b is None else b
        lay = self.lay
        args = (lay['nmaps'], self.hw_, self.nj_, self.C, _ptrs(self._lane(self.grads, b_off)), int(self.bf16),
                self.labels[b_off:].data_ptr(), self.result[b_off:].data_ptr(), self.ws.data_ptr(), b, b_off, self.B)
        if cfg is None:
            check(lib.ssd_op_multibox_loss_grad(*args, None))
        else:
            check(lib.ssd_op_multibox_loss_grad_ex(*args, C.byref(cfg), None))

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


def _bits(a):
    return a.view(np.uint8 if a.dtype == np.uint8 else np.uint32)


def verify(name, op, out, labels, got, gamma, alpha, bnorm=0.0, sumsq=0.0, wd=0.0):
    """all assertions of one finished focal forward + backward"""
    C_ = op.C
    pos = labels[:, :, C_] == 0
    assert np.array_equal(got['pos'].astype(bool), pos), f'{name}: positive mask'
    assert (got['sel'] == 1).all(), f'{name}: sel is not all ones ({int((got["sel"] != 1).sum())} anchors)'
    sf = fr.stage_f(got['ce'], got['pos'], got['sl1'], gamma, alpha, bnorm, sumsq, wd)
    e_sample, e_loss = _rel(got['sample'], sf['sample']), _rel(got['losses'], sf['losses'])
    d_out, pads = op.read_grads()
    e_g = e_full = float('nan')
    if not op.bf16:
        d_ref = fr.grad(got['result'], labels, got['ce'], got['pos'], got['sample'][:, 2], C_, gamma, alpha)
        e_g = float(np.abs(d_out - d_ref).max() / max(np.abs(d_ref).max(), 1e-300))
        e_full = max_rel(d_out, fr.full_chain(out, labels, C_, gamma, alpha, bnorm)[2])
    print(f'{name}: A {op.lay["A"]} C {C_} gamma {gamma} alpha {alpha} sample {e_sample:.2e} losses {e_loss:.2e} (bound {bound_sums(gamma):.2e}) '
          f'grad {e_g:.2e} (bound {bound_grad(gamma):.2e}) grad-vs-float64-chain {e_full:.2e} pos_n {got["sample"][:, 3].astype(int).tolist()} '
          f'exact zeros in ce {int((got["ce"] == 0).sum())}')
    for k in ('sample', 'losses'):
        assert np.isfinite(got[k]).all(), f'{name}: {k} is not finite'
    assert np.array_equal(got['sample'][:, 3], sf['sample'][:, 3]), f'{name}: pos_n'
    assert _close(got['sample'], sf['sample'], bound_sums(gamma)), f'{name}: sample rel {e_sample:.3e}'
    assert _close(got['losses'], sf['losses'], bound_sums(gamma)), f'{name}: losses rel {e_loss:.3e}'
    for p in pads:
        assert not p.any(), f'{name}: gradient pad columns are not zero'
    if not op.bf16:
        assert np.isfinite(d_out).all(), f'{name}: the gradient holds NaN or Inf'
        assert e_g <= bound_grad(gamma), f'{name}: gradient {e_g:.3e}'
        assert e_full < TOL, f'{name}: gradient against the float64 chain {e_full:.3e}'
    return sf, d_out


def run_case(name, layout, C_, pos_counts, kind, gamma, alpha, easy=None, **kw):
    out, y = fc.make(name, layout, C_, pos_counts, kind, easy)
    cfg = LossConfig(1, gamma, alpha)
    op = LossOp(*layout, C_, out, y)
    op.forward(cfg, **kw)
    op.backward(cfg)
    got = op.read()
    verify(name, op, out, y, got, gamma, alpha, bnorm=kw.get('bnorm', 0.0))
    return op, out, y, got


@pytest.mark.parametrize('case', fc.CASES, ids=fc.CASE_IDS)
def test_focal_case(case):
    name, layout, C_, pos_counts, kind, gamma, alpha, easy = case
    op, out, y, got = run_case(*case)
    # what the head kernels leave is what they leave under mining, bit for bit
    m = LossOp(*layout, C_, out, y)
    m.forward()
    gm = m.read()
    for k in ('pos', 'result', 'ce', 'sl1'):
        assert np.array_equal(_bits(got[k]), _bits(gm[k])), f'{name}: {k} differs from the mining call'
    if 0 in pos_counts:      # a sample without positives trains its background anchors; under mining it contributes exactly 0
        s = pos_counts.index(0)
        assert got['sample'][s, 3] == 0 and got['sample'][s, 1] == 0 and got['sample'][s, 2] > 0 and not gm['sample'][s].any()
        assert got['sample'][s, 0] > 0 or not (got['ce'][s] > 0).any()
        assert np.abs(op.read_grads()[0][s]).max() > 0
    if easy is not None:     # the nearly saturated rows are there: small, not 0
        neg = y[easy, :, C_] != 0
        assert ((got['ce'][easy][neg] > 0) & (got['ce'][easy][neg] < 1e-4)).all()
    if kind == 'palette':    # ... and so are the saturated ones
        assert (got['ce'] == 0).sum() > 0


def test_focal_mining_config_is_the_old_entry_points():
    """kind = SSD_LOSS_MINING (whatever gamma and alpha hold) and a NULL configuration through _ex: bitwise the old calls"""
    name = 'mining through _ex'
    out, y = fc.make(name, fc.MID, 20, [20, 300, 0, 700], 'palette')
    old = LossOp(*fc.MID, 20, out, y)
    old.forward(); old.backward()
    g0, d0 = old.read(), old.read_grads()[0]
    assert not g0['sel'].all()
    for cfg in (LossConfig(0, 99.0, -1.0), LossConfig(0, 2.0, 0.25)):
        op = LossOp(*fc.MID, 20, out, y)
        op.forward(cfg); op.backward(cfg)
        g1, d1 = op.read(), op.read_grads()[0]
        for k in g0:
            assert np.array_equal(_bits(g0[k]), _bits(g1[k])), f'{name}: {k}'
        assert np.array_equal(_bits(d0), _bits(d1)), f'{name}: gradient'


def test_focal_lanes_and_ticket():
    """one call over 5 samples == two calls (3 at 0, 2 at 3) of a step of 5, bit for bit; and again on the same workspace"""
    name = 'focal lanes vgg300'
    gamma, alpha = 2.0, 0.25
    cfg = LossConfig(1, gamma, alpha)
    out, y = fc.make(name, fc.VGG300, 20, [40, 1500, 0, 2900, 500], 'palette')
    rng = np.random.default_rng(3)
    w = rng.normal(0, 0.05, (4100,)).astype(np.float32)
    sumsq = float((w.astype(np.float64) ** 2).sum())
    w_ = dev(w)
    one = LossOp(*fc.VGG300, 20, out, y)
    one.forward(cfg, filters=w_, wd=0.0005)
    one.backward(cfg)
    g1 = one.read()
    verify(name, one, out, y, g1, gamma, alpha, sumsq=sumsq, wd=0.0005)
    assert g1['losses'][3] > 0
    d1 = one.read_grads()[0]
    two = LossOp(*fc.VGG300, 20, out, y)
    for rep in range(2):                     # the second round runs on the workspace the first one left: the ticket reset itself
        if rep:
            two.ws[two.offs[5]:two.offs[5] + 16].zero_()           # losses only: they must be written again
            for g in two.grads:
                g.fill_(SENTINEL)
        two.forward(cfg, b=3, b_off=0, filters=w_, wd=0.0005)
        if not rep:
            assert not host(two.ws[two.offs[5]:two.offs[5] + 16]).any(), 'losses written before the step completed'
        two.forward(cfg, b=2, b_off=3, wd=0.0005)
        two.backward(cfg, b=3, b_off=0)
        two.backward(cfg, b=2, b_off=3)
        g2 = two.read()
        for k in g1:
            assert np.array_equal(_bits(g1[k]), _bits(g2[k])), f'{name}: {k} differs between one call and two lanes (round {rep})'
        assert np.array_equal(_bits(d1), _bits(two.read_grads()[0])), f'{name}: gradient differs (round {rep})'
    # the same single call again on its own workspace
    one.forward(cfg, filters=w_, wd=0.0005)
    one.backward(cfg)
    g3 = one.read()
    for k in g1:
        assert np.array_equal(_bits(g1[k]), _bits(g3[k])), f'{name}: {k} differs on the second call'
    assert np.array_equal(_bits(d1), _bits(one.read_grads()[0]))


def test_focal_bnorm():
    """bnorm = 2.5 against the default (the step's own 4): sums keep their bits, weight and losses rescale"""
    name = 'focal bnorm vgg300'
    gamma, alpha = 2.0, 0.25
    case = (name, fc.VGG300, 20, [40, 1500, 0, 2900], 'palette', gamma, alpha)
    op, out, y, g0 = run_case(*case)
    d0 = op.read_grads()[0]
    op2, _, _, g1 = run_case(*case, bnorm=2.5)
    d1 = op2.read_grads()[0]
    for k in ('sel', 'ce'):
        assert np.array_equal(g0[k], g1[k])
    assert np.array_equal(g0['sample'][:, [0, 1, 3]].view(np.uint32), g1['sample'][:, [0, 1, 3]].view(np.uint32))
    # fp32 roundings apart: the weight is one division, a loss one division (3e-7 as in test_loss_bnorm); a gradient value is
    # the weight times kappa times a difference, three roundings on either side where mining has two: 6 eps = 3.6e-7
    f64 = lambda v: np.asarray(v, np.float64)
    assert _close(f64(g1['sample'][:, 2]) * 2.5, f64(g0['sample'][:, 2]) * 4, 3e-7)
    assert _close(f64(g1['losses'][1:3]) * 2.5, f64(g0['losses'][1:3]) * 4, 3e-7)
    assert max_rel(f64(d1) * 2.5, f64(d0) * 4) < 6 * EPS


def bf16_rne_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


@pytest.mark.parametrize('layout,C_,gamma', [(fc.VGG300, 20, 2.0), (fc.MID, 127, 0.5)], ids=['vgg300', 'mid 127 classes'])
def test_focal_grad_bf16(layout, C_, gamma):
    """bf16 gradient buffers hold round-to-nearest-even of the fp32 run's gradient, pad columns zero in both"""
    name = f'focal bf16 grads {C_}'
    alpha = 0.25
    cfg = LossConfig(1, gamma, alpha)
    A = lr.layout(*layout, C_)['A']
    out, y = fc.make(name, layout, C_, [A // 200, 0, A // 3], 'palette')
    f = LossOp(*layout, C_, out, y)
    f.forward(cfg); f.backward(cfg)
    _, d32 = verify(name + ' (fp32 run)', f, out, y, f.read(), gamma, alpha)
    h = LossOp(*layout, C_, out, y, bf16=True)
    h.forward(cfg); h.backward(cfg)
    verify(name, h, out, y, h.read(), gamma, alpha)
    d16, pads = h.read_grads()
    assert all(not p.any() for p in pads) and d16.dtype == np.uint16
    assert np.count_nonzero(d32) > 1000
    assert np.array_equal(d16, bf16_rne_bits(d32)), f'{name}: {(d16 != bf16_rne_bits(d32)).sum()} values differ from RNE'
