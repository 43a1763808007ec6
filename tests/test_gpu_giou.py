"""-m gpu: the GIoU localization loss in isolation (csrc/ops.hip: the LOC_GIOU instantiations of heads_kernel / heads_wide_kernel,
loss_grad_kernel<float|bf16_t> and focal_grad_kernel<float|bf16_t, narrow|wide>) through ssd_op_multibox_loss_ex2 /
ssd_op_multibox_loss_grad_ex2, under mining and under focal, against the float64 oracle of tests/giou_ref.py on the inputs of
tests/giou_cases.py: identical, touching, disjoint and nested boxes, offsets beyond the clamp (+-1e30 included), samples without
positives and with nothing else, A from 64 to 32256, 1..127 classes, forward lanes, bf16 gradient buffers.

Bounds and where they come from (eps = 2^-24, one fp32 rounding; the device expf is documented at 1 ulp = 2 eps in the HIP math
API's accuracy table; every division is IEEE; giou_eval is compiled without contraction, in the order it is written):
  pos, result, ce, sel     bit for bit what the same call leaves under smooth-L1
  smooth-L1 / NULL         every buffer and gradient bit for bit what the _ex entry points leave
  sl1 (the term)           weight * L against giou_ref.terms on the kernel's OWN result, absolute (L is O(1)).  A size w = exp(t / 5)
                           is expf(q) * (1 + (t - 5 q) / 5) with q = fl(t / 5) and t - 5 q exact by fma: 2 eps of expf, 1 of the
                           last fma, the quotient's own rounding second order: rho = 3 eps relative (20 eps without the
                           correction, |q| <= 20).  The centre difference (tc0 - gc0) / 10: 2 eps of its own value.  An edge in the
                           ground-truth box's frame (dx -+ wp / 2, -+ wg / 2): <= 4 eps (|dx| + wp / 2), 3 eps (wg / 2).  Where the
                           boxes overlap |dx| <= (wp + wg) / 2, so iw carries <= 9 eps (wp + wg) and I / U moves by
                           <= 9 eps (wp + wg) min(hp, hg) / U <= 18 eps per axis (U >= max(wp hp, wg hg)), 37 eps with the product's
                           rounding.  U = wp hp + wg hg - I: 8 eps (U + I) + 37 eps U + 1 eps <= 54 eps relative.  cw: two edges
                           of <= 8 eps cw each and the difference, 17 eps; C: 35 eps.  L = (1 - I/U) + (1 - U/C):
                           (37 + 54 + 1) + (54 + 35 + 1) + 3 = 185 eps = 1.1e-5 in the worst case of every step at once -- above the
                           issue's cap, so the cap is the bound:   BOUND_TERM = min(1e-5, 185 eps) = 1e-5 (absolute, on the term)
                           The errors measured are ~4 eps (printed by every case).
  sample, losses           stage B / stage F on the kernel's OWN ce and sl1, within those tests' bounds: 1e-5 under mining
                           (test_gpu_loss.py TOL_SUMS), 3.2e-6 + (2 gamma + 11) eps under focal (test_gpu_focal.py BOUND_SUMS)
  gradient                 loss_ref.grad / focal_ref.grad with giou_ref's loc columns, on the kernel's own result, ce and sample
                           weight, relative to the largest magnitude of the tensor.  A loc value is weight * w_b * dL/dt; dL/dt2 =
                           (gx1 - gx0) * wp / 10 is a sum of six terms k * extent * wp / 10, each bounded (|kI ih wp| <= 3,
                           |kA hp wp| <= 2, |kC ch wp| <= 1, since C >= U >= wp hp >= wp ih), each carrying the relative errors
                           of its k (kA = (I/U)/U - 1/C: a difference of two quotients of <= 1/U, 92 + 54 + 1 and 35 + 1 eps of
                           1/U), its extent (<= 17 eps) and wp (3 eps), then 5 roundings: <= (147 + 36 + 20 + 5) eps * 6 * 2 / 10
                           ~ 250 eps = 1.5e-5 of weight * w_b in the worst case -- above the cap again:
                               BOUND_GRAD = 1e-5 of the largest magnitude (the confidence columns: 1.6e-6, test_gpu_focal.py)
                           against the full float64 chain from the raw logits: 1e-3 (BASELINE.json north_star)
  exact zeros              the loc columns of every negative, every component with |t| > 100, pad columns
  identical boxes          exactly 0, term and gradient: the kernel works in the ground-truth box's frame, where tc == gc gives
                           dx = 0 and edges -+ w / 2 on both sides, so iw == cw == w, I == C == w h and U = w h + w h - I == I
                           without a rounding; kA = 1/U - 1/C == 0 and the two remaining terms of every edge cancel bit for bit
  bf16 gradient            the bits of round-to-nearest-even of the fp32 run's gradient
  finite                   everywhere
The measured errors are printed by every case."""
import ctypes as C

import numpy as np
import pytest
import torch

import focal_ref as fr
import giou_cases as gc
import giou_ref as gr
import loss_ref as lr
from gpu_util import lib, check, dev, host, max_rel
from ssd_tensorflow_amd.ssdvgg import LossConfig, LocLossConfig

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
TOL = 1e-3              # the gradient against the full float64 chain
CAP = 1e-5              # the issue's cap on both derived bounds
BOUND_TERM = min(CAP, 185 * EPS)
BOUND_GRAD = min(CAP, 250 * EPS)
TOL_SUMS_MINING = 1e-5
SENTINEL = 7.0


def bound_sums(conf, gamma):
    return TOL_SUMS_MINING if conf == 'mining' else min(CAP, 3.2e-6 + (2 * gamma + 11) * EPS)


def _ints(v):
    return (C.c_int * len(v))(*v)


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _ref(s):
    return None if s is None else C.byref(s)


class LossOp:
    """device buffers of one step of B samples on a layout, and the calls in lanes (test_gpu_focal.py's helper, restated, with the
    two configurations: entry 'ex2' takes both, 'ex' the confidence one only)"""

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

    def forward(self, cfg=None, loc=None, entry='ex2', b=None, b_off=0, bnorm=0.0, filters=None, wd=0.0):
        b = self.B if b is None else b
        lay = self.lay
        args = (lay['nmaps'], self.hw_, self.nj_, self.C, _ptrs(self._lane(self.heads, b_off)), self.labels[b_off:].data_ptr(),
                self.result[b_off:].data_ptr(), self.ws.data_ptr(), b, b_off, self.B, bnorm,
                None if filters is None else filters.data_ptr(), 0 if filters is None else filters.numel(), wd)
        if entry == 'ex2':
            check(lib.ssd_op_multibox_loss_ex2(*args, _ref(cfg), _ref(loc), None))
        else:
            assert loc is None
            check(lib.ssd_op_multibox_loss_ex(*args, _ref(cfg), None))

    def backward(self, cfg=None, loc=None, entry='ex2', b=None, b_off=0):
        b = self.B if b is None else b
        lay = self.lay
        args = (lay['nmaps'], self.hw_, self.nj_, self.C, _ptrs(self._lane(self.grads, b_off)), int(self.bf16),
                self.labels[b_off:].data_ptr(), self.result[b_off:].data_ptr(), self.ws.data_ptr(), b, b_off, self.B)
        if entry == 'ex2':
            check(lib.ssd_op_multibox_loss_grad_ex2(*args, _ref(cfg), _ref(loc), None))
        else:
            assert loc is None
            check(lib.ssd_op_multibox_loss_grad_ex(*args, _ref(cfg), None))

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
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def configs(conf, gamma, alpha, weight):
    return (LossConfig(1, gamma, alpha) if conf == 'focal' else LossConfig(0, 2.0, 0.25)), LocLossConfig(1, weight)


def stage_sums(conf, got, sl1, gamma, alpha, bnorm=0.0, sumsq=0.0, wd=0.0):
    if conf == 'focal':
        return fr.stage_f(got['ce'], got['pos'], sl1, gamma, alpha, bnorm, sumsq, wd)
    return lr.stage_b(got['ce'], got['pos'], sl1, bnorm, sumsq, wd)


def chain_grad(conf, result, labels, ce, pos, s, C_, gamma, alpha, weight):
    """the oracle's gradient from a given result, cross entropies and stage B / F"""
    if conf == 'focal':
        d = fr.grad(result, labels, ce, pos, s['sample'][:, 2], C_, gamma, alpha)
    else:
        d = lr.grad(result, labels, s['sel'], pos, s['sample'][:, 2], C_)
    return gr.with_loc_grad(d, result, labels, C_, weight, s['sample'][:, 2])


def verify(name, op, out, labels, got, conf, gamma, alpha, weight, bnorm=0.0, sumsq=0.0, wd=0.0):
    """all assertions of one finished GIoU forward + backward"""
    C_ = op.C
    pos = labels[:, :, C_] == 0
    assert np.array_equal(got['pos'].astype(bool), pos), f'{name}: positive mask'
    term = gr.terms(got['result'], labels, C_, weight)
    e_t = float(np.abs(got['sl1'].astype(np.float64) - term).max())
    s = stage_sums(conf, got, got['sl1'], gamma, alpha, bnorm, sumsq, wd)
    e_sample, e_loss = _rel(got['sample'], s['sample']), _rel(got['losses'], s['losses'])
    d_out, pads = op.read_grads()
    e_g = e_full = float('nan')
    if not op.bf16:
        want = dict(sample=got['sample'], sel=got['sel'])
        d_ref = chain_grad(conf, got['result'], labels, got['ce'], got['pos'], want, C_, gamma, alpha, weight)
        e_g = float(np.abs(d_out - d_ref).max() / max(np.abs(d_ref).max(), 1e-300))
        # the float64 chain from the raw head outputs.  Under mining the SELECTION is taken by the rule on the kernel's own cross
        # entropies (equal values are only equal in the precision they were computed in: loss_ref.py; test_gpu_loss.py judges the
        # selection), everything else -- softmax, GIoU terms, weights, gradient -- is float64 from the raw outputs
        a = lr.stage_a(out, labels, C_)
        sf = stage_sums(conf, dict(ce=got['ce'] if conf == 'mining' else a['ce'], pos=a['pos']), gr.terms(out, labels, C_, weight),
                        gamma, alpha, bnorm)
        e_full = max_rel(d_out, chain_grad(conf, a['result'], labels, a['ce'], a['pos'], sf, C_, gamma, alpha, weight))
    print(f'{name}: A {op.lay["A"]} C {C_} {conf} weight {weight} term abs {e_t:.2e} (bound {BOUND_TERM:.2e}) sample {e_sample:.2e} losses '
          f'{e_loss:.2e} (bound {bound_sums(conf, gamma):.2e}) grad {e_g:.2e} (bound {BOUND_GRAD:.2e}) grad-vs-float64-chain {e_full:.2e} '
          f'pos_n {got["sample"][:, 3].astype(int).tolist()} largest term {float(got["sl1"].max()):.4f}')
    assert np.isfinite(got['sl1']).all() and not got['sl1'][~pos].any() and (got['sl1'] >= 0).all(), f'{name}: sl1 off the positives'
    assert e_t <= BOUND_TERM, f'{name}: term {e_t:.3e}'
    for k in ('sample', 'losses'):
        assert np.isfinite(got[k]).all(), f'{name}: {k} is not finite'
    assert np.array_equal(got['sample'][:, 3], s['sample'][:, 3]), f'{name}: pos_n'
    assert _close(got['sample'], s['sample'], bound_sums(conf, gamma)), f'{name}: sample rel {e_sample:.3e}'
    assert _close(got['losses'], s['losses'], bound_sums(conf, gamma)), f'{name}: losses rel {e_loss:.3e}'
    for p in pads:
        assert not p.any(), f'{name}: gradient pad columns are not zero'
    if not op.bf16:
        assert np.isfinite(d_out).all(), f'{name}: the gradient holds NaN or Inf'
        assert e_g <= BOUND_GRAD, f'{name}: gradient {e_g:.3e}'
        assert e_full < TOL, f'{name}: gradient against the float64 chain {e_full:.3e}'
        loc = d_out[:, :, C_ + 1:]
        assert not loc[~pos].any(), f'{name}: a negative anchor has a localization gradient'
        assert not loc[np.abs(got['result'][:, :, C_ + 1:]) > 100].any(), f'{name}: a clamped component has a gradient'
    return s, d_out


def run_case(case, bf16=False, **kw):
    name, layout, C_, pos_counts, kind, conf, gamma, alpha, weight = case
    out, y, tie = gc.make(name, layout, C_, pos_counts, kind)
    cfg, loc = configs(conf, gamma, alpha, weight)
    op = LossOp(*layout, C_, out, y, bf16=bf16)
    op.forward(cfg, loc, **kw)
    op.backward(cfg, loc)
    got = op.read()
    _, d_out = verify(name, op, out, y, got, conf, gamma, alpha, weight, bnorm=kw.get('bnorm', 0.0))
    return op, out, y, tie, got, d_out


@pytest.mark.parametrize('case', gc.CASES, ids=gc.CASE_IDS)
def test_giou_case(case):
    name, layout, C_, pos_counts, kind, conf, gamma, alpha, weight = case
    op, out, y, tie, got, d_out = run_case(case)
    # what does not depend on the localization loss is what the same call leaves under smooth-L1, bit for bit
    cfg, _ = configs(conf, gamma, alpha, weight)
    m = LossOp(*layout, C_, out, y)
    m.forward(cfg, LocLossConfig(0, 1.0))
    gm = m.read()
    for k in ('pos', 'result', 'ce', 'sel'):
        assert np.array_equal(_bits(got[k]), _bits(gm[k])), f'{name}: {k} differs from the smooth-L1 call'
    assert not np.array_equal(got['sl1'], gm['sl1'])
    # the palette is there: clamped components, identical boxes (unit ones and others)
    t = got['result'][:, :, C_ + 1:]; g = y[:, :, C_ + 1:]
    pos = y[:, :, C_] == 0
    assert (np.abs(t[pos]) > 100).any() and tie.any()
    unit_same = pos & (t == 0).all(-1) & (g == 0).all(-1)
    same = pos & (t == g).all(-1)
    assert unit_same.any() and (same & ~unit_same).any()
    assert not got['sl1'][same].any() and not d_out[same][:, C_ + 1:].any(), f'{name}: identical boxes are not at exactly 0'
    print(f'{name}: identical boxes {int(same.sum())}: largest term {float(got["sl1"][same].max()):.2e}, largest gradient '
          f'{float(np.abs(d_out[same][:, C_ + 1:]).max()):.2e}')
    # boxes that touch in x and coincide in y (unit boxes, every step exact): I = 0, U = 2, C = 2, L = 1 to the bit, not live
    touch = pos & (np.abs(t[..., 0] - g[..., 0]) == 10) & (t[..., 1] == g[..., 1]) & (t[..., 2:] == 0).all(-1) & (g[..., 2:] == 0).all(-1)
    assert touch.any() and (got['sl1'][touch] == np.float32(weight)).all(), f'{name}: a touching pair'
    if 0 in pos_counts:      # a sample without positives has no localization term and no localization gradient
        s = pos_counts.index(0)
        assert not got['sl1'][s].any() and got['sample'][s, 1] == 0 and not d_out[s][:, C_ + 1:].any()


@pytest.mark.parametrize('conf', ['mining', 'focal'])
@pytest.mark.parametrize('layout,C_', [(gc.MID, 20), (gc.MID, 28)], ids=['narrow', 'wide'])
def test_smooth_l1_through_ex2_is_the_ex_entry_points(conf, layout, C_):
    """kind = SSD_LOC_SMOOTH_L1 (whatever weight holds) and a NULL localization configuration through _ex2: bitwise the _ex calls,
    every buffer, fp32 and bf16 gradients"""
    name = f'smooth-L1 through _ex2 {conf} {C_}'
    out, y, _ = gc.make(name, layout, C_, [20, 300, 0, 700], 'palette')
    cfg = LossConfig(1, 2.0, 0.25) if conf == 'focal' else LossConfig(0, 2.0, 0.25)
    for bf16 in (False, True):
        old = LossOp(*layout, C_, out, y, bf16=bf16)
        old.forward(cfg, entry='ex'); old.backward(cfg, entry='ex')
        g0, d0 = old.read(), old.read_grads()[0]
        assert g0['sl1'].any() and np.count_nonzero(d0) > 1000
        for loc in (LocLossConfig(0, float('nan')), LocLossConfig(0, 3.0), None):
            op = LossOp(*layout, C_, out, y, bf16=bf16)
            op.forward(cfg, loc); op.backward(cfg, loc)
            g1, d1 = op.read(), op.read_grads()[0]
            for k in g0:
                assert np.array_equal(_bits(g0[k]), _bits(g1[k])), f'{name}: {k}'
            assert np.array_equal(_bits(d0), _bits(d1)), f'{name}: gradient (bf16 {bf16})'
    if conf == 'mining':          # ... and a NULL confidence configuration beside them
        op = LossOp(*layout, C_, out, y)
        op.forward(None, None); op.backward(None, None)
        old = LossOp(*layout, C_, out, y)
        old.forward(cfg, entry='ex'); old.backward(cfg, entry='ex')
        assert np.array_equal(_bits(op.read_grads()[0]), _bits(old.read_grads()[0]))


@pytest.mark.parametrize('conf', ['mining', 'focal'])
def test_giou_lanes_and_ticket(conf):
    """one call over 5 samples == two calls (3 at 0, 2 at 3) of a step of 5, bit for bit; and again on the same workspace"""
    name = f'giou lanes vgg300 {conf}'
    gamma, alpha, weight = 2.0, 0.25, 2.0
    cfg, loc = configs(conf, gamma, alpha, weight)
    out, y, _ = gc.make(name, gc.VGG300, 20, [40, 1500, 0, 2900, 500], 'palette')
    rng = np.random.default_rng(3)
    w = rng.normal(0, 0.05, (4100,)).astype(np.float32)
    sumsq = float((w.astype(np.float64) ** 2).sum())
    w_ = dev(w)
    one = LossOp(*gc.VGG300, 20, out, y)
    one.forward(cfg, loc, filters=w_, wd=0.0005)
    one.backward(cfg, loc)
    g1 = one.read()
    verify(name, one, out, y, g1, conf, gamma, alpha, weight, sumsq=sumsq, wd=0.0005)
    assert g1['losses'][3] > 0
    d1 = one.read_grads()[0]
    two = LossOp(*gc.VGG300, 20, out, y)
    for rep in range(2):                     # the second round runs on the workspace the first one left: the ticket reset itself
        if rep:
            two.ws[two.offs[5]:two.offs[5] + 16].zero_()           # losses only: they must be written again
            for g in two.grads:
                g.fill_(SENTINEL)
        two.forward(cfg, loc, b=3, b_off=0, filters=w_, wd=0.0005)
        if not rep:
            assert not host(two.ws[two.offs[5]:two.offs[5] + 16]).any(), 'losses written before the step completed'
        two.forward(cfg, loc, b=2, b_off=3, wd=0.0005)
        two.backward(cfg, loc, b=3, b_off=0)
        two.backward(cfg, loc, b=2, b_off=3)
        g2 = two.read()
        for k in g1:
            assert np.array_equal(_bits(g1[k]), _bits(g2[k])), f'{name}: {k} differs between one call and two lanes (round {rep})'
        assert np.array_equal(_bits(d1), _bits(two.read_grads()[0])), f'{name}: gradient differs (round {rep})'
    # the same single call again on its own workspace
    one.forward(cfg, loc, filters=w_, wd=0.0005)
    one.backward(cfg, loc)
    g3 = one.read()
    for k in g1:
        assert np.array_equal(_bits(g1[k]), _bits(g3[k])), f'{name}: {k} differs on the second call'
    assert np.array_equal(_bits(d1), _bits(one.read_grads()[0]))


def bf16_rne_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


@pytest.mark.parametrize('case', [gc.CASES[0], gc.CASES[1], gc.CASES[10], gc.CASES[13]],
                         ids=['vgg300 mining', 'vgg300 focal', '28 classes mining', '127 classes focal'])
def test_giou_grad_bf16(case):
    """bf16 gradient buffers hold round-to-nearest-even of the fp32 run's gradient, pad columns zero in both"""
    _, _, _, _, _, d32 = run_case(case)
    h, _, _, _, _, _ = run_case(case, bf16=True)
    d16, pads = h.read_grads()
    assert all(not p.any() for p in pads) and d16.dtype == np.uint16
    assert np.count_nonzero(d32[:, :, case[2] + 1:]) > 20
    assert np.array_equal(d16, bf16_rne_bits(d32)), f'{case[0]}: {(d16 != bf16_rne_bits(d32)).sum()} values differ from RNE'
