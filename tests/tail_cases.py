"""Stage lists for the multi-stage launches of the bf16 tail (csrc/tail_bf16.hip tail_chain_bf16, conv_wgrad_group_bf16), shared by
the CPU plan tests (test_tail_plan.py) and the GPU tests (test_gpu_tail_chain.py).

A Chain is a list of stages over NAMED tensors: a stage whose src is an earlier stage's dst reads it from LDS, which is the code the
one-stage entry points never reach.  Three families:
  (a) NET_CHAINS      the nets' own launches, restated from csrc/net.hip: forward = the chain's layers in Net::build_orders' issue
                      order (a head right behind the map it reads), backward = reverse graph order (heads first) without the chain's
                      first layer, with launch_tail_backward's rule: a stage accumulates when an earlier stage already wrote that
                      gradient, and carries the relu mask when it is the tensor's last consumer.  Shapes: test_gpu_tail.TAIL_CASES.
  (b) STRESS_CHAINS   lists built for what (a) does not reach (see each builder)
  (c) REFUSED_CHAINS  lists the planner must refuse, with a word of the error text
WGRAD_GROUPS are the layer lists of the grouped weight gradient."""
import ctypes as C
from collections import namedtuple

import numpy as np

from ssd_tensorflow_amd._lib import lib, TailStage, TailPlanStage

St = namedtuple('St', 'hi wi ci ho wo co k stride ph pw dgrad relu accum out_f32 bias src dst mask')
Layer = namedtuple('Layer', 'hi wi ci ho wo co k stride ph pw')


def _same_pad(n, k, s):
    out = -(-n // s)
    return max((out - 1) * s + k - n, 0) // 2, out


def geom(hi, wi, k, stride, padding):
    """(ph, pw, ho, wo), TF semantics; 'BR1' = one row / column of zeros below / right of the image, then VALID"""
    if padding == 'SAME':
        ph, ho = _same_pad(hi, k, stride)
        pw, wo = _same_pad(wi, k, stride)
        return ph, pw, ho, wo
    extra = 1 if padding == 'BR1' else 0
    return 0, 0, (hi + extra - k) // stride + 1, (wi + extra - k) // stride + 1


class Chain:
    """stages + the shape (h, w, c, 'bf16' | 'f32') of every tensor they name"""

    def __init__(self, name, b):
        self.name, self.b, self.stages, self.tensors = name, b, [], {}
        self.poison = set()      # input tensors filled with values near the top of the bf16 range (and the stage that reads them: tiny filters)

    def _tensor(self, name, h, w, c, kind='bf16'):
        if name in self.tensors:
            assert self.tensors[name] == (h, w, c, kind), (name, self.tensors[name], (h, w, c, kind))
        self.tensors[name] = (h, w, c, kind)

    def fwd(self, src, dst, hi, wi, ci, co, k, stride=1, padding='SAME', relu=True, f32=False, bias=True):
        ph, pw, ho, wo = geom(hi, wi, k, stride, padding)
        self._tensor(src, hi, wi, ci)
        self._tensor(dst, ho, wo, co, 'f32' if f32 else 'bf16')
        self.stages.append(St(hi, wi, ci, ho, wo, co, k, stride, ph, pw, False, relu, False, f32, bias, src, dst, None))
        return self

    def dgrad(self, src, dst, hi, wi, ci, co, k, stride=1, padding='SAME', accum=False, mask=None):
        """the data gradient of the convolution (hi, wi, ci) -> (ho, wo, co): src = dy, dst = dx"""
        ph, pw, ho, wo = geom(hi, wi, k, stride, padding)
        self._tensor(src, ho, wo, co)
        self._tensor(dst, hi, wi, ci)
        if mask:
            self._tensor(mask, hi, wi, ci)
        self.stages.append(St(hi, wi, ci, ho, wo, co, k, stride, ph, pw, True, False, accum, False, False, src, dst, mask))
        return self

    def produced_before(self, i, name):
        return any(s.dst == name for s in self.stages[:i])

    def inputs(self):
        """tensors a launch reads that no earlier stage of it wrote: sources, masks, accumulated gradients"""
        need = []
        for i, s in enumerate(self.stages):
            for n in (s.src, s.mask, s.dst if s.accum else None):
                if n and not self.produced_before(i, n) and n not in need:
                    need.append(n)
        return need

    def layers(self):
        return [Layer(*s[:10]) for s in self.stages]


# ------------------------------------------------------------------------------------------------------------ (a) the nets' chains
def _net_layers(pname):
    """[(name, in tensor, hi, ci, co, k, stride, padding, head)] in graph order: the extra layers from the chain's first on, then the
    heads of the maps they produce (3x3 SAME, 152 = 6 box types, 104 = 4 box types x 25 padded to 8 channels)"""
    if pname == 'vgg300':
        ex = [('conv9_1', 10, 512, 128, 1, 1, 'SAME'), ('conv9_2', 10, 128, 256, 3, 2, 'SAME'), ('conv10_1', 5, 256, 128, 1, 1, 'SAME'),
              ('conv10_2', 5, 128, 256, 3, 1, 'VALID'), ('conv11_1', 3, 256, 128, 1, 1, 'SAME'), ('conv11_2', 3, 128, 256, 3, 1, 'VALID')]
        heads = [('head3', 'conv9_2', 5, 152), ('head4', 'conv10_2', 3, 104), ('head5', 'conv11_2', 1, 104)]
        first_in = 'conv8_2'
    else:
        ex = [('conv10_1', 8, 256, 128, 1, 1, 'SAME'), ('conv10_2', 8, 128, 256, 3, 2, 'SAME'), ('conv11_1', 4, 256, 128, 1, 1, 'SAME'),
              ('conv11_2', 4, 128, 256, 3, 1, 'VALID'), ('conv12_1', 2, 256, 128, 1, 1, 'SAME'), ('conv12_2', 2, 128, 256, 3, 1, 'BR1')]
        heads = [('head4', 'conv10_2', 4, 152), ('head5', 'conv11_2', 2, 104), ('head6', 'conv12_2', 1, 104)]
        first_in = 'conv9_2'
    ops, prev = [], first_in
    for (n, hi, ci, co, k, s, p) in ex:
        ops.append((n, prev, hi, ci, co, k, s, p, False))
        prev = n
    for (n, src, hi, co) in heads:
        ops.append((n, src, hi, 256, co, 3, 1, 'SAME', True))
    return ops


def net_forward(pname, b):
    ops = _net_layers(pname)
    ch = Chain(f'{pname} forward b={b}', b)
    for op in [o for o in ops if not o[8]]:      # issue order: a head right behind the tensor it reads
        ch.fwd(op[1], op[0], op[2], op[2], op[3], op[4], op[5], op[6], op[7], relu=True)
        for h in [o for o in ops if o[8] and o[1] == op[0]]:
            ch.fwd(h[1], h[0], h[2], h[2], h[3], h[4], h[5], h[6], h[7], relu=False, f32=True)
    return ch


def net_backward(pname, b):
    ops = _net_layers(pname)
    consumers = {}
    for op in ops:
        consumers[op[1]] = consumers.get(op[1], 0) + 1
    done = {}
    ch = Chain(f'{pname} backward b={b}', b)
    for op in reversed(ops[1:]):      # reverse graph order; the chain's first layer keeps its own launch
        n, src = op[0], op[1]
        last = done.get(src, 0) + 1 == consumers[src]
        ch.dgrad('g:' + n, 'g:' + src, op[2], op[2], op[3], op[4], op[5], op[6], op[7], accum=done.get(src, 0) > 0, mask=src if last else None)
        done[src] = done.get(src, 0) + 1
    return ch


def net_wgrad_layers(pname):
    """the layers of the step's grouped weight gradient: the chain's in graph order, without its first"""
    out = []
    for op in _net_layers(pname)[1:]:
        ph, pw, ho, wo = geom(op[2], op[2], op[5], op[6], op[7])
        out.append(Layer(op[2], op[2], op[3], ho, wo, op[4], op[5], op[6], ph, pw))
    return out


NET_CHAINS = [f(p, b) for p in ('vgg300', 'vgg512') for f in (net_forward, net_backward) for b in (1, 3)]


# ------------------------------------------------------------------------------------------------------------ (b) stress lists
def sixteen_stages():
    """TAIL_MAX_STAGES stages of 1x1 and 3x3 layers on a 6x7 map (42 pixels: three pixel blocks, the last ragged).  Channel counts:
    72 = a k tail (TF_KTAIL) at a pixel pitch of 160 bytes, no multiple of 256; 8 = one n block and, behind 320 channels x 9 taps, a
    4-way k split; 320 = 20 tasks, a second round of the 16 waves.  Every stage boundary changes the number of n blocks (the filter
    stream's step) and most change the k split; waves gain and lose tasks across boundaries in both directions."""
    c = [64, 320, 8, 72, 128, 320, 72, 8, 64, 128, 72, 320, 64, 8, 320, 128, 64]
    k = [1, 3, 3, 1, 3, 1, 3, 1, 3, 3, 3, 3, 1, 1, 1, 3]
    ch = Chain('16 stages on 6x7', 2)
    for i in range(16):
        ch.fwd(f't{i}', f't{i + 1}', 6, 7, c[i], c[i + 1], k[i], relu=i != 15, bias=i != 7)
    return ch


def far_reader():
    """t1 is read by stage 1 and again by the last stage, the launch's own input t0 by stage 0 and stage 4: both stay live across
    stages that allocate and free other regions"""
    ch = Chain('a tensor read by stage 1 and by the last stage', 3)
    ch.fwd('t0', 't1', 5, 5, 64, 128, 3)
    ch.fwd('t1', 't2', 5, 5, 128, 72, 1)
    ch.fwd('t2', 't3', 5, 5, 72, 320, 3)
    ch.fwd('t3', 't4', 5, 5, 320, 64, 1)
    ch.fwd('t0', 't5', 5, 5, 64, 72, 1)
    ch.fwd('t4', 't6', 5, 5, 64, 8, 3)
    ch.fwd('t1', 't7', 5, 5, 128, 136, 3, padding='VALID', relu=False)
    return ch


def reuse():
    """regions freed and taken again by tensors of other sizes: smaller than the hole, exactly as large, larger (placed elsewhere)"""
    ch = Chain('regions freed and reused', 2)
    ch.fwd('t0', 't1', 5, 5, 128, 64, 1)
    ch.fwd('t1', 't2', 5, 5, 64, 72, 3)          # t2 (smaller) takes t0's place
    ch.fwd('t2', 't3', 5, 5, 72, 64, 3)          # t3 takes t1's place: exactly as large
    ch.fwd('t3', 't4', 5, 5, 64, 320, 1)         # t4 is larger than any hole
    ch.fwd('t4', 't5', 5, 5, 320, 8, 3)          # 4-way k split: scratch above t4 and t5
    ch.fwd('t5', 't6', 5, 5, 8, 128, 3, relu=False)
    return ch


def poisoned_reuse():
    """The launch's input t0 holds finite values near the top of the bf16 range (2^126 ... 2^127; stage 0's filter is +-1..3 x 2^-126, so
    its output is O(10)).  Its region goes to t2, a 72-channel tensor (TF_KTAIL input of stage 2, pitch 160): t2's pixel rows cover less
    than t0's did, so the 16 pad bytes of each row and everything behind the last row still hold t0's values.  A gather that reads
    past SC or past a pixel row multiplies them with real filter values: Inf or NaN instead of a small error."""
    ch = Chain('reuse under a KTAIL input after a tenant near the top of the bf16 range', 2)
    ch.poison.add('t0')
    ch.fwd('t0', 't1', 5, 5, 128, 64, 1)
    ch.fwd('t1', 't2', 5, 5, 64, 72, 3)
    ch.fwd('t2', 't3', 5, 5, 72, 128, 3)
    ch.fwd('t3', 't4', 5, 5, 128, 72, 1)         # t4: KTAIL input again, in t1's old place
    ch.fwd('t4', 't5', 5, 5, 72, 64, 3, relu=False)
    return ch


def dgrad_accumulate():
    """Data gradients.  g:x is written by stage 0 (its first consumer's gradient, kept in LDS because stage 3 accumulates into it), two
    unrelated stages run, stage 3 accumulates into the LDS copy and masks, stage 4 -- a stride-2 layer's gradient: only every other
    source pixel meets a tap -- gathers from it.  Stage 5 accumulates into a gradient written before the launch (TF_LOAD_OUT behind an
    input that is already in LDS)."""
    ch = Chain('accumulate into an LDS-resident gradient, stride-2 data gradient', 3)
    ch.dgrad('g:h', 'g:x', 5, 5, 64, 104, 3)                                     # x's head: first consumer, no mask
    ch.dgrad('g:v', 'g:c', 5, 5, 72, 128, 3, padding='VALID', mask='c')          # unrelated (produces the gradient stage 3 reads)
    ch.dgrad('g:z', 'g:y', 2, 2, 128, 64, 1)                                     # unrelated
    ch.dgrad('g:c', 'g:x', 5, 5, 64, 72, 1, accum=True, mask='x')
    ch.dgrad('g:x', 'g:w', 10, 10, 72, 64, 3, stride=2, mask='w')
    ch.dgrad('g:x', 'g:n', 5, 5, 128, 64, 1, accum=True)
    return ch


def accumulate_at_once():
    """the accumulate right behind the stage that produced the tensor (no stage in between for its global copy to settle), twice"""
    ch = Chain('accumulate right behind the producer', 3)
    ch.dgrad('g:a', 'g:x', 3, 3, 64, 72, 3)
    ch.dgrad('g:b', 'g:x', 3, 3, 64, 128, 1, accum=True)
    ch.dgrad('g:d', 'g:x', 3, 3, 64, 8, 3, accum=True, mask='x')
    ch.dgrad('g:x', 'g:w', 5, 5, 72, 64, 3, padding='VALID', mask='w')
    return ch


def output_over_a_dead_input():
    """Stage 2 writes its output over the launch's own input t0 in GLOBAL memory -- legal: t0's only reader was stage 0, nobody reads
    the new values inside the launch.  t0's LDS region has long gone to t2, stage 2's input.  (The planner looked the output's region
    up by pointer alone, found t0's dead one, and the epilogue wrote the output over the pixels other waves were still gathering.)"""
    ch = Chain('output over a dead input', 2)
    ch.fwd('t0', 't1', 5, 5, 64, 128, 3)
    ch.fwd('t1', 't2', 5, 5, 128, 64, 1)
    ch.fwd('t2', 't0', 5, 5, 64, 64, 3)
    ch.fwd('t2', 't3', 5, 5, 64, 72, 1, relu=False)
    return ch


def f32_heads_between():
    ch = Chain('fp32-output heads between bf16 stages', 3)
    ch.fwd('t0', 't1', 3, 3, 72, 128, 1)
    ch.fwd('t1', 'h1', 3, 3, 128, 104, 3, relu=False, f32=True)
    ch.fwd('t1', 't2', 3, 3, 128, 64, 3, padding='VALID')
    ch.fwd('t2', 'h2', 1, 1, 64, 152, 3, relu=False, f32=True)
    ch.fwd('t2', 't3', 1, 1, 64, 72, 1)
    ch.fwd('t3', 'h3', 1, 1, 72, 8, 1, relu=False, f32=True)
    return ch


def pixel_counts():
    """M = 100 (two pixel groups: 4 + 3 blocks), 25 (2 blocks), 9 and 1 (one ragged block); (42: sixteen_stages)"""
    ch = Chain('maps of 100, 25, 9 and 1 pixels', 3)
    ch.fwd('t0', 't1', 10, 10, 64, 72, 1)
    ch.fwd('t1', 't2', 10, 10, 72, 128, 3, stride=2)
    ch.fwd('t2', 't3', 5, 5, 128, 64, 1)
    ch.fwd('t3', 't4', 5, 5, 64, 72, 3, padding='VALID')
    ch.fwd('t4', 't5', 3, 3, 72, 8, 1)
    ch.fwd('t5', 't6', 3, 3, 8, 64, 3, padding='VALID')
    ch.fwd('t6', 't7', 1, 1, 64, 320, 1, relu=False)
    return ch


STRESS_CHAINS = [sixteen_stages(), far_reader(), reuse(), poisoned_reuse(), dgrad_accumulate(), accumulate_at_once(), output_over_a_dead_input(),
                 f32_heads_between(), pixel_counts()]
ALL_CHAINS = NET_CHAINS + STRESS_CHAINS


# ------------------------------------------------------------------------------------------------------------ (c) refused lists
def _seventeen():
    ch = sixteen_stages()
    ch.name = '17 stages'
    ch.fwd('t16', 't17', 6, 7, 64, 64, 1)
    return ch


def _overwrite():
    ch = Chain('a stage overwrites an LDS-resident tensor', 2)
    ch.fwd('t0', 't1', 5, 5, 64, 64, 1)
    ch.fwd('t1', 't2', 5, 5, 64, 64, 3)
    ch.fwd('t2', 't1', 5, 5, 64, 64, 1)
    ch.fwd('t1', 't3', 5, 5, 64, 64, 1)
    return ch


def _too_much_lds():
    ch = Chain('two 10x10x512 maps live at once', 1)      # 2 x 100 pixels x (1024 + 16) bytes
    ch.fwd('t0', 't1', 10, 10, 512, 512, 1)
    ch.fwd('t1', 't2', 10, 10, 512, 64, 1)
    return ch


def _unsupported():
    ch = Chain('a 5x5 filter', 2)
    ch.fwd('t0', 't1', 5, 5, 64, 64, 1)
    ch.fwd('t1', 't2', 5, 5, 64, 64, 5)
    return ch


REFUSED_CHAINS = [(_seventeen(), '1..16 stages (got 17)'), (_overwrite(), 'overwrites a tensor an earlier stage left in LDS'),
                  (_too_much_lds(), 'bytes of LDS (limit 163840)'), (_unsupported(), 'stage 1 has an unsupported shape')]


# ------------------------------------------------------------------------------------------------------------ grouped weight gradient
def _layer(hi, wi, ci, co, k, stride=1, padding='SAME'):
    ph, pw, ho, wo = geom(hi, wi, k, stride, padding)
    return Layer(hi, wi, ci, ho, wo, co, k, stride, ph, pw)


# 12 layers = WGRAD_GROUP_MAX: 1 ... 27 workgroups per layer (taps x ceil(Ci / 64) x ceil(Co / 128)), ragged channel tiles, ragged pixels
TWELVE_LAYERS = [_layer(6, 7, 64, 320, 1), _layer(6, 7, 320, 8, 3), _layer(6, 7, 8, 72, 3), _layer(5, 5, 72, 128, 1), _layer(1, 1, 128, 136, 3),
                 _layer(10, 10, 136, 72, 3, stride=2), _layer(3, 3, 72, 8, 1), _layer(3, 3, 8, 64, 3, padding='VALID'), _layer(2, 2, 64, 264, 3, padding='BR1'),
                 _layer(5, 5, 264, 72, 1), _layer(4, 4, 72, 320, 3, padding='VALID'), _layer(1, 1, 320, 64, 1)]
WGRAD_GROUPS = [('vgg300', net_wgrad_layers('vgg300'), 3), ('vgg512', net_wgrad_layers('vgg512'), 2), ('12 layers', TWELVE_LAYERS, 2)]
THIRTEEN_LAYERS = TWELVE_LAYERS + [_layer(1, 1, 64, 64, 1)]


# ------------------------------------------------------------------------------------------------------------ the C structures
def c_stages(chain, ptr_of, wgt_of=None):
    """ssd_tail_stage[]: ptr_of(tensor name) -> address (or key), wgt_of(stage index) -> the filter mirror's address"""
    arr = (TailStage * len(chain.stages))()
    for i, s in enumerate(chain.stages):
        a = arr[i]
        a.hi, a.wi, a.ci, a.ho, a.wo, a.co, a.kh, a.kw, a.stride, a.dil, a.pad_h, a.pad_w = s.hi, s.wi, s.ci, s.ho, s.wo, s.co, s.k, s.k, s.stride, 1, s.ph, s.pw
        a.dgrad, a.relu, a.accum, a.out_f32 = int(s.dgrad), int(s.relu), int(s.accum), int(s.out_f32)
        a.src, a.dst = ptr_of(s.src), ptr_of(s.dst)
        a.mask = ptr_of(s.mask) if s.mask else None
        a.bias = ptr_of(('bias', i)) if s.bias else None
        a.wgt = wgt_of(i) if wgt_of else None
    return arr


def plan_of(chain):
    """-> (rc, [plan stage as a dict], lds_total); tensors are keyed by distinct integers, no GPU is opened"""
    keys = {}

    def key(name):
        return keys.setdefault(name, 0x1000 * (len(keys) + 1))
    arr = c_stages(chain, key)
    n = len(chain.stages)
    out = (TailPlanStage * n)()
    total = C.c_int(-1)
    rc = lib.ssd_op_tail_chain_plan(arr, n, out, C.byref(total))
    if rc != 0:
        return rc, None, None
    plan = []
    for p in out:
        d = {f: getattr(p, f) for f, _ in TailPlanStage._fields_ if f != 'tasks'}
        d['tasks'] = [(p.tasks[t][0], p.tasks[t][1]) for t in range(p.ntask)]
        plan.append(d)
    return rc, plan, total.value


# ------------------------------------------------------------------------------------------------------------ a live batch
def live_boxes(preset):
    """ground truth that gives EVERY map of the preset a positive anchor: per map one box of the map's own scale (its first, square box
    type) centred on one of its cells -- that anchor overlaps it fully.  -> (boxes [n, 4] cx cy w h, classes [n])"""
    boxes = []
    for (f, scale, _) in preset['maps']:
        c = (f // 2 + 0.5) / f
        boxes.append([c, c, scale, scale])
    return np.array(boxes, np.float64), np.arange(len(boxes)) % 20


def map_ranges(preset):
    """[(first anchor, end)] per map, in the anchor order map -> type -> row -> col"""
    out, a0 = [], 0
    for (f, _, ars) in preset['maps']:
        n = f * f * (len(ars) + 2)
        out.append((a0, a0 + n))
        a0 += n
    return out


def positives_per_map(y, preset, num_classes=20):
    """y [A, C + 5] (the label oracle's vector of one image) -> the number of positive anchors of each map"""
    pos = y[:, num_classes] == 0      # (the background indicator is column num_classes)
    return [int(np.count_nonzero(pos[a0:a1])) for a0, a1 in map_ranges(preset)]
