"""-m gpu: the MULTI-STAGE code of the bf16 tail (csrc/tail_bf16.hip tail_chain_bf16_kernel, tail_pack_kernel; conv_bf16.hip
conv_wgrad_group_bf16_kernel), which the one-stage entry points never run: a stage's epilogue writing its output into the LDS region
the next stage gathers from, the host's LDS plan with several regions (tests/test_tail_plan.py checks the plan itself), an
accumulate into an LDS-resident tensor, the k-split scratch above whatever is live, the hand-over of the filter stream across a
stage boundary (prime_next / primed), and the prefix tables that map a workgroup to its layer.

The reference is the SAME kernel one stage per launch (ssd_op_conv2d_fwd_bf16_chain / ssd_op_conv2d_dgrad_bf16_chain, pinned value for
value against exact arithmetic by test_gpu_conv_exact.py::test_bf16_chain_exact and against the oracle by test_gpu_tail.py), on
copies of the same buffers.  The results must be BIT-IDENTICAL, and so there is no tolerance anywhere in this file: a stage's task
plan and summation order depend on its own geometry only, and an accumulate adds the same rounded bf16 values whether they come
from LDS or from global memory.  The grouped weight gradient is compared in the same way with ssd_op_conv2d_wgrad_bf16_direct per
layer.  The stage lists are tests/tail_cases.py.

That these tests can fail -- one-line edits of a scratch copy of the sources, one library each, this file (and test_tail_plan.py)
run against it; nothing of them is committed:
  edit                                                       caught by
  ---------------------------------------------------------  -----------------------------------------------------------------------
  epilogue's LDS write at the wrong pitch (out_pitch - 16)   test_chain_is_bit_identical... : every list
  `in->last = i` dropped (planner)                           test_chain_is_bit_identical... : every list; test_tail_plan.py
                                                             test_regions_of_a_stage_do_not_overlap, test_scratch_is_clear...
  `scratch_off` fixed at TAIL_ZERO_BYTES (planner)           test_chain_is_bit_identical... : every list; test_tail_plan.py
                                                             test_scratch_is_clear_of_everything_live
  prime_next takes the task of stage s, not s + 1            test_chain_is_bit_identical... : every list
  `>=` -> `>` in tail_pack_kernel's prefix lookup            test_chain_is_bit_identical... : every list (one-stage launches pack n = 1
                                                             filter and never run the lookup: the reference stays right)
  `>=` -> `>` in conv_wgrad_group_bf16_kernel's lookup       test_grouped_weight_gradient_is_bit_identical... : all 6 cases
  the accumulate reads dst from global memory, not LDS       NOT caught, and no list can: the epilogue that wrote the LDS copy wrote the
                                                             same rounded bf16 values to global memory (or TF_LOAD_OUT copied them
                                                             from there), so the edit changes where equal bits are read, and only a
                                                             store still in flight could tell -- it did not, also not with the
                                                             accumulate right behind the producer ('accumulate right behind the
                                                             producer', added for this edit and kept for the plan it exercises).
(The edits that make a workgroup read or write at another layer's offsets were run with slack behind the op's filter store and with
the filters of a list in one allocation -- filter_arena -- so that the wrong addresses stayed inside allocations.)

A bug these lists found, in the planner: a stage may write its output, in global memory only, over a tensor whose last reader has
run (the launch's own input, say).  The planner looked the output's LDS region up by pointer alone, found the dead region -- whose
bytes by then belonged to another tensor, in the list 'output over a dead input' to the stage's own INPUT -- and the epilogue wrote
the output over pixels other waves were still gathering.  Caught by test_chain_is_bit_identical...[output over a dead input] and
by test_tail_plan.py::test_consumers_read_where_producers_wrote_and_loads_are_exact; an output now goes to LDS only while its
region is live.  The nets' own lists never did this: their plans are unchanged.
"""
import pytest
import torch

import tail_cases as tc
from gpu_util import lib, check, ptr
from ssd_tensorflow_amd._lib import last_error, WgradItem

pytestmark = pytest.mark.gpu
SENTINEL = -7.0


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def make_buffers(ch, seed):
    """-> (tensors by name incl. ('bias', stage), filter mirrors by stage), on the host: inputs Gaussian (or near the top of the bf16
    range), everything a stage writes filled with a sentinel; filters scaled so that activations stay O(1) through 16 stages"""
    g = torch.Generator().manual_seed(seed)
    inputs = set(ch.inputs())
    t = {}
    for name, (h, w, c, kind) in ch.tensors.items():
        shape = (ch.b, h, w, c)
        if name in ch.poison:
            v = (torch.randint(0, 2, shape, generator=g) * 2 - 1) * (1 + torch.rand(shape, generator=g)) * 2.0 ** 126
        elif name in inputs:
            v = torch.randn(shape, generator=g)
        else:
            v = torch.full(shape, SENTINEL)
        t[name] = v.to(torch.float32 if kind == 'f32' else torch.bfloat16)
        assert bool(torch.isfinite(t[name]).all())
    wgt = []
    for i, s in enumerate(ch.stages):
        kk = s.k * s.k
        if s.src in ch.poison:      # +-{1, 2, 3} x 2^-126: normal bf16 numbers, products of a few units
            w = (torch.randint(0, 2, (kk, s.ci, s.co), generator=g) * 2 - 1) * torch.randint(1, 4, (kk, s.ci, s.co), generator=g) * 2.0 ** -126
        else:
            w = torch.randn((kk, s.ci, s.co), generator=g) * (2.0 / (kk * (s.co if s.dgrad else s.ci))) ** 0.5
        # forward: the [tap][Co][Ci] mirror, data gradient: [tap][Ci][Co]
        wgt.append((w if s.dgrad else w.transpose(1, 2)).contiguous().to(torch.bfloat16))
        if s.bias:
            t[('bias', i)] = torch.randn((s.co,), generator=g) * 0.1
    return t, wgt


def filter_arena(wgt_h):
    """the stages' filter mirrors in ONE device allocation, back to back (as the step keeps its mirrors), with 256 KB behind the last:
    a pack workgroup mapped to the wrong layer (the prefix-lookup mutation) then reads a neighbour's filter, not unmapped memory"""
    flat = torch.cat([w.reshape(-1) for w in wgt_h] + [torch.zeros(128 * 1024, dtype=torch.bfloat16)]).cuda()
    out, o = [], 0
    for w in wgt_h:
        out.append(flat[o:o + w.numel()].view(w.shape))
        o += w.numel()
    return out


def run_chain(ch, t, wgt):
    arr = tc.c_stages(ch, lambda n: ptr(t[n]), lambda i: ptr(wgt[i]))
    rc = lib.ssd_op_tail_chain_bf16(arr, len(ch.stages), ch.b, None)
    torch.cuda.synchronize()
    return rc


def run_stage_by_stage(ch, t, wgt):
    for i, s in enumerate(ch.stages):
        geom = (ch.b, s.hi, s.wi, s.ci, s.ho, s.wo, s.co, s.k, s.k, s.stride, 1, s.ph, s.pw)
        if s.dgrad:
            check(lib.ssd_op_conv2d_dgrad_bf16_chain(ptr(t[s.src]), ptr(wgt[i]), ptr(t[s.dst]), ptr(t[s.mask]) if s.mask else None, int(s.accum), *geom, None))
        else:
            check(lib.ssd_op_conv2d_fwd_bf16_chain(ptr(t[s.src]), ptr(wgt[i]), ptr(t[('bias', i)]) if s.bias else None, ptr(t[s.dst]), int(s.out_f32),
                                                   *geom, int(s.relu), None))
    torch.cuda.synchronize()


@pytest.mark.parametrize('ch', tc.ALL_CHAINS, ids=[c.name for c in tc.ALL_CHAINS])
def test_chain_is_bit_identical_to_its_stages_one_per_launch(ch):
    host, wgt_h = make_buffers(ch, 1234 + len(ch.stages))
    wgt = filter_arena(wgt_h)
    a = {k: v.cuda() for k, v in host.items()}
    b = {k: v.cuda() for k, v in host.items()}
    check(run_chain(ch, a, wgt))
    run_stage_by_stage(ch, b, wgt)
    written = {s.dst for s in ch.stages}
    for name in ch.tensors:
        got, want = a[name].cpu(), b[name].cpu()
        if name not in written:
            assert torch.equal(bits(got), bits(host[name])), f'{name} is an input: the launch must not write it'
            continue
        assert bool(torch.isfinite(want.float()).all()), f'{name}: the one-stage launches themselves are not finite'
        assert bool(torch.isfinite(got.float()).all()), f'{name}: Inf / NaN out of the chain'
        assert not torch.equal(bits(want), bits(host[name])), f'{name} was not written'
        diff = bits(got) != bits(want)
        n = int(diff.sum())
        if n:
            idx = torch.nonzero(diff)[:5].tolist()
            pytest.fail(f'{ch.name}: {name} differs from the one-stage launches in {n} of {diff.numel()} elements, first at (image, row, col, channel) {idx}: '
                        f'{[float(got[tuple(i)]) for i in idx]} vs {[float(want[tuple(i)]) for i in idx]}')


@pytest.mark.parametrize('ch,text', tc.REFUSED_CHAINS, ids=[c.name for c, _ in tc.REFUSED_CHAINS])
def test_refused_lists_leave_their_outputs_alone(ch, text):
    host, wgt_h = make_buffers(ch, 99)
    wgt = filter_arena(wgt_h)
    a = {k: v.cuda() for k, v in host.items()}
    assert run_chain(ch, a, wgt) != 0 and text in last_error(), last_error()
    for name in a:
        assert torch.equal(bits(a[name].cpu()), bits(host[name])), f'{name} changed although the launch was refused'


def wgrad_buffers(layers, b, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for L in layers:
        kk = L.k * L.k
        out.append(dict(x=torch.randn((b, L.hi, L.wi, L.ci), generator=g).to(torch.bfloat16).cuda(),
                        dy=torch.randn((b, L.ho, L.wo, L.co), generator=g).to(torch.bfloat16).cuda(),
                        w=torch.randn((kk, L.ci, L.co), generator=g).cuda()))
    return out


def wgrad_outputs(layers):
    return [dict(dw=torch.full((L.k * L.k, L.ci, L.co), SENTINEL, device='cuda'), db=torch.full((L.co,), SENTINEL, device='cuda')) for L in layers]


def wgrad_items(layers, bufs, outs):
    arr = (WgradItem * len(layers))()
    for a, L, i, o in zip(arr, layers, bufs, outs):
        a.hi, a.wi, a.ci, a.ho, a.wo, a.co, a.kh, a.kw, a.stride, a.dil, a.pad_h, a.pad_w = L.hi, L.wi, L.ci, L.ho, L.wo, L.co, L.k, L.k, L.stride, 1, L.ph, L.pw
        a.x, a.dy, a.dw, a.dbias, a.w = ptr(i['x']), ptr(i['dy']), ptr(o['dw']), ptr(o['db']), ptr(i['w'])
    return arr


@pytest.mark.parametrize('wd', [0.0005, 0.0])
@pytest.mark.parametrize('name,layers,b', tc.WGRAD_GROUPS, ids=[g[0] for g in tc.WGRAD_GROUPS])
def test_grouped_weight_gradient_is_bit_identical_to_one_launch_per_layer(name, layers, b, wd):
    bufs = wgrad_buffers(layers, b, 7)
    grouped, single = wgrad_outputs(layers), wgrad_outputs(layers)
    check(lib.ssd_op_conv2d_wgrad_group_bf16(wgrad_items(layers, bufs, grouped), len(layers), wd, b, None))
    for L, i, o in zip(layers, bufs, single):
        check(lib.ssd_op_conv2d_wgrad_bf16_direct(ptr(i['x']), ptr(i['dy']), ptr(o['dw']), ptr(o['db']), ptr(i['w']), wd, b, L.hi, L.wi, L.ci, L.ho, L.wo,
                                                  L.co, L.k, L.k, L.stride, 1, L.ph, L.pw, None))
    torch.cuda.synchronize()
    for k, (L, got, want) in enumerate(zip(layers, grouped, single)):
        for key in ('dw', 'db'):
            g_, w_ = got[key].cpu(), want[key].cpu()
            assert bool(torch.isfinite(g_).all()) and not bool((w_ == SENTINEL).any()), f'layer {k} {key}: the one-layer launch left a sentinel'
            n = int((bits(g_) != bits(w_)).sum())
            assert n == 0, f'{name}, layer {k} {tuple(L)}: {key} differs from the one-layer launch in {n} of {g_.numel()} elements'


def test_grouped_weight_gradient_refuses_thirteen_layers():
    layers = tc.THIRTEEN_LAYERS
    bufs, outs = wgrad_buffers(layers, 1, 8), wgrad_outputs(layers)
    assert lib.ssd_op_conv2d_wgrad_group_bf16(wgrad_items(layers, bufs, outs), len(layers), 0.0005, 1, None) != 0
    assert '1..12 layers (got 13)' in last_error(), last_error()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o['dw'] == SENTINEL).all()) and bool((o['db'] == SENTINEL).all())
