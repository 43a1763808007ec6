"""CPU: the host's plan of a multi-stage tail-chain launch (csrc/tail_bf16.hip plan_chain, through ssd_op_tail_chain_plan), checked
from the returned plan alone against liveness recomputed here.

What a plan must guarantee for the kernel to be right (tail_chain_bf16_kernel reads nothing else): feature maps that are live in the
same stage never share LDS bytes, nothing touches the row of zeros a tap outside the image reads, a stage's k-split scratch lies
clear of everything live while it is written, a consumer gathers from exactly the bytes its producer wrote, a tensor is loaded from
global memory exactly when no earlier stage left it in LDS, and the tasks of a stage cover its (n block, pixel group, k range)
product exactly once.  The lists are tests/tail_cases.py: the nets' own launches, lists built for what those do not reach, and lists
the planner must refuse.

Mutations of the planner this file caught (each a one-line edit of a scratch copy, one library per edit, this file run against it):
  `in->last = i` dropped (a tensor's region is free again behind the stage that loaded or produced it)
        test_regions_of_a_stage_do_not_overlap [every list], test_scratch_is_clear_of_everything_live [most lists]
  `scratch_off` fixed at TAIL_ZERO_BYTES
        test_scratch_is_clear_of_everything_live [every list]
and a bug it found: the output of a stage that writes (in global memory) over a tensor whose last reader has run was sent to that
tensor's dead LDS region, by then another tensor's bytes -- test_consumers_read_where_producers_wrote_and_loads_are_exact
[output over a dead input]; the planner now keeps an output in LDS only while its region is live.
The kernel-side mutations, and the whole table, are recorded in test_gpu_tail_chain.py."""
import pytest

from oracle import boxes as ob
import tail_cases as tc
from ssd_tensorflow_amd._lib import (last_error, TAIL_ZERO_BYTES, TAIL_LDS_MAX, TF_RELU, TF_ACCUM, TF_OUT_F32, TF_LOAD_IN, TF_LOAD_OUT,
                                     TF_KTAIL)

IDS = [c.name for c in tc.ALL_CHAINS]


@pytest.fixture(scope='module')
def plans():
    out = {}
    for ch in tc.ALL_CHAINS:
        rc, plan, total = tc.plan_of(ch)
        assert rc == 0, f'{ch.name}: {last_error()}'
        out[ch.name] = (plan, total)
    return out


def liveness(ch):
    """{tensor: (first, last)} of the tensors a launch keeps in LDS, recomputed from the stage list: a tensor is live from the stage
    that loads or produces it to the last stage that gathers from it or accumulates into it.  An output nobody reads later, and an
    fp32 output, is written to global memory only."""
    live = {}
    for i, s in enumerate(ch.stages):
        if s.src in live:
            live[s.src] = (live[s.src][0], i)
        else:
            live[s.src] = (i, i)
        if s.out_f32:
            continue
        later = any(t.src == s.dst or (t.dst == s.dst and t.accum) for t in ch.stages[i + 1:])
        if s.dst in live and s.accum:
            live[s.dst] = (live[s.dst][0], i)
        elif s.accum or later:
            assert s.dst not in live, 'a well-formed list never overwrites an LDS-resident tensor'
            live[s.dst] = (i, i)
    return live


def regions(ch, plan):
    """{tensor: (offset, bytes)} as the plan reports them, every report of one tensor agreeing"""
    reg = {}
    for s, p in zip(ch.stages, plan):
        for name, off, nbytes in ((s.src, p['in_off'], p['in_bytes']), (s.dst, p['out_off'], p['out_bytes'])):
            if off < 0:
                continue
            assert reg.setdefault(name, (off, nbytes)) == (off, nbytes), f'{name} moved: {reg[name]} -> {(off, nbytes)}'
    return reg


def overlap(a, b):
    return a[0] < b[0] + b[1] and b[0] < a[0] + a[1]


@pytest.mark.parametrize('ch', tc.ALL_CHAINS, ids=IDS)
def test_every_live_tensor_has_a_region_of_its_size(ch, plans):
    plan, total = plans[ch.name]
    live, reg = liveness(ch), regions(ch, plan)
    assert set(reg) == set(live), 'the tensors kept in LDS are the ones a later stage needs'
    for name, (off, nbytes) in reg.items():
        h, w, c, kind = ch.tensors[name]
        assert kind == 'bf16' and nbytes == h * w * (c * 2 + 16) + 256, f'{name}: pixel rows at pitch SC*2+16, + 256'
        assert off % 16 == 0 and off >= TAIL_ZERO_BYTES, f'{name} touches the zero row'
        assert off + nbytes <= total <= TAIL_LDS_MAX
    for s, p in zip(ch.stages, plan):
        if p['out_off'] < 0:
            assert s.dst not in live or live[s.dst][1] < ch.stages.index(s), f'{s.dst} is needed later but not kept'


@pytest.mark.parametrize('ch', tc.ALL_CHAINS, ids=IDS)
def test_regions_of_a_stage_do_not_overlap(ch, plans):
    plan, total = plans[ch.name]
    live, reg = liveness(ch), regions(ch, plan)
    for i in range(len(ch.stages)):
        now = [n for n, (a, b) in live.items() if a <= i <= b]
        for x in range(len(now)):
            for y in range(x + 1, len(now)):
                assert not overlap(reg[now[x]], reg[now[y]]), f'stage {i}: {now[x]} {reg[now[x]]} and {now[y]} {reg[now[y]]} share LDS'


@pytest.mark.parametrize('ch', tc.ALL_CHAINS, ids=IDS)
def test_scratch_is_clear_of_everything_live(ch, plans):
    plan, total = plans[ch.name]
    live, reg = liveness(ch), regions(ch, plan)
    for i, p in enumerate(plan):
        assert p['scratch_bytes'] == (p['ksplit'] - 1) * p['tiles'] * 4 * 64 * 4 * 4, 'one 16x64 fp32 tile x 4 pixel blocks per parked task'
        if p['scratch_bytes'] == 0:
            continue
        sc = (p['scratch_off'], p['scratch_bytes'])
        assert sc[0] % 16 == 0 and sc[0] >= TAIL_ZERO_BYTES and sc[0] + sc[1] <= total <= TAIL_LDS_MAX
        for n, (a, b) in live.items():
            if a <= i <= b:
                assert not overlap(sc, reg[n]), f'stage {i}: scratch {sc} over {n} {reg[n]}'


@pytest.mark.parametrize('ch', tc.ALL_CHAINS, ids=IDS)
def test_consumers_read_where_producers_wrote_and_loads_are_exact(ch, plans):
    plan, total = plans[ch.name]
    live = liveness(ch)
    where = {}      # tensor -> offset of the stage that loaded or produced it
    for i, (s, p) in enumerate(zip(ch.stages, plan)):
        f = p['flags']
        assert bool(f & TF_RELU) == s.relu and bool(f & TF_ACCUM) == s.accum and bool(f & TF_OUT_F32) == s.out_f32
        sc = s.co if s.dgrad else s.ci
        assert bool(f & TF_KTAIL) == (sc % 128 != 0)
        resident = s.src in where
        assert bool(f & TF_LOAD_IN) == (not resident), f'stage {i}: TF_LOAD_IN exactly when no earlier stage left {s.src} in LDS'
        if resident:
            assert p['in_off'] == where[s.src], f'stage {i} gathers {s.src} from {p["in_off"]}, it was written at {where[s.src]}'
        where[s.src] = p['in_off']
        out_resident = s.dst in where
        assert bool(f & TF_LOAD_OUT) == (s.accum and not out_resident), f'stage {i}: TF_LOAD_OUT'
        if s.accum:
            assert p['out_off'] >= 0
            if out_resident:
                assert p['out_off'] == where[s.dst], f'stage {i} accumulates into {s.dst} at {p["out_off"]}, it lies at {where[s.dst]}'
        if p['out_off'] >= 0:
            where[s.dst] = p['out_off']
        assert (p['out_off'] >= 0) == (s.dst in live and live[s.dst][0] <= i <= live[s.dst][1])
        # (the pitch: in_bytes / out_bytes are pixels x (channels * 2 + 16) + 256, asserted per tensor above)


@pytest.mark.parametrize('ch', tc.ALL_CHAINS, ids=IDS)
def test_tasks_cover_a_stage_exactly_once(ch, plans):
    plan, total = plans[ch.name]
    for i, (s, p) in enumerate(zip(ch.stages, plan)):
        M, dn, sc = (s.hi * s.wi, s.ci, s.co) if s.dgrad else (s.ho * s.wo, s.co, s.ci)
        nblk_n, nblk_m = -(-dn // 16), -(-M // 16)
        ngrp_m = -(-nblk_m // 4)
        assert p['gpt'] == -(-(-(-sc // 32)) // 4) and p['ngroups'] == s.k * s.k * p['gpt']
        assert p['tiles'] == nblk_n * ngrp_m and p['ntask'] == p['tiles'] * p['ksplit'] and 1 <= p['ksplit'] <= 4
        assert p['ntask'] <= 64 and (p['ksplit'] == 1 or p['ntask'] <= 16), 'a k split meets behind ONE barrier: one task per wave'
        seen, ranges = set(), {}
        for t, (a, b) in enumerate(p['tasks']):
            nb, mg, ks, nmb = a & 255, (a >> 8) & 255, (a >> 16) & 255, a >> 24
            g0, g1 = b & 0xFFFF, b >> 16
            assert nb < nblk_n and mg < ngrp_m and ks < p['ksplit']
            assert (nb, mg, ks) not in seen, f'stage {i}: task {(nb, mg, ks)} twice'
            seen.add((nb, mg, ks))
            assert g0 < g1 <= p['ngroups'], f'stage {i}, task {t}: k groups [{g0}, {g1}) of {p["ngroups"]}'
            assert nmb == min(4, nblk_m - 4 * mg), f'stage {i}: {nmb} pixel blocks in group {mg} of {M} pixels'
            assert t == ks * p['tiles'] + mg * nblk_n + nb, 'the splits of one tile are `tiles` apart in task order (the kernel finds its scratch by that)'
            ranges.setdefault((nb, mg), {})[ks] = (g0, g1)
        assert len(seen) == nblk_n * ngrp_m * p['ksplit']
        for tile, r in ranges.items():
            edge = 0
            for ks in range(p['ksplit']):
                assert r[ks][0] == edge, f'stage {i}, tile {tile}: split {ks} starts at {r[ks][0]}, the one before ended at {edge}'
                edge = r[ks][1]
            assert edge == p['ngroups']


def test_the_lists_reach_what_they_were_built_for(plans):
    """the cases are what tail_cases.py says they are (a planner change that moves a threshold must not silently empty them)"""
    by = {c.name: c for c in tc.ALL_CHAINS}
    assert [len(c.stages) for c in tc.NET_CHAINS] == [9, 9, 8, 8, 9, 9, 8, 8]
    plan, total = plans['16 stages on 6x7']
    assert len(plan) == 16
    assert {p['ksplit'] for p in plan} == {1, 2, 3, 4}
    assert any(a['ntask'] > 16 and b['ntask'] < 16 for a, b in zip(plan, plan[1:])), 'more than 16 tasks, then fewer'
    assert any(a['ntask'] < b['ntask'] for a, b in zip(plan, plan[1:])) and any(a['ntask'] > b['ntask'] for a, b in zip(plan, plan[1:]))
    assert all(a['tiles'] != b['tiles'] for a, b in zip(plan, plan[1:])), 'every boundary changes the filter stream\'s step'
    assert any(p['flags'] & TF_KTAIL and p['in_bytes'] == 42 * 160 + 256 for p in plan) and any(p['ntask'] == 4 and p['ksplit'] == 4 for p in plan)
    # reuse: a region taken again by another tensor after its last reader
    for name in ('regions freed and reused', 'reuse under a KTAIL input after a tenant near the top of the bf16 range'):
        ch = by[name]
        reg, live = regions(ch, plans[name][0]), liveness(ch)
        assert any(overlap(reg[x], reg[y]) and live[x][1] < live[y][0] for x in reg for y in reg if x != y), name
    ch = by['reuse under a KTAIL input after a tenant near the top of the bf16 range']
    reg = regions(ch, plans[ch.name][0])
    assert reg['t2'][0] == reg['t0'][0] and reg['t2'][1] < reg['t0'][1] and plans[ch.name][0][2]['flags'] & TF_KTAIL
    # far readers: live across at least three other stages
    live = liveness(by['a tensor read by stage 1 and by the last stage'])
    assert live['t1'] == (0, 6) and live['t0'] == (0, 4)
    # accumulate into an LDS-resident tensor two stages after it was written; TF_LOAD_OUT without TF_LOAD_IN
    plan = plans['accumulate into an LDS-resident gradient, stride-2 data gradient'][0]
    assert plan[3]['flags'] & TF_ACCUM and not plan[3]['flags'] & (TF_LOAD_OUT | TF_LOAD_IN) and plan[3]['out_off'] == plan[0]['out_off']
    assert plan[5]['flags'] & TF_LOAD_OUT and not plan[5]['flags'] & TF_LOAD_IN
    # pixel blocks per task 1 .. 4, two pixel groups
    nmbs = {a >> 24 for n in ('maps of 100, 25, 9 and 1 pixels', '16 stages on 6x7') for p in plans[n][0] for a, _ in p['tasks']}
    assert nmbs == {1, 2, 3, 4}
    assert any(((a >> 8) & 255) == 1 for p in plans['maps of 100, 25, 9 and 1 pixels'][0] for a, _ in p['tasks'])
    assert any(p['flags'] & TF_OUT_F32 for p in plans['fp32-output heads between bf16 stages'][0])


@pytest.mark.parametrize('ch,text', tc.REFUSED_CHAINS, ids=[c.name for c, _ in tc.REFUSED_CHAINS])
def test_refused_lists(ch, text):
    rc, plan, total = tc.plan_of(ch)
    assert rc != 0 and text in last_error(), last_error()


@pytest.mark.parametrize('pname', ['vgg300', 'vgg512'])
def test_live_boxes_give_every_map_a_positive_anchor(pname):
    """the precondition of test_gpu_tail's live case, on the label oracle alone"""
    preset = ob.get_preset(pname)
    g, c = tc.live_boxes(preset)
    y = ob.encode_labels(g, c, preset, 20)
    pos = tc.positives_per_map(y, preset)
    assert len(pos) == len(preset['maps']) and min(pos) >= 1, pos
    assert tc.map_ranges(preset)[-1][1] == preset['num_anchors'] == y.shape[0]
