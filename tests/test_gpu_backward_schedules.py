"""-m gpu: one training step under every schedule backward can take (csrc/net.hip backward_step, backward_conv, backward_join), in
fp32 and in bf16 with its default fusions -- pool fusion 7 (conv1_1's weight gradient inside conv1_2's data gradient included) and
the tail chain both ways; fp32: Winograd 15, dual mode 1.  The reference handle runs the plain step with the weight gradients on
their own stream; a second handle with the same weights and inputs runs them on the main stream (ssd_set_overlap 0), or the
staged backward on torch's weight-gradient stream with ranges of at least 1M floats, the caller consuming them on that stream
(sync_main=False) or on the main stream (True).  The schedules issue the same deterministic kernels, so after each of two steps the
losses, the result and the three arenas must be BIT-identical.  vgg300 at batch 3 (odd: forward's lanes are uneven), and vgg512 at
batch 1 in bf16, whose seven maps give bw_class its other head count.  Like test_gpu_winograd_dual_step.py this would most likely
show a missing hand-off as differing bits and proves none absent: the hand-off table in net.hip carries the argument."""
import numpy as np
import pytest
import torch

from oracle import boxes as ob, ssdvgg_ref as ref
from step_state import make, state, assert_same

pytestmark = pytest.mark.gpu
STEPS = 2
MIN_FLOATS = 1_000_000


def step_plain(net, x, y):
    net.train_step_dev(x, y)


def step_staged(sync_main):
    def step(net, x, y):
        # the staged backward as parallel.train_step_dp drives it, without the collectives
        net.use_torch_wgrad_stream()
        net.forward_dev(x, y)
        ranges = list(net.backward_staged(y, x.shape[0], MIN_FLOATS, sync_main=sync_main))
        assert ranges == net.backward_ranges(MIN_FLOATS) and len(ranges) >= 4
        net.apply_gradients_dev()
    return step


@pytest.fixture(scope='module')
def cache():
    held = {}
    yield held
    held.clear()      # (the arenas' copies live on the GPU)


def reference(cache, preset_name, batch, dtype):
    """weights, batches and the plain step's state after every step: computed once per configuration, never written again"""
    key = (preset_name, batch, dtype)
    if key not in cache:
        preset = ob.get_preset(preset_name)
        w = ref.init_params(preset, 20, seed=6, alive=True)
        rng = np.random.default_rng(23)
        batches = [tuple(torch.from_numpy(a).cuda() for a in ref.synth_batch(rng, batch, preset)[:2]) for _ in range(STEPS)]
        sess, net = make(w, None, True, preset_name, batch, dtype)
        try:
            states = []
            for x, y in batches:
                step_plain(net, x, y)
                states.append(state(net, batch))
            assert float(states[-1]['grads'].abs().max()) > 0
        finally:
            sess.close()
        cache[key] = (w, batches, states)
    return cache[key]


def run_against_reference(cache, preset_name, batch, dtype, overlap, step):
    w, batches, want = reference(cache, preset_name, batch, dtype)
    sess, net = make(w, None, overlap, preset_name, batch, dtype)
    try:
        for i, (x, y) in enumerate(batches):
            step(net, x, y)
            assert_same(state(net, batch), want[i], f'step {i}')
        assert net.global_step == STEPS
    finally:
        sess.close()


@pytest.mark.parametrize('overlap,step', [(False, step_plain), (True, step_staged(False)), (True, step_staged(True))],
                         ids=['one-stream', 'staged', 'staged, sync_main'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_step_bit_identical_across_backward_schedules(cache, dtype, overlap, step):
    run_against_reference(cache, 'vgg300', 3, dtype, overlap, step)


def test_vgg512_bf16_staged_step_bit_identical_to_the_plain_step(cache):
    run_against_reference(cache, 'vgg512', 1, 'bf16', True, step_staged(False))
