"""-m gpu: the fp32 training step with ONE transform of dy per Winograd layer in backward (csrc/net.hip wgrad_handoff: the main stream
runs the dual kernel into wino_yt_ and one of two Ya buffers, the weight-gradient stream waits for it) against the step with one
transform per gradient (ssd_set_wino_dual(h, 0)): mode 2 takes the one transform on EVERY layer with both Winograd gradients, mode 1 on
the layers of the default shape rule.  Two vgg300 handles, the same weights and inputs, three steps.  Losses, result and
the three arenas must be BIT-identical after every step -- with the weight gradients on their own stream, on the main stream
(ssd_set_overlap 0), and through the staged backward with ranges small enough that several stages are returned.  Batch 3: odd, so
forward's two lanes are uneven.  A race on a scratch buffer would most likely show as differing bits here, but no test proves it
absent: DESIGN.md 4.9 carries the ordering argument."""
import numpy as np
import pytest
import torch

from oracle import boxes as ob, ssdvgg_ref as ref
from step_state import make, state, assert_same

pytestmark = pytest.mark.gpu
B, STEPS = 3, 3


@pytest.fixture(scope='module')
def data():
    preset = ob.get_preset('vgg300')
    w = ref.init_params(preset, 20, seed=6, alive=True)
    rng = np.random.default_rng(23)
    batches = [ref.synth_batch(rng, B, preset)[:2] for _ in range(STEPS)]
    return w, [(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()) for x, y in batches]


def step_plain(net, x, y):
    net.train_step_dev(x, y)


def step_staged(net, x, y):
    # the staged backward as parallel.train_step_dp drives it, without the collectives: ranges of at least 1M floats
    net.use_torch_wgrad_stream()
    net.forward_dev(x, y)
    ranges = list(net.backward_staged(y, B, 1_000_000, sync_main=False))
    assert len(ranges) >= 4 and ranges == net.backward_ranges(1_000_000)
    net.apply_gradients_dev()


@pytest.mark.parametrize('mode,overlap,step', [(2, True, step_plain), (1, True, step_plain), (2, False, step_plain), (2, True, step_staged)],
                         ids=['overlap', 'overlap, shape rule', 'one-stream', 'staged'])
def test_step_bit_identical_with_and_without_the_dual_transform(data, mode, overlap, step):
    w, batches = data
    sess1, dual = make(w, mode, overlap)
    sess2, two = make(w, 0, overlap)
    try:
        for i, (x, y) in enumerate(batches):
            step(dual, x, y)
            step(two, x, y)
            assert_same(state(dual), state(two), f'step {i}')
        assert dual.global_step == STEPS
        assert float(dual.grads_flat.abs().max()) > 0
    finally:
        sess1.close(); sess2.close()
