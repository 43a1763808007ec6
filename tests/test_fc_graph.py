"""CPU: the fc graph (SSDVGG.build_from_vgg(a_trous=False), ssdvgg.py:210-228) -- arena sizes, the C ABI's new entry points,
the fc weights converter and the CPU restatement the GPU tests compare against (tests/fc_ref.py)."""
import numpy as np
import pytest
import torch

from oracle import boxes as ob
from oracle import ssdvgg_ref as ref
import fc_ref


def head_padding(pname, c7):
    """zero columns of the fused heads: widths rounded up to 8 channels (150 -> 152, 100 -> 104)"""
    preset = ob.get_preset(pname)
    fch = [512, c7, 512, 256, 256, 256, 256]
    pad = 0
    for i, (fk, s, ars) in enumerate(preset['maps']):
        w = (2 + len(ars)) * 25
        p = (w + 7) // 8 * 8 - w
        pad += 9 * fch[i] * p + p
    return pad


@pytest.mark.parametrize('pname', ['vgg300', 'vgg512'])
def test_arena_floats_graph(pname):
    from ssd_tensorflow_amd._lib import lib, last_error
    n = lib.ssd_arena_floats_graph(pname.encode(), 20, 1)
    assert n == fc_ref.REF_PARAMS[pname] + head_padding(pname, 4096)
    # the a-trous graph through the new entry point and the old one: what it always was
    a = lib.ssd_arena_floats(pname.encode(), 20)
    assert a == lib.ssd_arena_floats_graph(pname.encode(), 20, 0)
    assert a == {'vgg300': 26285486, 'vgg512': 26959300}[pname] + head_padding(pname, 1024)
    assert lib.ssd_arena_floats_graph(pname.encode(), 20, 2) == 0 and 'graph must be 0' in last_error()


def test_new_symbols_and_constants():
    from ssd_tensorflow_amd import _lib
    import os, re
    for n in ('ssd_arena_floats_graph', 'ssd_create_graph', 'ssd_graph'):
        assert hasattr(_lib.lib, n) and n in _lib.SIGNATURES
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ssdvgg_hip.h')).read()
    assert re.search(r'#define SSD_GRAPH_A_TROUS 0\b', hdr) and re.search(r'#define SSD_GRAPH_FC 1\b', hdr)
    assert len(_lib.SIGNATURES['ssd_create_graph'][1]) == 12


def fake_vgg(rng):
    vgg = {}
    for l in ref.VGG:
        if l != 'pool':
            vgg[l[0] + '/filter'] = rng.normal(0, 1, (3, 3, l[1], l[2])).astype(np.float32)
            vgg[l[0] + '/biases'] = rng.normal(0, 1, (l[2],)).astype(np.float32)
    for n, s in fc_ref.FC_VARS.items():
        vgg[n] = rng.normal(0, 1, s).astype(np.float32)
    return vgg


def test_vgg16_to_ssd_fc(tmp_path):
    from ssd_tensorflow_amd import weights
    vgg = fake_vgg(np.random.default_rng(0))
    out = weights.vgg16_to_ssd(vgg, a_trous=False)
    assert not any(k.startswith('mod_conv') for k in out)
    for n, s in fc_ref.FC_VARS.items():
        assert out[n].shape == s and np.array_equal(out[n], vgg[n])
    assert out['conv5_3/filter'].shape == (3, 3, 512, 512)
    # the whole trunk + fc variables of the fc graph, nothing else
    trunk = tuple(l[0] + '/' for l in ref.VGG if l != 'pool') + ('fc6/', 'fc7/')
    want = {k for k in fc_ref.param_shapes(ob.get_preset('vgg300')) if k.startswith(trunk)}
    assert set(out) == want
    # the default keeps the decimated a-trous variables
    at = weights.vgg16_to_ssd(vgg)
    assert at['mod_conv6/filter'].shape == (3, 3, 512, 1024) and 'fc6/weights' not in at
    weights.save_vgg_npz(str(tmp_path / 'vgg16_ssd_fc.npz'), vgg, a_trous=False)
    z = np.load(str(tmp_path / 'vgg16_ssd_fc.npz'))
    assert z['fc7/weights'].shape == (1, 1, 4096, 4096)
    bad = dict(vgg, **{'fc6/weights': vgg['fc6/weights'][:, :, :, :1024]})
    with pytest.raises(ValueError, match='fc6/weights'):
        weights.vgg16_to_ssd(bad, a_trous=False)


@pytest.mark.parametrize('pname', ['vgg300', 'vgg512'])
def test_fc_param_count(pname):
    shapes = fc_ref.param_shapes(ob.get_preset(pname))
    assert sum(int(np.prod(s)) for s in shapes.values()) == fc_ref.REF_PARAMS[pname]
    assert shapes['conv8_1/filter'] == (1, 1, 4096, 256) and shapes['classifiers/classifier1_0/filter'] == (3, 3, 4096, 25)
    assert 'mod_conv6/filter' not in shapes and 'mod_conv7/biases' not in shapes


def test_fc_cpu_restatement_forward():
    preset = ob.get_preset('vgg300')
    w = fc_ref.init_params(preset, seed=3)
    assert sum(v.size for v in w.values()) == fc_ref.REF_PARAMS['vgg300']
    rng = np.random.default_rng(0)
    x, y, _ = ref.synth_batch(rng, 1, preset)
    params = {k: torch.from_numpy(v) for k, v in w.items()}
    with torch.no_grad():
        out, result = fc_ref.forward(params, torch.from_numpy(x), preset)
        L = fc_ref.losses(out, torch.from_numpy(y), params)
    assert out.shape == (1, 8732, 25) and result.shape == (1, 8732, 25)
    assert torch.allclose(result[..., :21].sum(-1), torch.ones(1, 8732), atol=1e-5)
    # the L2 term counts the fc filters, which oracle.l2_term (every '*/filter') misses
    fc = sum(float((params[n].double() ** 2).sum()) / 2 for n in ('fc6/weights', 'fc7/weights'))
    assert fc > 0
    assert abs(float(L['l2']) - 0.0005 * (float(ref.l2_term(params)) + fc)) < 1e-4 * float(L['l2'])
    assert abs(float(L['total']) - float(L['l2']) - float(L['confidence']) - float(L['localization'])) < 1e-4 * float(L['total'])


def test_build_from_vgg_fc_reads_the_fc_npz(tmp_path, monkeypatch):
    """build_from_vgg(a_trous=False) asks for <vgg_dir>/vgg16_ssd_fc.npz (checked without a GPU by stopping at _create)."""
    from ssd_tensorflow_amd.ssdvgg import SSDVGG
    seen = {}

    def fake_create(self, num_classes, max_batch, training, seed, dtype='f32', a_trous=True):
        seen['a_trous'] = a_trous
        raise RuntimeError('stop')

    monkeypatch.setattr(SSDVGG, '_create', fake_create)
    net = SSDVGG(None, 'vgg300')
    with pytest.raises(RuntimeError, match='stop'):
        net.build_from_vgg(str(tmp_path), 20, a_trous=False)
    assert seen['a_trous'] is False
