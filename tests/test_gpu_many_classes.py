"""-m gpu: more than 27 classes (up to the library's 127) through every layer: the label encoder, decode + NMS (the wide
scan and the 128-class per-image tables), the wide heads / loss kernel and the loss gradient on wider tiles, training
and inference drivers.  Pinned to the reference at 80 classes (g11 / g12, tools/make_golden.py) and to the oracle
elsewhere; 27 and 28 classes sit on both sides of the kernel switch."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import boxes as ob
from oracle import ssdvgg_ref as ref
from oracle import average_precision as oap
from golden_util import load
from gpu_util import max_rel, rel_err
from ssd_tensorflow_amd import ssdutils as su
from ssd_tensorflow_amd._lib import lib, check, np_ptr
from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session

pytestmark = pytest.mark.gpu
PRESETS = ['vgg300', 'vgg512']
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3
TOL_BF = 4e-3
WD = 0.0005


def dense_pred_c(d, pi):
    """[A, C+5] from a sparse g11 record: rows not stored are pure background."""
    A, C = int(d['A'][0]), int(d['num_classes'][0])
    row = np.zeros(C + 5, np.float32); row[C] = 1
    pred = np.tile(row, (A, 1))
    pred[d[f'predrows_{pi}']] = d[f'predvals_{pi}']
    return pred


def cases(d):
    for pi in range(int(d['npred'][0])):
        for si in range(int(d['nset'][0])):
            tag = f'{pi}_{si}'
            if f'set_{tag}' in d.files:
                thr, cap, mo = d[f'set_{tag}']
                yield pi, tag, float(thr), (None if cap < 0 else int(cap)), (None if mo < 0 else int(mo))


def random_gt(rng, n_img, C, nmax=8):
    gts, cls = [], []
    for _ in range(n_img):
        n = int(rng.integers(0, nmax + 1))
        w = rng.uniform(0.02, 0.9, n); h = rng.uniform(0.02, 0.9, n)
        gts.append(np.stack([rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2), w, h], 1).reshape(-1, 4))
        c = rng.integers(0, C, n)
        if n:
            c[0] = C - 1
        cls.append(c)
    return gts, cls


def softmax_pred(rng, b, A, C, n_hot=60, run=6):
    logits = rng.normal(0, 1, (b, A, C + 1)).astype(np.float32)
    logits[:, :, C] += 4
    for i in range(b):
        hot = rng.choice(A - run, n_hot, replace=False)
        cl = rng.integers(0, C, n_hot)
        for k in range(run):
            logits[i, hot + k, cl] += 8 + rng.normal(0, 1, n_hot)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return np.concatenate([e / e.sum(-1, keepdims=True), rng.normal(0, 0.1, (b, A, 4))], -1).astype(np.float32)


# ---- labels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pname', PRESETS)
def test_labels_c80_golden(pname):
    g = load(f'g12_labels_c80_{pname}.npz')
    C, n = int(g['num_classes'][0]), int(g['ncases'][0])
    preset = su.get_preset_by_name(pname)
    gts, cls = [g[f'gt_{i}'] for i in range(n)], [g[f'cls_{i}'] for i in range(n)]
    vec = su.encode_labels_batch(preset, C, gts, cls)
    dvec = su.encode_labels_batch_dev(preset, C, gts, cls).cpu().numpy()
    assert vec.shape == (n, preset.num_anchors, C + 5) and np.array_equal(vec, dvec)
    for ci in range(n):
        pos = np.nonzero(vec[ci, :, C] == 0)[0]
        assert np.array_equal(pos, g[f'pos_{ci}']), f'case {ci}: positive anchor set'
        rows, want = vec[ci][pos], g[f'rows_{ci}']
        assert np.array_equal(rows[:, :C + 1], want[:, :C + 1]), f'case {ci}: classes'
        assert np.allclose(rows[:, C + 1:], want[:, C + 1:], rtol=2e-7, atol=1e-7), f'case {ci}: offsets'
        neg = np.ones(preset.num_anchors, bool); neg[pos] = False
        assert np.all(vec[ci][neg, C] == 1) and not vec[ci][neg, :C].any() and not vec[ci][neg, C + 1:].any()


@pytest.mark.parametrize('pname', PRESETS)
@pytest.mark.parametrize('C', [27, 28, 80, 127])
def test_labels_random_vs_oracle(pname, C):
    rng = np.random.default_rng(C)
    preset = su.get_preset_by_name(pname); op = ob.get_preset(pname)
    anch = ob.anchors(op); aabs = ob.anchors_abs(anch)
    gts, cls = random_gt(rng, 6, C)
    vec = su.encode_labels_batch(preset, C, gts, cls)
    for i in range(len(gts)):
        want = ob.encode_labels(gts[i], cls[i], op, C, anch, aabs)
        assert np.array_equal(vec[i][:, :C + 1], want[:, :C + 1]), f'image {i}: class columns'
        assert np.allclose(vec[i][:, C + 1:], want[:, C + 1:], rtol=2e-7, atol=1e-7)


# ---- decode + NMS ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pname', PRESETS)
def test_detect_c80_golden(pname):
    g = load(f'g11_detect_c80_{pname}.npz')
    preset = su.get_preset_by_name(pname)
    n = 0
    for pi, tag, thr, cap, max_out in cases(g):
        pred = dense_pred_c(g, pi)
        before = pred.copy()
        dec = su.detect_batch(pred, preset, thr, cap, None, nms=False)[0]
        assert np.array_equal(pred, before), 'pred must not be modified'
        assert np.array_equal(dec['idx'], g[f'idx_{tag}']), f'{tag}: decode order'
        assert np.array_equal(dec['cls'], g[f'cls_{tag}'])
        assert np.array_equal(dec['conf'], g[f'conf_{tag}'])
        assert np.array_equal(dec['box'], g[f'box_{tag}']), f'{tag}: integer boxes'
        det = su.detect_batch(pred, preset, thr, cap, max_out, nms=True)[0]
        keep = g[f'keep_{tag}']
        assert np.array_equal(det['idx'], g[f'idx_{tag}'][keep]), f'{tag}: NMS survivors / order'
        assert np.array_equal(det['cls'], g[f'cls_{tag}'][keep])
        assert np.array_equal(det['conf'], g[f'conf_{tag}'][keep])
        assert np.array_equal(det['box'], g[f'box_{tag}'][keep])
        n += 1
    assert n == 9


@pytest.mark.parametrize('C', [27, 28, 127])
def test_detect_vs_oracle_across_the_switch(C):
    """Both per-image paths (<= 1024 candidates in LDS, more through the bitonic sorts), every mode, against the oracle;
    the last class id is hot so the key's class field is used to its top."""
    rng = np.random.default_rng(C)
    A = 8732
    preset = su.get_preset_by_name('vgg300')
    oa = ob.anchors(ob.get_preset('vgg300'))
    pred = np.zeros((3, A, C + 5), np.float32); pred[:, :, C] = 1
    for i, ncand in enumerate((300, 1500, 0)):
        hot = rng.choice(A, ncand, replace=False)
        cls = rng.integers(0, C, ncand)
        cls[:20] = C - 1
        conf = rng.uniform(0.2, 0.99, ncand).astype(np.float32)
        pred[i, hot, C] = 1 - conf
        pred[i, hot, cls] = conf
        pred[i, :, C + 1:] = rng.normal(0, 0.3, (A, 4))
    for thr, cap, mo in ((0.2, None, 200), (0.2, 200, None), (0.2, 1100, 400)):
        for nms in (True, False):
            dets = su.detect_batch(pred, preset, thr, cap, mo, nms=nms)
            for i in range(3):
                want = ob.detect(pred[i], oa, thr, cap, mo) if nms else ob.decode(pred[i], oa, thr, cap)
                n = len(dets[i]['idx'])
                assert n == (len(want['idx']) if mo is None else min(len(want['idx']), mo)), (thr, cap, mo, nms, i)
                for k in ('idx', 'box', 'conf', 'cls'):
                    assert np.array_equal(dets[i][k], want[k][:n]), (k, thr, cap, mo, nms, i)


def test_detect_c80_batch_properties_full_size():
    """b = 128 x 8732 anchors at 80 classes: properties at full size, the oracle on a sample of images."""
    rng = np.random.default_rng(80)
    A, b, C = 8732, 128, 80
    pred = softmax_pred(rng, b, A, C, n_hot=50)
    preset = su.get_preset_by_name('vgg300')
    dets = su.detect_batch(pred, preset, 0.5, None, 200, nms=True)
    oa = ob.anchors(ob.get_preset('vgg300'))
    for i, d in enumerate(dets):
        n = len(d['conf'])
        assert 0 < n <= 200 and np.all(d['conf'] >= np.float32(0.5)) and np.all(d['cls'] < C)
        seen = []
        for j in range(n):
            if not seen or seen[-1] != d['cls'][j]:
                assert d['cls'][j] not in seen
                seen.append(d['cls'][j])
            elif j:
                assert d['conf'][j] <= d['conf'][j - 1]
        assert np.all(d['box'][:, 0] <= d['box'][:, 1]) and np.all(d['box'][:, 1] <= 999)
        if i % 32 == 0:
            want = ob.detect(pred[i], oa, 0.5, None, 200)
            for k in ('idx', 'box', 'conf', 'cls'):
                assert np.array_equal(d[k], want[k])


@pytest.mark.parametrize('C', [0, 128])
def test_class_count_out_of_range_raises(C):
    with pytest.raises(RuntimeError, match='1..127'):
        su.encode_labels_batch(su.get_preset_by_name('vgg300'), C, [np.zeros((0, 4))], [np.zeros(0, np.int64)])
    with pytest.raises(RuntimeError, match='1..127'):
        su.detect_batch(np.zeros((1, 8732, C + 5), np.float32), su.get_preset_by_name('vgg300'), 0.5, nms=True)
    with Session(0) as sess:
        with pytest.raises(RuntimeError, match='1..127'):
            SSDVGG(sess, 'vgg300').build_from_vgg(None, C, max_batch=1, training=False)


# ---- the network: wide heads / loss, the loss gradient ------------------------------------------------------------------
def head_out(net, preset, b, nv, prefix=''):
    """[b, A, nv] in anchor order from the fused head buffers (columns j*nv..)."""
    parts = []
    for i, (fk, s, ars) in enumerate(preset['maps']):
        buf = net.activation(prefix + f'head{i}', b)
        for j in range(2 + len(ars)):
            parts.append(buf[..., j * nv:(j + 1) * nv].reshape(b, fk * fk, nv))
    return np.concatenate(parts, 1)


def batch(rng, b, preset, C):
    anch = ob.anchors(preset); aabs = ob.anchors_abs(anch)
    x = ref.synth_images(rng, b, preset)
    ys = []
    for _ in range(b):
        while True:
            g, _ = ref.synth_gt(rng)
            c = rng.integers(0, C, len(g)); c[0] = C - 1
            y = ob.encode_labels(g, c, preset, C, anch, aabs)
            if np.count_nonzero(y[:, C]) < y.shape[0]:
                break
        ys.append(y)
    return x, np.stack(ys)


def step_check(pname, b, C, dtype='f32', seed=1234):
    preset = ob.get_preset(pname)
    nv = C + 5
    w = ref.init_params(preset, C, seed=42, alive=True)
    m = ref.RefModel(pname, C, params=w)
    sess = Session(0)
    net = SSDVGG(sess, pname)
    net.build_from_vgg(None, C, max_batch=b, training=True, weights=w, dtype=dtype)
    x, y = batch(np.random.default_rng(seed), b, preset, C)
    m.set_optimizer([0.001], [], 0.9, WD)
    net.build_optimizer(learning_rate=0.001, weight_decay=WD, momentum=0.9)

    # forward: result and losses from the GPU's own head outputs (the heads / loss kernel alone) ...
    r, L = sess.run([net.result, net.losses], feed_dict={net.image_input: x, net.labels: y})
    assert r.shape[0] == b and r.shape[2] == nv
    out_gpu = head_out(net, preset, b, nv)
    conf, loc, d_out, _ = ref.loss_numpy(out_gpu, y, C)
    assert abs(L['confidence'] - conf) < TOL * abs(conf) and abs(L['localization'] - loc) < TOL * abs(loc)
    sm = torch.softmax(torch.from_numpy(out_gpu[..., :C + 1]), -1).numpy()
    assert max_rel(r[..., :C + 1], sm) < TOL and np.array_equal(r[..., C + 1:], out_gpu[..., C + 1:])
    # ... and end to end against the oracle
    r_ref, L_ref = m.eval_step(x, y)
    if dtype == 'f32':
        assert max_rel(r, r_ref) < TOL
        for k in ('total', 'localization', 'confidence', 'l2'):
            assert abs(L[k] - L_ref[k]) < TOL * abs(L_ref[k]), (k, L[k], L_ref[k])
    else:
        assert abs(L['l2'] - L_ref['l2']) < TOL * L_ref['l2']
        assert abs(L['total'] - L_ref['total']) < 0.05 * abs(L_ref['total'])

    # backward: d(loss)/d(head outputs) against the oracle's from the same head outputs; pad columns stay zero
    xt = torch.from_numpy(x).cuda(); yt = torch.from_numpy(y).cuda()
    net.forward_backward_dev(xt, yt)
    torch.cuda.synchronize()
    got = head_out(net, preset, b, nv, 'grad:')
    assert max_rel(got, d_out) < (TOL if dtype == 'f32' else TOL_BF)
    for i, (fk, s, ars) in enumerate(preset['maps']):
        assert not net.activation(f'grad:head{i}', b)[..., (2 + len(ars)) * nv:].any()
    if dtype == 'f32':
        _, _, g_ref = m.grads(x, y)
        g = net.save_gradients()
        assert set(g) == set(g_ref)
        top = [k for k in g_ref if k.startswith(('classifiers', 'conv8', 'conv9', 'conv10', 'conv11', 'mod_conv'))]
        assert max(rel_err(g[k], g_ref[k]) for k in top) < TOL
    sess.close()


def test_step_vgg300_c80():
    step_check('vgg300', 2, 80)


@pytest.mark.usefixtures('direct_convs')
def test_step_vgg300_c80_on_the_direct_kernels():
    step_check('vgg300', 2, 80)


@pytest.mark.usefixtures('unfused_pools')
def test_step_vgg512_c127():
    step_check('vgg512', 1, 127, seed=77)


def test_step_vgg300_c80_bf16():
    step_check('vgg300', 2, 80, dtype='bf16')


@pytest.mark.parametrize('C', [27, 28])
def test_step_across_the_switch(C):
    step_check('vgg300', 1, C, seed=5)


# ---- average precision ----------------------------------------------------------------------------------------------------
def test_ap_c80_vs_oracle():
    rng = np.random.default_rng(80)
    nimg, ncls = 200, 80
    gb, gk, gs, db, dc, dk, ds = [], [], [], [], [], [], []
    for img in range(nimg):
        for _ in range(int(rng.integers(0, 6))):
            x0, y0 = rng.integers(0, 700, 2); w, h = rng.integers(30, 300, 2)
            k = int(rng.integers(0, ncls))
            gb.append([x0, x0 + w, y0, y0 + h]); gk.append(k); gs.append(img)
            for _ in range(int(rng.integers(0, 3))):
                j = rng.integers(-20, 20, 4)
                db.append([x0 + j[0], x0 + w + j[1], y0 + j[2], y0 + h + j[3]]); dk.append(k if rng.random() < 0.8 else int(rng.integers(0, ncls)))
                ds.append(img); dc.append(rng.uniform(0.01, 1.0))
    db = np.ascontiguousarray(db, np.float32); dc = np.ascontiguousarray(dc, np.float32)
    dk = np.ascontiguousarray(dk, np.int32); ds = np.ascontiguousarray(ds, np.int32)
    gbf = np.ascontiguousarray(gb, np.float64); gk = np.ascontiguousarray(gk, np.int32); gs = np.ascontiguousarray(gs, np.int32)
    want = oap.compute_aps(db, dc, dk, ds, gbf, gk, gs)
    ap = np.zeros(ncls); present = np.zeros(ncls, np.int32)
    check(lib.ssd_average_precision(0, len(dc), np_ptr(db), np_ptr(dc), np_ptr(dk), np_ptr(ds), len(gk), np_ptr(gbf), np_ptr(gk),
                                    np_ptr(gs), ncls, 0.5, np_ptr(ap), np_ptr(present)))
    assert sorted(np.nonzero(present)[0]) == sorted(want) and max(want) > 27
    for k, v in want.items():
        assert ap[k] == v, (k, ap[k], v)


# ---- drivers ---------------------------------------------------------------------------------------------------------------
def test_train_then_infer_80_classes(tmp_path, capsys):
    from ssd_tensorflow_amd import train, infer
    run = str(tmp_path / 'c80')
    assert train.main(['--name', run, '--tensorboard-dir', str(tmp_path / 'tb'), '--data-dir', 'shapes', '--synthetic-classes', '80',
                       '--epochs', '1', '--batch-size', '4', '--synthetic-train', '8', '--synthetic-valid', '4',
                       '--checkpoint-interval', '1']) == 0
    assert re.search(r'# classes:\s+80\n', capsys.readouterr().out)
    with np.load(os.path.join(run, 'final.npz'), allow_pickle=False) as ck:
        assert int(ck['__num_classes__']) == 80 and ck['__class_names__'].dtype.kind == 'U'
        assert list(ck['__class_names__']) == ['class_%d' % i for i in range(80)]
    odir = str(tmp_path / 'out')
    assert infer.main(['--name', run, '--synthetic', '3', '--batch-size', '2', '--threshold', '0.0', '--pascal-summary', 'true',
                       '--output-dir', odir]) == 0
    assert re.search(r'# classes:\s+80\n', capsys.readouterr().out)
    names = [f[len('comp4_det_test_'):-4] for f in os.listdir(odir) if f.startswith('comp4_det_test_')]
    assert names and set(names) <= {'class_%d' % i for i in range(80)}, names
