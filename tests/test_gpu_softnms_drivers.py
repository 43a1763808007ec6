"""GPU: infer.py and detect.py with --soft-nms end to end, untiled (--decode all) and tiled (--tile N --tile-decode
all): the banner names the rule, annotated pictures are written, the rows arrive in confidence order, and the AP of --ap-on host
and --ap-on gpu is the same dict."""
import os

import numpy as np
import pytest

import source_jpegset as SJ
from ssd_tensorflow_amd import detect, infer

pytestmark = pytest.mark.gpu

SHAPES = [(300, 520), (280, 300)]        # (h, w): 2 windows + the whole picture, 1 window at tile 300
PICK = ('[i] AP [', '[i] mAP', '[i] Processed')


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    d = tmp_path_factory.mktemp('softnms_set')
    rng = np.random.default_rng(38)
    SJ.write_dataset(d, [('pic%d' % k, rng.integers(0, 256, (h, w, 3)).astype(np.uint8), None) for k, (h, w) in enumerate(SHAPES)], 0)
    return str(d)


def _rows_in_confidence_order(odir):
    """the per-class files list a picture's rows in the order the decode emitted them: descending confidence"""
    n = 0
    for f in os.listdir(odir):
        if not f.startswith('comp4_det_test_'):
            continue
        per_image = {}
        for line in open(os.path.join(odir, f)):
            name, conf = line.split()[:2]
            per_image.setdefault(name, []).append(float(conf))
        for confs in per_image.values():
            assert confs == sorted(confs, reverse=True), (f, confs)
            n += len(confs)
    return n


def _pick(lines):
    return [l for l in lines if l.startswith(PICK)]


def test_infer_soft_nms_untiled_on_host_and_gpu(tmp_path, capsys):
    def run(out, extra):
        odir = str(tmp_path / out)
        rc = infer.main(['--name', str(tmp_path / 'none'), '--preset', 'vgg300', '--num-classes', '3', '--synthetic', '4', '--synthetic-boxes', '2',
                         '--batch-size', '2', '--threshold', '0.01', '--output-dir', odir, '--decode', 'all', '--keep-top-k', '37',
                         '--pascal-summary', 'true', *extra])
        return rc, odir, capsys.readouterr().out.splitlines()

    soft = ['--soft-nms', 'gaussian', '--soft-nms-sigma', '0.3']
    rc, odir, host = run('host', soft + ['--annotate', 'true', '--ap-on', 'host'])
    assert rc == 0
    assert any(l.startswith('[i] Decode:') and l.endswith('all (nms top k 400, keep top k 37, soft nms gaussian, sigma 0.3, min score the threshold)')
               for l in host), host
    pictures = [f for f in os.listdir(odir) if f.endswith('.png')]
    assert len(pictures) == 4 and all(os.path.getsize(os.path.join(odir, f)) > 1000 for f in pictures)
    assert _rows_in_confidence_order(odir) > 4
    rc, _, gpu = run('gpu', soft + ['--annotate', 'true', '--ap-on', 'gpu'])
    assert rc == 0 and _pick(gpu) == _pick(host) and any(l.startswith('[i] mAP') for l in host)
    # another rule than the default's: the hard run reports other confidences
    rc, hdir, hard = run('hard', ['--ap-on', 'host'])
    assert rc == 0 and any(l.endswith('all (nms top k 400, keep top k 37)') for l in hard)
    read = lambda d: {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.startswith('comp4_')}
    assert read(hdir) != read(odir)


def test_infer_soft_nms_tiled_on_host_and_gpu(tmp_path, capsys, dataset):
    def run(out, extra):
        odir = str(tmp_path / out)
        rc = infer.main(['--name', str(tmp_path / 'none'), '--preset', 'vgg300', '--num-classes', '20', '--data-source', 'jpegset', '--data-dir', dataset,
                         '--sample', 'trainval', '--batch-size', '2', '--threshold', '0.01', '--output-dir', odir, '--tile', '300', '--tile-decode',
                         'all', '--nms-top-k', '60', '--keep-top-k', '37', '--pascal-summary', 'true', '--soft-nms', 'gaussian', *extra])
        return rc, odir, capsys.readouterr().out.splitlines()

    rc, odir, host = run('host', ['--annotate', 'true', '--ap-on', 'host'])
    assert rc == 0
    assert any(l.startswith('[i] Tile decode:') and l.endswith('all (nms top k 60, keep top k 37, soft nms gaussian, sigma 0.5, min score the threshold)')
               for l in host), host
    assert len([f for f in os.listdir(odir) if f.endswith('.png')]) == 2 and _rows_in_confidence_order(odir) > 4
    rc, gdir, gpu = run('gpu', ['--annotate', 'true', '--ap-on', 'gpu'])
    assert rc == 0 and _pick(gpu) == _pick(host) and len(_pick(host)) > 3
    tree = lambda d: {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}
    assert tree(odir) == tree(gdir)


def test_detect_soft_nms_untiled_and_tiled(tmp_path, capsys):
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    rng = np.random.default_rng(39)
    pictures = []
    for k, (h, w) in enumerate(SHAPES):
        pictures.append(str(tmp_path / ('pic%d.npy' % k)))
        np.save(pictures[-1], rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
    model = str(tmp_path / 'model.npz')
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 1, max_batch=2)      # one class: random weights reach detect.py's threshold of 0.5
        net.build_optimizer()
        net.save_checkpoint(model, class_names=['thing'])
    outs = {}
    for name, flags in (('hard', ['--decode', 'all']), ('soft', ['--decode', 'all', '--soft-nms', 'gaussian']),
                        ('tiled', ['--tile', '300', '--tile-decode', 'all', '--soft-nms', 'linear', '--soft-nms-min-score', '0.1'])):
        odir = str(tmp_path / name)
        assert detect.main(['--model', model, '--output-dir', odir, '--batch-size', '2'] + flags + pictures) == 0
        capsys.readouterr()
        listing = sorted(os.listdir(odir))
        assert [f for f in listing if f.endswith('.png')] == ['pic0.npy.png', 'pic1.npy.png']
        outs[name] = {f: open(os.path.join(odir, f)).read() for f in listing if f.endswith('.txt')}
        assert len(outs[name]) == 2
    assert any(len(v) > 0 for v in outs['hard'].values()) and any(len(v) > 0 for v in outs['soft'].values())
