"""GPU: infer.py with --tile N --tile-decode all end to end on a small data source: annotated pictures, the
per-class files, the AP on the host and on the GPU, against the library call; --tile-decode argmax is the run without the flag;
--tile-decode all without --tile is an argument error."""
import os

import numpy as np
import pytest

import source_jpegset as SJ
from ssd_tensorflow_amd import infer, tiling
from ssd_tensorflow_amd import ssdutils as su
from ssd_tensorflow_amd import utils as ut

pytestmark = pytest.mark.gpu

SHAPES = [(300, 520), (280, 300), (450, 380)]        # (h, w): 2 + whole, 1, 2 + whole tiles at tile 300
PICK = ('[i] AP [', '[i] mAP', '[i] Processed')


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    d = tmp_path_factory.mktemp('tiledet_set')
    rng = np.random.default_rng(28)
    SJ.write_dataset(d, [('pic%d' % k, rng.integers(0, 256, (h, w, 3)).astype(np.uint8), None) for k, (h, w) in enumerate(SHAPES)], 0)
    return str(d)


def _run(tmp_path, capsys, dataset, out, extra):
    odir = str(tmp_path / out)
    rc = infer.main(['--name', str(tmp_path / 'none'), '--preset', 'vgg300', '--num-classes', '20', '--data-source', 'jpegset', '--data-dir', dataset,
                     '--sample', 'trainval', '--batch-size', '2', '--threshold', '0.01', '--output-dir', odir, *extra])
    return rc, odir, capsys.readouterr().out.splitlines()


def _tree(d):
    return {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}


def test_infer_tile_decode_all_on_host_and_gpu_equals_the_library(tmp_path, capsys, dataset):
    flags = ['--tile', '300', '--tile-decode', 'all', '--nms-top-k', '60', '--keep-top-k', '37', '--pascal-summary', 'true']
    rc, odir, host = _run(tmp_path, capsys, dataset, 'host', flags + ['--annotate', 'true', '--ap-on', 'host'])
    assert rc == 0
    assert any(l.startswith('[i] Tile decode:') and l.endswith('all (nms top k 60, keep top k 37)') for l in host)
    rc, gdir, gpu = _run(tmp_path, capsys, dataset, 'gpu', flags + ['--annotate', 'true', '--ap-on', 'gpu'])
    assert rc == 0
    pick = lambda ls: [l for l in ls if l.startswith(PICK)]
    assert pick(gpu) == pick(host) and len(pick(host)) > 5 and any(l.startswith('[i] mAP') for l in host)
    assert _tree(odir) == _tree(gdir)
    pictures = sorted(f for f in os.listdir(odir) if f.endswith('.png'))
    assert len(pictures) == 3 and all(os.path.getsize(os.path.join(odir, f)) > 1000 for f in pictures)
    # the library call on the same network (the driver's random weights are seeded)
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd.pascal_summary import PascalSummary
    files = [os.path.join(dataset, 'pic%d.npy' % k) for k in range(3)]
    want = []
    with Session(0) as sess:
        net = SSDVGG(sess, su.get_preset_by_name('vgg300'))
        net.build_from_vgg(None, 20, max_batch=2, training=False)
        det = tiling.TiledDetector(net, 300, threshold=0.01, decode='all', nms_top_k=60, keep_top_k=37)
        for packed, offs, shapes, idxs in tiling.source_batches(files, 2, sess.device):
            want += [{k: v.copy() for k, v in d.items()} for d in det.launch(packed, offs, shapes).get()]
    counts = [len(w['idx']) for w in want]
    assert len(want) == 3 and max(counts) == 37 and len({int(c) for w in want for c in w['cls']}) > 1
    assert [l for l in host if l.startswith('[i] Processed')] == ['[i] Processed 3 images, %d detections' % sum(counts)]
    names = dict(SJ.get_source().lid2name)
    summary = PascalSummary()
    for f, (h, w_), w in zip(files, SHAPES, want):
        summary.add_detections(f, su.boxes_from_detection(w, names), img_size=ut.Size(w_, h))
    os.makedirs(str(tmp_path / 'summary'))
    summary.write_summary(str(tmp_path / 'summary'))
    assert _tree(str(tmp_path / 'summary')) == {k: v for k, v in _tree(odir).items() if k.startswith('comp4_')} != {}


def test_tile_decode_argmax_is_the_run_without_the_flag(tmp_path, capsys, dataset):
    flags = ['--tile', '300', '--pascal-summary', 'true', '--annotate', 'true']
    rc_a, dir_a, lines_a = _run(tmp_path, capsys, dataset, 'plain', flags)
    rc_b, dir_b, lines_b = _run(tmp_path, capsys, dataset, 'argmax', flags + ['--tile-decode', 'argmax', '--nms-top-k', '5', '--keep-top-k', '5'])
    assert rc_a == 0 and rc_b == 0
    strip = lambda ls: [l for l in ls if 'Output directory' not in l]
    assert strip(lines_a) == strip(lines_b)
    ta, tb = _tree(dir_a), _tree(dir_b)
    assert ta == tb and len(ta) > 3 and any(len(v) > 0 for k, v in ta.items() if k.startswith('comp4_'))


def test_tile_decode_all_without_tile_is_an_argument_error(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        infer.main(['--name', str(tmp_path / 'none'), '--preset', 'vgg300', '--tile-decode', 'all', str(tmp_path / 'x.npy')])
    assert e.value.code not in (0, None)
    assert '--tile-decode all needs --tile' in capsys.readouterr().err
