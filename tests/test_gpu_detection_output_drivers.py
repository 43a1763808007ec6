"""GPU: infer.py with --decode all end to end: annotated pictures, the per-class .txt files, the AP on the host
and on the GPU; --decode all with --tile is an argument error; --decode argmax is the run without the flag."""
import collections
import os

import pytest

from ssd_tensorflow_amd import infer

pytestmark = pytest.mark.gpu


def _run(tmp_path, capsys, out, extra):
    odir = str(tmp_path / out)
    rc = infer.main(['--name', str(tmp_path / 'none'), '--preset', 'vgg300', '--num-classes', '3', '--synthetic', '4', '--synthetic-boxes', '2',
                     '--batch-size', '2', '--threshold', '0.01', '--output-dir', odir, *extra])
    lines = capsys.readouterr().out.splitlines()
    return rc, odir, lines


def _per_image_counts(odir):
    counts = collections.Counter()
    files = [f for f in os.listdir(odir) if f.startswith('comp4_det_test_')]
    for f in files:
        for line in open(os.path.join(odir, f)):
            counts[line.split()[0]] += 1
    return counts, files


def test_infer_decode_all_annotates_and_respects_keep_top_k(tmp_path, capsys):
    rc, odir, lines = _run(tmp_path, capsys, 'all', ['--decode', 'all', '--annotate', 'true', '--pascal-summary', 'true', '--keep-top-k', '37'])
    assert rc == 0
    assert any(l.startswith('[i] Decode:') and l.endswith('all (nms top k 400, keep top k 37)') for l in lines)
    pictures = sorted(f for f in os.listdir(odir) if f.endswith('.png'))
    assert len(pictures) == 4 and all(os.path.getsize(os.path.join(odir, f)) > 1000 for f in pictures)
    counts, files = _per_image_counts(odir)
    assert len(counts) == 4 and len(files) >= 2            # random weights at 0.01: more than one class in the output
    assert max(counts.values()) <= 37 and sum(counts.values()) > 4
    done = [l for l in lines if l.startswith('[i] Processed')]
    assert done == ['[i] Processed 4 images, %d detections' % sum(counts.values())]
    assert any(l.startswith('[i] mAP') for l in lines)
    # the same detections reach the device accumulator
    rc, _, gpu = _run(tmp_path, capsys, 'all_gpu', ['--decode', 'all', '--keep-top-k', '37', '--ap-on', 'gpu'])
    assert rc == 0
    pick = lambda ls: [l for l in ls if l.startswith('[i] AP [') or l.startswith('[i] mAP') or l.startswith('[i] Processed')]
    assert pick(gpu) == pick(lines)


def test_decode_all_with_tile_is_an_argument_error(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        infer.main(['--name', str(tmp_path / 'none'), '--preset', 'vgg300', '--decode', 'all', '--tile', '300', str(tmp_path / 'x.npy')])
    assert e.value.code not in (0, None)
    assert '--decode all does not apply to --tile' in capsys.readouterr().err


def test_decode_argmax_is_the_run_without_the_flag(tmp_path, capsys):
    rc_a, dir_a, lines_a = _run(tmp_path, capsys, 'plain', ['--pascal-summary', 'true'])
    rc_b, dir_b, lines_b = _run(tmp_path, capsys, 'argmax', ['--decode', 'argmax', '--pascal-summary', 'true', '--nms-top-k', '5', '--keep-top-k', '5'])
    assert rc_a == 0 and rc_b == 0
    strip = lambda ls: [l for l in ls if 'Output directory' not in l]
    assert strip(lines_a) == strip(lines_b)
    assert sorted(os.listdir(dir_a)) == sorted(os.listdir(dir_b)) and os.listdir(dir_a)
    for f in os.listdir(dir_a):
        assert open(os.path.join(dir_a, f), 'rb').read() == open(os.path.join(dir_b, f), 'rb').read(), f
    counts, _ = _per_image_counts(dir_a)
    assert max(counts.values()) == 200                      # (the reference decode's [:200], not --keep-top-k)
