"""-m gpu: train.py --match: a tiny synthetic run under 'paper', the rule in the checkpoint's metadata,
and --continue-training taking the checkpoint's rule over the flag's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_train_match_paper_checkpoint_and_resume(tmp_path, capsys):
    from ssd_tensorflow_amd import train
    common = ['--batch-size', '2', '--synthetic-train', '4', '--synthetic-valid', '2', '--lr-values', '0.0001;0.00001',
              '--lr-boundaries', '4', '--tensorboard-dir', str(tmp_path / 'tb')]
    run = str(tmp_path / 'run')
    # two steps (4 samples, batch 2), one checkpoint
    assert train.main(['--name', run, '--epochs', '1', '--checkpoint-interval', '1', '--match', 'paper'] + common) == 0
    out = capsys.readouterr().out
    assert '[i] Matching rule:' in out and 'paper' in out.split('[i] Matching rule:')[1].splitlines()[0]
    with np.load(run + '/e1.npz', allow_pickle=False) as ck:
        assert str(ck['__match__']) == 'paper' and int(ck['__global_step__']) == 2
        assert '__class_names__' in ck.files and '__a_trous__' in ck.files
    assert train.checkpoint_match(run + '/e1.npz') == 'paper'
    # the flag's default disagrees with the checkpoint: the checkpoint's rule is taken, and the driver says so
    assert train.main(['--name', run, '--epochs', '2', '--checkpoint-interval', '1', '--continue-training', 'true'] + common) == 0
    out = capsys.readouterr().out
    assert "disagrees with the checkpoint" in out and "'paper'" in out
    assert 'paper' in out.split('[i] Matching rule:')[1].splitlines()[0]
    with np.load(run + '/e2.npz', allow_pickle=False) as ck:
        assert str(ck['__match__']) == 'paper' and int(ck['__global_step__']) == 4


def test_default_run_records_the_reference_rule(tmp_path):
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    from ssd_tensorflow_amd import train
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 20, max_batch=1)
        path = str(tmp_path / 'c.npz')
        net.save_checkpoint(path)
        assert train.checkpoint_match(path) == 'reference'
        with pytest.raises(ValueError, match='match'):
            net.save_checkpoint(path, match='caffe')
