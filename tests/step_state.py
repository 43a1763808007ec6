"""Shared by the GPU tests that compare whole training steps bit for bit (test_gpu_winograd_dual_step.py,
test_gpu_backward_schedules.py): a training handle on given weights, its state after a step, and the comparison."""
import numpy as np
import torch

from ssd_tensorflow_amd._lib import lib, check
from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session


def make(w, mode, overlap, preset='vgg300', batch=3, dtype='f32'):
    """mode: ssd_set_wino_dual, None leaves the handle's default; overlap False: ssd_set_overlap 0"""
    sess = Session(0)
    net = SSDVGG(sess, preset)
    net.build_from_vgg(None, 20, max_batch=batch, weights=w, dtype=dtype)
    net.build_optimizer(learning_rate=0.001, weight_decay=0.0005, momentum=0.9)
    net.set_stream(torch.cuda.current_stream().cuda_stream)
    if mode is not None:
        check(lib.ssd_set_wino_dual(net._h, mode))
    if not overlap:
        check(lib.ssd_set_overlap(net._h, 0))
    return sess, net


def state(net, batch=3):
    torch.cuda.synchronize()
    res = np.empty((batch, net.preset.num_anchors, net.num_vars), np.float32)
    check(lib.ssd_get_result(net._h, batch, res.ctypes.data))
    return dict(losses=net.get_losses(), result=res.view(np.uint32), grads=net.grads_flat.clone(), params=net.params_flat.clone(),
                momentum=net.momentum_flat.clone())


def assert_same(a, b, where):
    assert a['losses'] == b['losses'], f'{where}: losses {a["losses"]} != {b["losses"]}'
    assert np.array_equal(a['result'], b['result']), f'{where}: result differs'
    for k in ('grads', 'params', 'momentum'):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), \
            f'{where}: {k}_flat differs in {int((a[k].view(torch.int32) != b[k].view(torch.int32)).sum())} words'
