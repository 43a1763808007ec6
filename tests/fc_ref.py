"""CPU restatement of the reference's fc graph (SSDVGG.build_from_vgg(a_trous=False) -> __build_vgg_mods, ssdvgg.py:210-228),
built from the oracle's primitives: VGG-16's fc6 / fc7 as a 7x7 and a 1x1 convolution, 4096 wide, under the variables
fc6/weights, fc6/biases, fc7/weights, fc7/biases; conv8_1 and the map-1 head read 4096 channels.  The L2 term adds the two
fc filters (ssdvgg.py:220, 228) to oracle.l2_term's '*/filter' sum."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import boxes as ob
from oracle import ssdvgg_ref as ref

FC_VARS = {'fc6/weights': (7, 7, 512, 4096), 'fc6/biases': (4096,), 'fc7/weights': (1, 1, 4096, 4096), 'fc7/biases': (4096,)}
REF_PARAMS = {'vgg300': 144995758, 'vgg512': 145669572}      # the reference's parameter count at 20 classes


def param_shapes(preset, num_classes=20):
    """Ordered {tf_variable_name: shape} of the fc graph."""
    out = {}
    for name, shp in ref.param_shapes(preset, num_classes).items():
        if name == 'mod_conv6/filter':
            out.update(FC_VARS)
            continue
        if name.startswith(('mod_conv6/', 'mod_conv7/')):
            continue
        if name == 'conv8_1/filter' or name.startswith('classifiers/classifier1_') and name.endswith('/filter'):
            shp = shp[:2] + (4096,) + shp[3:]
        out[name] = shp
    return out


def init_params(preset, num_classes=20, seed=42):
    """ref.init_params(alive=True)'s scheme on the fc graph's shapes (the fc filters are He-uniform filters)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shp in param_shapes(preset, num_classes).items():
        if name.endswith(('/filter', '/weights')):
            kh, kw, ci, co = shp
            w = rng.uniform(-1, 1, shp).astype(np.float32) * np.float32(math.sqrt(6.0 / (kh * kw * ci)))
            if name.startswith('conv1_1'):
                w /= 100.0
            if name.startswith('classifiers'):
                w *= 0.05
            out[name] = w.astype(np.float32)
        elif name.endswith('/scale'):
            out[name] = np.full(shp, 20.0, np.float32)
        else:
            out[name] = rng.normal(0.02, 0.02, shp).astype(np.float32)
    return out


def forward(params, x_nhwc, preset, num_classes=20):
    """(out [B,A,C+5] raw head outputs, result) of the fc graph."""
    nv = num_classes + 5
    x = x_nhwc.permute(0, 3, 1, 2)

    def cbr(x, w, b, stride=1, padding='SAME', relu=True):
        y = ref.conv2d_tf(x, params[w], stride, padding) + params[b].view(1, -1, 1, 1)
        return F.relu(y) if relu else y

    for l in ref.VGG:
        if l == 'pool':
            x = ref.maxpool_tf(x, 2, 2)
        else:
            x = cbr(x, l[0] + '/filter', l[0] + '/biases')
            if l[0] == 'conv4_3':
                conv4_3 = x
    x = ref.maxpool_tf(x, 3, 1)                                  # mod_pool5
    x = cbr(x, 'fc6/weights', 'fc6/biases')                      # mod_conv6, ssdvgg.py:215-220
    x = cbr(x, 'fc7/weights', 'fc7/biases')                      # mod_conv7, ssdvgg.py:223-228
    fmaps = [None, x]
    for (n, k, ci, co, s, p) in ref.extra_layers(preset):
        if n == 'conv12_2':
            x = F.pad(x, (0, 1, 0, 1))
        x = cbr(x, n + '/filter', n + '/biases', s, p)
        if n.endswith('_2'):
            fmaps.append(x)
    fmaps[0] = ref.l2norm_tf(conv4_3, params['l2_norm_conv4_3/scale'])
    outs = []
    for i, (fk, s, ars) in enumerate(preset['maps']):
        for j in range(2 + len(ars)):
            n = f'classifiers/classifier{i}_{j}'
            y = ref.conv2d_tf(fmaps[i], params[n + '/filter']) + params[n + '/biases'].view(1, -1, 1, 1)
            outs.append(y.permute(0, 2, 3, 1).reshape(y.shape[0], fk * fk, nv))
    out = torch.cat(outs, 1)
    logits = out[:, :, :num_classes + 1]
    result = torch.cat([F.softmax(logits, -1), out[:, :, num_classes + 1:]], -1)
    return out, result


def l2_term(params):
    return ref.l2_term(params) + sum((params[n] * params[n]).sum() / 2 for n in ('fc6/weights', 'fc7/weights'))


def losses(out, labels, params, num_classes=20, weight_decay=0.0005):
    L = ref.losses(out, labels, params, num_classes, weight_decay)
    extra = weight_decay * (l2_term(params) - ref.l2_term(params))
    L['l2'] = L['l2'] + extra
    L['total'] = L['total'] + extra
    return L


class RefModelFC:
    """ref.RefModel's eval / gradient / momentum step on the fc graph."""

    def __init__(self, preset_name, params, num_classes=20, momentum=0.9, weight_decay=0.0005, lr=0.001):
        self.preset = ob.get_preset(preset_name)
        self.num_classes = num_classes
        self.params = {k: torch.tensor(np.asarray(v, np.float32)).requires_grad_(True) for k, v in params.items()}
        self.momentum, self.weight_decay, self.lr = momentum, weight_decay, lr

    def eval_step(self, x, y):
        with torch.no_grad():
            out, result = forward(self.params, torch.as_tensor(x, dtype=torch.float32), self.preset, self.num_classes)
            L = losses(out, torch.as_tensor(y, dtype=torch.float32), self.params, self.num_classes, self.weight_decay)
        return result.numpy(), {k: float(v) for k, v in L.items()}

    def grads(self, x, y):
        for p in self.params.values():
            p.grad = None
        out, result = forward(self.params, torch.as_tensor(x, dtype=torch.float32), self.preset, self.num_classes)
        L = losses(out, torch.as_tensor(y, dtype=torch.float32), self.params, self.num_classes, self.weight_decay)
        L['total'].backward()
        g = {k: (p.grad.detach().numpy().copy() if p.grad is not None else np.zeros(p.shape, np.float32))
             for k, p in self.params.items()}
        return result.detach().numpy(), {k: float(v) for k, v in L.items()}, g
