"""Host-side mirror of the reference's class SSDVGG (ssdvgg.py:87-649) over the C ABI of
libssdvgg_hip.so.  Same method names, argument meaning and attribute names, so the
reference's train.py / infer.py loops read unchanged:

    net = SSDVGG(sess, preset)
    net.build_from_vgg(vgg_dir, num_classes)
    net.build_optimizer(learning_rate=..., weight_decay=..., momentum=..., global_step=...)
    result, loss_batch, _ = sess.run([net.result, net.losses, net.optimizer],
                                     feed_dict={net.image_input: x, net.labels: y})

`Session` stands in for tf.Session: it owns no graph, it routes run() to the handle.
PyTorch appears only as the allocator of the parameter / gradient / momentum arenas
(so torch.distributed can all-reduce the gradient arena in place) and as stream owner.
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import lib, check, np_ptr
from .ssdutils import get_preset_by_name, SSD_PRESETS, detect_batch

LOSS_NAMES = ('total', 'localization', 'confidence', 'l2')      # ssdvgg.py:594-599
# compute types of a handle (include/ssdvgg_hip.h SSD_DTYPE_*); 'fp8', 'mxfp8' and 'mxfp6' are inference only
DTYPES = {'f32': 0, 'bf16': 1, 'fp8': 2, 'mxfp8': 3, 'mxfp6': 4}
# losses of a training handle (include/ssdvgg_hip.h SSD_LOSS_*): the reference's hard-negative mining, or the focal loss
LOSS_KINDS = {'mining': 0, 'focal': 1}


class LossConfig(C.Structure):
    """ssd_loss_config of the C ABI"""
    _fields_ = [('kind', C.c_int), ('focal_gamma', C.c_float), ('focal_alpha', C.c_float)]


def loss_config(loss='mining', focal_gamma=2.0, focal_alpha=0.25):
    """The ABI's configuration of a loss given by name; a bad name, gamma outside [0, 5] or alpha outside (0, 1): ValueError."""
    if loss not in LOSS_KINDS:
        raise ValueError('loss must be one of %s, got %r' % (sorted(LOSS_KINDS), loss))
    g, a = float(focal_gamma), float(focal_alpha)
    if loss == 'focal' and not (0.0 <= g <= 5.0 and 0.0 < a < 1.0):
        raise ValueError('focal loss takes gamma in [0, 5] and alpha in (0, 1), got gamma %r, alpha %r' % (focal_gamma, focal_alpha))
    return LossConfig(LOSS_KINDS[loss], g, a)


def checkpoint_loss(ck):
    """(loss name, gamma, alpha) of an opened checkpoint; one from before the option is 'mining'."""
    if '__loss__' not in ck.files:
        return 'mining', 2.0, 0.25
    return str(ck['__loss__']), float(ck['__focal_gamma__']), float(ck['__focal_alpha__'])


# localization losses of a training handle (include/ssdvgg_hip.h SSD_LOC_*): the reference's smooth-L1, or GIoU
LOC_LOSS_KINDS = {'smooth_l1': 0, 'giou': 1}


class LocLossConfig(C.Structure):
    """ssd_loc_loss_config of the C ABI"""
    _fields_ = [('kind', C.c_int), ('weight', C.c_float)]


def loc_loss_config(loc_loss='smooth_l1', loc_weight=1.0):
    """The ABI's configuration of a localization loss given by name; a bad name, or a weight that is not a finite number > 0:
    ValueError.  Under 'smooth_l1' the weight is ignored and stored as 1."""
    if loc_loss not in LOC_LOSS_KINDS:
        raise ValueError('localization loss must be one of %s, got %r' % (sorted(LOC_LOSS_KINDS), loc_loss))
    w = float(loc_weight)
    if loc_loss == 'smooth_l1':
        return LocLossConfig(LOC_LOSS_KINDS[loc_loss], 1.0)
    if not (np.isfinite(w) and w > 0.0):
        raise ValueError('localization loss %r takes a finite weight > 0, got %r' % (loc_loss, loc_weight))
    return LocLossConfig(LOC_LOSS_KINDS[loc_loss], w)


def checkpoint_loc_loss(ck):
    """(localization loss name, weight) of an opened checkpoint; one from before the option is 'smooth_l1'."""
    if '__loc_loss__' not in ck.files:
        return 'smooth_l1', 1.0
    return str(ck['__loc_loss__']), float(ck['__loc_weight__'])


class GradClipConfig(C.Structure):
    """ssd_grad_clip_config of the C ABI"""
    _fields_ = [('max_norm', C.c_float)]


def grad_clip_config(clip_norm=0.0):
    """The ABI's configuration of gradient clipping by global norm (include/ssdvgg_hip.h): 0 off, a number > 0 the
    threshold, inf measures the norm of every update and never clips.  A negative value or NaN: ValueError."""
    v = float(clip_norm)
    if not v >= 0.0:
        raise ValueError('gradient clipping takes clip_norm 0 (off), a number > 0 or inf, got %r' % (clip_norm,))
    return GradClipConfig(v)


def checkpoint_clip_norm(ck):
    """clip_norm of an opened checkpoint; one from before the option is 0.0 (off)."""
    if '__clip_norm__' not in ck.files:
        return 0.0
    return float(ck['__clip_norm__'])


# update rules of a training handle (include/ssdvgg_hip.h SSD_UPDATE_*): the reference's momentum, or AdamW
UPDATE_KINDS = {'momentum': 0, 'adamw': 1}
ADAM_DEFAULTS = (0.9, 0.999, 1e-8, 0.01)      # beta1, beta2, eps, decay


class UpdateRuleConfig(C.Structure):
    """ssd_update_rule_config of the C ABI"""
    _fields_ = [('kind', C.c_int), ('beta1', C.c_float), ('beta2', C.c_float), ('eps', C.c_float), ('decay', C.c_float)]


def update_rule_config(optimizer='momentum', adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8, adam_decay=0.01):
    """The ABI's configuration of an update rule given by name (include/ssdvgg_hip.h).  beta1 or beta2 outside
    [0, 1), an eps that is not a finite number > 0, a decay that is not a finite number >= 0 (as float32, what the library
    gets), or a bad name, in that order: ValueError."""
    b1, b2, eps, decay = (float(np.float32(x)) for x in (adam_beta1, adam_beta2, adam_eps, adam_decay))
    for name, b in (('beta1', b1), ('beta2', b2)):
        if not 0.0 <= b < 1.0:
            raise ValueError('update rule: %s must lie in [0, 1), got %r' % (name, b))
    if not (np.isfinite(eps) and eps > 0.0):
        raise ValueError('update rule: eps must be a finite number > 0, got %r' % (adam_eps,))
    if not (np.isfinite(decay) and decay >= 0.0):
        raise ValueError('update rule: decay must be a finite number >= 0, got %r' % (adam_decay,))
    if optimizer not in UPDATE_KINDS:
        raise ValueError('update rule must be one of %s, got %r' % (sorted(UPDATE_KINDS), optimizer))
    return UpdateRuleConfig(UPDATE_KINDS[optimizer], b1, b2, eps, decay)


def checkpoint_update_rule(ck):
    """(optimizer name, beta1, beta2, eps, decay) of an opened checkpoint; one without __optimizer__ is a momentum run's."""
    if '__optimizer__' not in ck.files:
        return ('momentum',) + ADAM_DEFAULTS
    return (str(ck['__optimizer__']),) + tuple(float(np.float32(ck[k])) for k in
                                               ('__adam_beta1__', '__adam_beta2__', '__adam_eps__', '__adam_decay__'))


# which set of a checkpoint with a weight EMA becomes an inference handle's parameters (build_from_metagraph)
WEIGHT_SETS = ('auto', 'raw', 'ema')


def ema_decay_config(ema_decay=0.0):
    """The decay of the weight EMA as the library gets it, a float32 (include/ssdvgg_hip.h "weight EMA"): 0 is off;
    anything else outside (0, 1) -- NaN, and 1.0 as a float32 too: ValueError."""
    d = float(np.float32(ema_decay))
    if d != 0.0 and not 0.0 < d < 1.0:
        raise ValueError('weight EMA: decay must be 0 (off) or lie in (0, 1) as a float32, got %r' % (ema_decay,))
    return abs(d) if d == 0.0 else d


def checkpoint_ema(ck):
    """The decay of the weight EMA of an opened checkpoint's run; a file without __ema_decay__ is a run's without one: 0.0."""
    if '__ema_decay__' not in ck.files:
        return 0.0
    return float(np.float32(ck['__ema_decay__']))


def checkpoint_has_ema(ck):
    """whether an opened checkpoint holds the averaged weights (__ema__/<variable>) beside the raw ones"""
    return any(k.startswith('__ema__/') for k in ck.files)


NO_EMA_IN_FILE = "weights='ema': %s holds no weight EMA (its run had --ema-decay 0)"


class _Token:
    """An opaque stand-in for a TF tensor/op handle; only identity matters."""
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return f'<ssd token {self.name}>'


class _DetectionList:
    """The detections of one pass as a sequence of per-image dicts {conf, cls, idx, box} (what detect_last returned as
    a list).  The arrays are VIEWS of the handle's pinned host mirror of that pass: an image's dict is built when it
    is indexed, so collecting a batch costs the host one event wait and no per-image work it does not ask for.  Valid
    until the second-next pass is launched (two slots alternate); copy what must live longer."""

    def __init__(self, count, conf, cls, idx, box, out_cap, net=None, serial=0):
        self.count, self.conf, self.cls, self.idx, self.box, self.out_cap = count, conf, cls, idx, box, out_cap
        self.net, self.serial = net, serial      # the views point into pinned memory the handle owns: checked on every access

    def __len__(self):
        return len(self.count)

    def _check_alive(self):
        """The slot behind these views is rewritten by the second-next pass, moved (freed) when it has to grow and freed with the
        handle: an access after any of these is an error here, not a read of freed memory."""
        net = self.net
        if net is None:
            return
        if net._h is None:
            raise RuntimeError('these detections belong to a closed SSDVGG handle: copy what must outlive it')
        if net._det_serial - self.serial not in (0, 1):
            raise RuntimeError('these detections were overwritten: only the two most recent passes are kept (copy what must live longer)')

    def __getitem__(self, i):
        self._check_alive()
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        n = min(int(self.count[i]), self.out_cap)
        return dict(conf=self.conf[i, :n], cls=self.cls[i, :n], idx=self.idx[i, :n], box=self.box[i, :n])

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class _Detections:
    """Ticket of SSDVGG.detect_last_launch."""
    def __init__(self, net, serial, b, out_cap, slots=None):
        self.net, self.serial, self.b, self.out_cap = net, serial, b, out_cap
        self._slots = slots

    def dev_slots(self):
        """(count, conf, cls, box, b, out_cap, stream): the pass's device-visible output slots and the stream it runs on --
        what a kernel enqueued behind the pass reads (average_precision.DeviceAPCalculator.add_pass)."""
        if self.net._det_serial != self.serial:
            raise RuntimeError('the slots of these detections belong to an earlier pass: use them right after the launch')
        return (*self._slots, self.b, self.out_cap, getattr(self.net, '_stream_ptr', 0))

    def get(self):
        which = self.net._det_serial - self.serial
        if which not in (0, 1):
            raise RuntimeError('these detections were overwritten: only the two most recent passes are kept')
        ptrs = [C.c_void_p() for _ in range(5)]
        b = C.c_int(); out_cap = C.c_int()
        check(lib.ssd_detect_host(self.net._h, which, *[C.byref(p) for p in ptrs], C.byref(b), C.byref(out_cap)))
        b, oc = b.value, out_cap.value
        key = (ptrs[0].value, ptrs[4].value, b, oc)
        views = self.net._det_views.get(key)
        if views is None:      # the slots' host arrays move only when a slot grows: the numpy views are built once per layout

            def view(p, ctype, dtype, shape):
                n = int(np.prod(shape))
                return np.frombuffer((ctype * n).from_address(p.value), dtype=dtype).reshape(shape)
            views = (view(ptrs[0], C.c_int, np.int32, (b,)), view(ptrs[1], C.c_float, np.float32, (b, oc)),
                     view(ptrs[2], C.c_int, np.int32, (b, oc)), view(ptrs[3], C.c_int, np.int32, (b, oc)),
                     view(ptrs[4], C.c_int, np.int32, (b, oc, 4)))
            if len(self.net._det_views) > 8:
                self.net._det_views.clear()
            self.net._det_views[key] = views
        return _DetectionList(*views, oc, net=self.net, serial=self.serial)


class _Annotated:
    """Ticket of SSDVGG.annotate_last_launch.  With keep_device: `dev` is the packed device tensor the drawing wrote (image i as
    [h][w][3] at byte offset offs[i], shapes[i] = (h, w)) and `stream` the torch stream it was written on."""
    def __init__(self, host, done, offs, shapes, dev=None, stream=None):
        self.host, self.done, self.offs, self.shapes, self.dev, self.stream = host, done, offs, shapes, dev, stream

    def get(self):
        from . import annotate as A
        if self.host is None:
            raise RuntimeError('annotate_last_launch(to_host=False) keeps the pictures on the GPU: there are no host pixels to get')
        self.done.synchronize()
        return A.unpack(self.host.numpy(), self.offs, self.shapes)


class LearningRate:
    """compute_lr's result (train.py:43-47): piecewise-constant values over global_step."""
    def __init__(self, values, boundaries):
        values = [float(v) for v in values]; boundaries = [int(b) for b in boundaries]
        if len(values) != len(boundaries) + 1:
            raise ValueError('lr_values must hold one more entry than lr_boundaries')
        self.values, self.boundaries = values, boundaries


class Session:
    """Minimal tf.Session look-alike: `with Session() as sess: sess.run(fetches, feed_dict)`."""
    def __init__(self, device=None):
        self.device = int(os.environ.get('LOCAL_RANK', '0')) if device is None else int(device)
        self.nets = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        for n in self.nets:
            n.close()
        self.nets = []

    def run(self, fetches, feed_dict=None):
        single = not isinstance(fetches, (list, tuple))
        flist = [fetches] if single else list(fetches)
        net = None
        for f in flist:
            owner = getattr(f, 'owner', None) if not isinstance(f, dict) else next(iter(f.values())).owner
            net = owner or net
        if net is None:
            raise ValueError('nothing runnable in fetches')
        out = net._run(flist, feed_dict or {})
        return out[0] if single else out


class SSDVGG:
    def __init__(self, session, preset):
        self.preset = get_preset_by_name(preset) if isinstance(preset, str) else preset
        self.session = session
        self._h = None
        self.weights = 'raw'      # the set the parameters hold: 'ema' after build_from_metagraph took a checkpoint's average
        self.__built = False
        self.__build_names()
        if session is not None:
            session.nets.append(self)

    # ------------------------------------------------------------------ construction
    def build_from_vgg(self, vgg_dir, num_classes, a_trous=True, progress_hook='tqdm', max_batch=32,
                       training=True, seed=42, weights=None, dtype='f32', background_prior=None):
        """ssdvgg.py:96-118.  There is no vgg.zip offline: the VGG-16 trunk starts from
        Xavier-uniform synthetic weights (seed) unless `weights` ({tf_name: array}) or
        `<vgg_dir>/vgg16_ssd.npz` supplies them.  dtype 'f32' (default) or 'bf16' (bf16 activations and
        filter mirrors on the bf16 matrix cores; fp32 master weights, loss and optimizer), or -- training=False only --
        'fp8': the bf16 net with conv3_2 ... mod_conv7 (the fc graph's 7x7 fc6 included) on e4m3 operands; call calibrate_fp8 or set
        fp8_scales before infer; or 'mxfp8': the same layers with one E8M0 block scale per pixel and 32 channels, chosen by each
        producer from its own values -- no calibration, infer works at once and an image's result depends on that image alone
        (the fc graph's 7x7 fc6 stays on bf16 unless the environment has SSD_MXFP8_BIGK=1 when the net is built); or 'mxfp6': the
        mxfp8 net's layers and pools on 6-bit e2m3 operands with E8M0 block scales on activations and filters, again without
        calibration (the fc graph's 7x7 fc6 stays on bf16).
        a_trous=False builds the reference's other graph (ssdvgg.py:210-228): VGG-16's fc6 / fc7 as a 7x7 and a
        1x1 convolution, 4096 wide, variables fc6/* and fc7/*; its weights come from `<vgg_dir>/vgg16_ssd_fc.npz`.
        background_prior=P (0 < P < 1; the focal loss's start): after everything else, every classifier's biases are
        set so that an untrained anchor gives each of the C object classes the probability P / C: the background entry
        log(C * (1 - P) / P), the other class entries 0 (the four offset entries keep their values)."""
        if background_prior is not None and not 0.0 < float(background_prior) < 1.0:
            raise ValueError('background_prior must lie in (0, 1), got %r' % (background_prior,))
        self.num_classes = num_classes + 1
        self.num_vars = num_classes + 5
        self._create(num_classes, max_batch, training, seed, dtype, a_trous)
        path = os.path.join(vgg_dir, 'vgg16_ssd.npz' if a_trous else 'vgg16_ssd_fc.npz') if vgg_dir else None
        if weights is None and path and os.path.exists(path):
            weights = dict(np.load(path))
        if weights:
            self.load_variables(weights)
        if background_prior is not None:
            p = float(background_prior)
            names = [n for n, _ in self.variables() if n.startswith('classifiers/') and n.endswith('/biases')]
            biases = self.save_variables(names)
            for a in biases.values():
                a[:num_classes] = 0.0
                a[num_classes] = np.log(num_classes * (1.0 - p) / p)
            self.load_variables(biases)
        self.__built = True

    def build_from_metagraph(self, metagraph_file, checkpoint_file, max_batch=32, training=False, dtype='f32', weights='auto'):
        """ssdvgg.py:120-130: restore a trained net.  checkpoint_file is an .npz written by
        save_checkpoint (variables under the reference's TF names + preset/num_classes).
        weights: which set of a run with a weight EMA becomes the parameters.  'raw': the variables, the last
        iterate; 'ema': the averages under __ema__/<name> in their place (an error if the file has none); 'auto' (the default):
        'ema' for training=False when the file has them, else 'raw' -- so a file without them loads as before under every dtype.
        With training=True the raw weights always go to the parameters (build_optimizer_from_metagraph restores the average)."""
        if weights not in WEIGHT_SETS:
            raise ValueError('weights must be one of %s, got %r' % (list(WEIGHT_SETS), weights))
        ck = np.load(checkpoint_file, allow_pickle=False)
        num_classes = int(ck['__num_classes__'])
        self.num_classes = num_classes + 1
        self.num_vars = num_classes + 5
        a_trous = bool(int(ck['__a_trous__'])) if '__a_trous__' in ck.files else True      # (older checkpoints: a-trous)
        has_ema = checkpoint_has_ema(ck)
        if weights == 'ema' and not has_ema:
            raise ValueError(NO_EMA_IN_FILE % (checkpoint_file,))
        self._create(num_classes, max_batch, training, 0, dtype, a_trous)
        self.weights = 'ema' if has_ema and not training and weights != 'raw' else 'raw'      # the set the parameters hold
        if self.weights == 'ema':      # (save_checkpoint writes an average for every variable)
            self.load_variables({k[len('__ema__/'):]: ck[k] for k in ck.files if k.startswith('__ema__/')})
        else:
            self.load_variables({k: ck[k] for k in ck.files if not k.startswith('__')})
        self._ckpt = ck
        self.__built = True

    def _create(self, num_classes, max_batch, training, seed, dtype='f32', a_trous=True):
        import torch
        if dtype not in DTYPES:
            raise ValueError("dtype must be 'f32', 'bf16' or 'fp8' (with block scales: 'mxfp8', 'mxfp6'), got %r" % (dtype,))
        if dtype in ('fp8', 'mxfp8', 'mxfp6') and training:
            raise ValueError("dtype %r is inference only: build with training=False" % (dtype,))
        self.dtype = dtype
        dev = self.session.device if self.session is not None else 0
        self.device = dev
        self.max_batch = int(max_batch)
        self.training = bool(training)
        self.a_trous = bool(a_trous)
        graph = 0 if self.a_trous else 1      # SSD_GRAPH_A_TROUS / SSD_GRAPH_FC
        n = lib.ssd_arena_floats_graph(self.preset.name.encode(), num_classes, graph)
        if n == 0:
            raise RuntimeError(_lib.last_error())
        tdev = torch.device('cuda', dev)
        self.params_flat = torch.empty(n, dtype=torch.float32, device=tdev)
        self.grads_flat = torch.zeros(n, dtype=torch.float32, device=tdev) if training else None
        self.momentum_flat = torch.zeros(n, dtype=torch.float32, device=tdev) if training else None
        h = C.c_void_p()
        check(lib.ssd_create_graph(self.preset.name.encode(), num_classes, self.max_batch, dev, int(training), seed,
                                   self.params_flat.data_ptr(),
                                   self.grads_flat.data_ptr() if training else None,
                                   self.momentum_flat.data_ptr() if training else None,
                                   DTYPES[dtype], graph, C.byref(h)))
        self._h = h
        fl = C.c_size_t(); ff = C.c_size_t()
        check(lib.ssd_arenas(h, None, None, None, C.byref(fl), C.byref(ff)))
        self.arena_floats, self.filter_floats = fl.value, ff.value
        self._n_classes = num_classes
        # tokens the callers feed / fetch (ssdvgg.py:128-150,193-194,378,593-599)
        self.image_input = self._tok('image_input:0')
        self.keep_prob = self._tok('keep_prob:0')
        self.result = self._tok('result/result:0')
        self.labels = None
        self.losses = None
        self.optimizer = None
        self.eval_op = None

    def _tok(self, name):
        t = _Token(name)
        t.owner = self
        return t

    def close(self):
        if self._h is not None:
            lib.ssd_destroy(self._h)
            self._h = None
            if hasattr(self, '_det_views'):
                self._det_views.clear()      # (views of pinned memory that ssd_destroy has just freed)
            self._bf16_messages = None       # (parallel.Bf16Message buffers of this handle's gradient arena)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ optimizer
    def build_optimizer(self, learning_rate=0.001, weight_decay=0.0005, momentum=0.9, global_step=None, loss='mining',
                        focal_gamma=2.0, focal_alpha=0.25, loc_loss='smooth_l1', loc_weight=1.0, clip_norm=0.0, optimizer='momentum',
                        adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8, adam_decay=0.01, ema_decay=0.0):
        """ssdvgg.py:375-599.  learning_rate: float or LearningRate (train.py:43-47).  loss: 'mining' (the reference's 3:1
        hard-negative mining) or 'focal' (every anchor, damped by (1 - p_t)^focal_gamma and weighted focal_alpha on positives,
        1 - focal_alpha on background; a sample without positives still trains its background anchors).
        loc_loss: 'smooth_l1' (the reference's, on the four encoded offsets) or 'giou' (loc_weight * (1 - GIoU) of the predicted
        against the ground-truth box of every positive anchor); either goes with either `loss`.
        clip_norm: clip the gradient by its global norm in the update (0, the default: off; inf: measure only).
        optimizer: 'momentum' (the reference's rule, the default) or 'adamw'  with adam_beta1, adam_beta2, adam_eps
        and the decoupled adam_decay on the filters; under 'adamw' `momentum` is ignored and `weight_decay` stays the L2 term of
        the loss (0 gives pure AdamW).  Changing the rule zeroes the accumulators.
        ema_decay: keep an exponential moving average of the weights behind every update (0, the default: off);
        averaged_weights() evaluates on it and save_checkpoint keeps both sets."""
        if not self.training:
            raise RuntimeError('build_from_* was called with training=False')
        self.set_loss(loss, focal_gamma, focal_alpha)
        self.set_loc_loss(loc_loss, loc_weight)
        self.set_grad_clip(clip_norm)
        self.set_update_rule(optimizer, adam_beta1, adam_beta2, adam_eps, adam_decay)
        self.set_ema(ema_decay)
        lr = learning_rate if isinstance(learning_rate, LearningRate) else LearningRate([learning_rate], [])
        vals = np.array(lr.values, np.float32)
        bnds = np.array(lr.boundaries + [0], np.int64)
        check(lib.ssd_set_optimizer(self._h, np_ptr(vals), np_ptr(bnds), len(lr.values), float(momentum), float(weight_decay)))
        if global_step is not None:
            check(lib.ssd_set_global_step(self._h, int(global_step)))
        self.labels = self._tok('labels:0')
        self.optimizer = self._tok('optimizer/optimizer')
        self.eval_op = self._tok('total_loss/loss:0 (deferred)')      # forward + loss without the update; read with get_losses_step
        self.losses = {k: self._tok(n) for k, n in zip(
            LOSS_NAMES, ('total_loss/loss:0', 'localization_loss/localization_loss:0',
                         'confidence_loss/confidence_loss:0', 'total_loss/l2_loss:0'))}

    def build_optimizer_from_metagraph(self):
        """ssdvgg.py:133-150: optimizer state (momentum, global_step, schedule) from the checkpoint."""
        ck = getattr(self, '_ckpt', None)
        if ck is None:
            raise RuntimeError('build_from_metagraph first')
        lr = LearningRate(list(ck['__lr_values__']), list(ck['__lr_boundaries__']))
        loss, gamma, alpha = checkpoint_loss(ck)
        loc_loss, loc_weight = checkpoint_loc_loss(ck)
        rule, b1, b2, eps, decay = checkpoint_update_rule(ck)
        self.build_optimizer(lr, float(ck['__weight_decay__']), float(ck['__momentum__']), int(ck['__global_step__']),
                             loss=loss, focal_gamma=gamma, focal_alpha=alpha, loc_loss=loc_loss, loc_weight=loc_weight,
                             clip_norm=checkpoint_clip_norm(ck), optimizer=rule, adam_beta1=b1, adam_beta2=b2, adam_eps=eps,
                             adam_decay=decay, ema_decay=checkpoint_ema(ck))
        for k in ck.files:
            if k.startswith('__momentum__/'):
                a = np.ascontiguousarray(ck[k], np.float32)
                check(lib.ssd_load_momentum(self._h, k[len('__momentum__/'):].encode(), np_ptr(a), a.size))
            elif k.startswith('__adam_v__/'):
                a = np.ascontiguousarray(ck[k], np.float32)
                check(lib.ssd_load_second_moment(self._h, k[len('__adam_v__/'):].encode(), np_ptr(a), a.size))
            elif k.startswith('__ema__/'):
                a = np.ascontiguousarray(ck[k], np.float32)
                check(lib.ssd_load_ema(self._h, k[len('__ema__/'):].encode(), np_ptr(a), a.size))
        if rule == 'adamw':
            check(lib.ssd_set_adam_step(self._h, int(ck['__adam_step__'])))
        if checkpoint_ema(ck) != 0.0:
            check(lib.ssd_set_ema_step(self._h, int(ck['__ema_step__'])))

    def build_summaries(self, restore):
        """ssdvgg.py:625-649 builds TensorBoard histograms; observability is out of scope here."""
        return None

    # ------------------------------------------------------------------ variables
    def variables(self):
        """[(tf_name, shape)] in arena order."""
        out = []
        buf = C.create_string_buffer(128)
        nd = C.c_int(); shp = (C.c_int * 4)()
        for i in range(lib.ssd_num_variables(self._h)):
            check(lib.ssd_variable_info(self._h, i, buf, 128, C.byref(nd), shp))
            out.append((buf.value.decode(), tuple(shp[k] for k in range(nd.value))))
        return out

    def load_variables(self, weights):
        known = dict(self.variables())
        for name, arr in weights.items():
            if name not in known:
                raise RuntimeError('no such variable: ' + name)
            a = np.ascontiguousarray(arr, np.float32)
            if tuple(a.shape) != known[name]:
                raise ValueError(f'{name}: shape {a.shape}, expected {known[name]}')
            check(lib.ssd_load_variable(self._h, name.encode(), np_ptr(a), a.size))

    def _save(self, fn, names=None):
        out = {}
        for name, shape in self.variables():
            if names is not None and name not in names:
                continue
            a = np.empty(shape, np.float32)
            check(fn(self._h, name.encode(), np_ptr(a), a.size))
            out[name] = a
        return out

    def save_variables(self, names=None):
        return self._save(lib.ssd_save_variable, names)

    def save_gradients(self, names=None):
        return self._save(lib.ssd_save_gradient, names)

    def save_momentum(self, names=None):
        return self._save(lib.ssd_save_momentum, names)

    def save_second_moment(self, names=None):
        """AdamW's second moment by variable name; an error while the handle has never been under AdamW"""
        return self._save(lib.ssd_save_second_moment, names)

    # ------------------------------------------------------------------ weight EMA
    def set_ema(self, decay=0.0):
        """Keep an exponential moving average of the weights behind every update from the next one on (ssd_set_ema): decay in
        (0, 1), warmed up as min(decay, (1 + t) / (10 + t)).  Switching it on copies the current weights and counts from t = 0;
        another decay while it is on keeps the average and t; 0 switches it off."""
        check(lib.ssd_set_ema(self._h, ema_decay_config(decay)))

    def get_ema(self):
        """(decay, t, swapped): the decay (0.0: off), the count of EMA updates since it was switched on, and whether the average
        is swapped in (swap_ema)"""
        d = C.c_float(); t = C.c_longlong(); s = C.c_int()
        check(lib.ssd_get_ema(self._h, C.byref(d), C.byref(t), C.byref(s)))
        return float(d.value), t.value, bool(s.value)

    def save_ema(self, names=None):
        """The averaged weights by variable name (while swapped: the raw ones, and save_variables the averaged); an error while
        the handle has never had the EMA on"""
        return self._save(lib.ssd_save_ema, names)

    def swap_ema(self):
        """Exchange the contents of the parameters and the average on the GPU (ssd_ema_swap): forward, detect and
        save_variables then run on the average until the next call; updates, backward and loads are refused meanwhile."""
        check(lib.ssd_ema_swap(self._h))

    @contextlib.contextmanager
    def averaged_weights(self):
        """`with net.averaged_weights():` -- the block runs on the averaged weights; the raw ones are back when it is left, by an
        exception too.  With the EMA off (or inside another such block) it does nothing, so callers need no branch."""
        on = False
        if self.training:
            decay, _, swapped = self.get_ema()
            on = decay != 0.0 and not swapped
        if on:
            self.swap_ema()
        try:
            yield on
        finally:
            if on:
                self.swap_ema()

    @property
    def adam_step(self):
        """AdamW updates since the accumulators were zeroed (the t of the bias corrections)"""
        t = C.c_longlong()
        check(lib.ssd_get_adam_step(self._h, C.byref(t)))
        return t.value

    @property
    def global_step(self):
        s = C.c_longlong()
        check(lib.ssd_get_global_step(self._h, C.byref(s)))
        return s.value

    def save_checkpoint(self, path, lr=None, momentum=0.9, weight_decay=0.0005, class_names=None, match='reference'):
        """tf.train.Saver.save counterpart (train.py:336-343): one .npz, reference variable names.  `class_names`
        (one per class id; default: training_data.default_class_names) is stored as a unicode array, no pickle; `match`, the
        matching rule the labels of the run were encoded with, as a string under __match__."""
        from .training_data import default_class_names
        from .ssdutils import match_id
        match_id(match)
        if self.training and self.get_ema()[2]:
            raise RuntimeError('weight EMA: save_checkpoint is refused while the average is swapped in (leave averaged_weights() first)')
        names = list(class_names) if class_names is not None else default_class_names(self._n_classes)
        if len(names) != self._n_classes:
            raise ValueError(f'{len(names)} class names for {self._n_classes} classes')
        d = self.save_variables()
        if self.training:
            d.update({'__momentum__/' + k: v for k, v in self.save_momentum().items()})
        lr = lr or LearningRate([0.001], [])
        d.update(__preset__=np.array(self.preset.name), __num_classes__=np.array(self._n_classes),
                 __global_step__=np.array(self.global_step), __lr_values__=np.array(lr.values, np.float64),
                 __lr_boundaries__=np.array(lr.boundaries, np.int64), __momentum__=np.array(momentum),
                 __weight_decay__=np.array(weight_decay), __class_names__=np.array([str(n) for n in names], dtype=np.str_),
                 __a_trous__=np.array(int(self.a_trous)), __match__=np.array(str(match)))
        if self.training:
            loss, gamma, alpha = self.get_loss()
            d.update(__loss__=np.array(loss), __focal_gamma__=np.array(gamma), __focal_alpha__=np.array(alpha))
            loc_loss, loc_weight = self.get_loc_loss()
            d.update(__loc_loss__=np.array(loc_loss), __loc_weight__=np.array(loc_weight))
            d.update(__clip_norm__=np.array(self.get_grad_clip()))
            rule, b1, b2, eps, decay = self.get_update_rule()
            if rule != 'momentum':      # (a momentum run's file holds the keys it held before the option)
                d.update(__optimizer__=np.array(rule), __adam_beta1__=np.array(b1, np.float32), __adam_beta2__=np.array(b2, np.float32),
                         __adam_eps__=np.array(eps, np.float32), __adam_decay__=np.array(decay, np.float32),
                         __adam_step__=np.array(self.adam_step, np.int64))
                d.update({'__adam_v__/' + k: v for k, v in self.save_second_moment().items()})
            ema_decay, ema_step, _ = self.get_ema()
            if ema_decay != 0.0:        # (a run without the average writes the keys it wrote before the option)
                d.update(__ema_decay__=np.array(ema_decay, np.float32), __ema_step__=np.array(ema_step, np.int64))
                d.update({'__ema__/' + k: v for k, v in self.save_ema().items()})
        np.savez(path, **d)

    # ------------------------------------------------------------------ steps
    def _check_x(self, x):
        x = np.ascontiguousarray(x, np.float32)
        H, W = self.preset.image_size.h, self.preset.image_size.w
        if x.ndim != 4 or x.shape[1:] != (H, W, 3):
            raise ValueError(f'image_input must be [b, {H}, {W}, 3] float32, got {x.shape}')   # data_queue.py:63-79
        if x.shape[0] < 1 or x.shape[0] > self.max_batch:
            raise ValueError(f'batch {x.shape[0]} outside 1..{self.max_batch} (max_batch)')
        return x

    def _check_y(self, y, b):
        y = np.ascontiguousarray(y, np.float32)
        if y.shape != (b, self.preset.num_anchors, self.num_vars):
            raise ValueError(f'labels must be [{b}, {self.preset.num_anchors}, {self.num_vars}] float32, got {y.shape}')
        return y

    # ---- device-resident feeds: a torch CUDA tensor in the feed goes through the *_dev entry points --------------
    @staticmethod
    def _is_cuda(t):
        return hasattr(t, 'is_cuda') and t.is_cuda

    def _dev_xy(self, x, y):
        import torch
        H, W = self.preset.image_size.h, self.preset.image_size.w
        if x.dtype != torch.float32 or x.dim() != 4 or tuple(x.shape[1:]) != (H, W, 3):
            raise ValueError(f'image_input must be [b, {H}, {W}, 3] float32, got {tuple(x.shape)} {x.dtype}')
        if x.shape[0] < 1 or x.shape[0] > self.max_batch:
            raise ValueError(f'batch {x.shape[0]} outside 1..{self.max_batch} (max_batch)')
        x = x.contiguous()
        if y is not None:
            if not self._is_cuda(y):
                y = torch.from_numpy(self._check_y(y, x.shape[0])).to(x.device)
            if y.dtype != torch.float32 or tuple(y.shape) != (x.shape[0], self.preset.num_anchors, self.num_vars):
                raise ValueError(f'labels must be [{x.shape[0]}, {self.preset.num_anchors}, {self.num_vars}] float32, got {tuple(y.shape)}')
            y = y.contiguous()
        return x, y

    def _dev_result(self, b, want_result):
        if not want_result:
            return None
        res = np.empty((b, self.preset.num_anchors, self.num_vars), np.float32)
        check(lib.ssd_get_result(self._h, b, np_ptr(res)))
        return res

    def train_step(self, x, y, want_result=True, want_losses=True):
        if self._is_cuda(x):
            x, y = self._dev_xy(x, y)
            self.train_step_dev(x, y)
            # neither fetch: nothing waits for the step (the driver reads the losses one step late, get_losses_step)
            return self._dev_result(x.shape[0], want_result), (self.get_losses() if want_losses else None)
        x = self._check_x(x); y = self._check_y(y, x.shape[0])
        res = np.empty(y.shape, np.float32) if want_result else None
        L = np.zeros(4, np.float32)
        check(lib.ssd_train_step(self._h, np_ptr(x), np_ptr(y), x.shape[0], np_ptr(res), np_ptr(L)))
        return res, dict(zip(LOSS_NAMES, (float(v) for v in L)))

    def eval_step(self, x, y, want_result=True, want_losses=True):
        if self._is_cuda(x):
            x, y = self._dev_xy(x, y)
            self.eval_step_dev(x, y)
            return self._dev_result(x.shape[0], want_result), (self.get_losses() if want_losses else None)
        x = self._check_x(x); y = self._check_y(y, x.shape[0])
        res = np.empty(y.shape, np.float32) if want_result else None
        L = np.zeros(4, np.float32)
        check(lib.ssd_eval_step(self._h, np_ptr(x), np_ptr(y), x.shape[0], np_ptr(res), np_ptr(L)))
        return res, dict(zip(LOSS_NAMES, (float(v) for v in L)))

    def infer(self, x):
        if self._is_cuda(x):
            x, _ = self._dev_xy(x, None)
            self.infer_dev(x)
            return self._dev_result(x.shape[0], True)
        x = self._check_x(x)
        res = np.empty((x.shape[0], self.preset.num_anchors, self.num_vars), np.float32)
        check(lib.ssd_infer(self._h, np_ptr(x), x.shape[0], np_ptr(res)))
        return res

    # ------------------------------------------------------------------ fp8 inference (dtype='fp8')
    def calibrate_fp8(self, x, accumulate=False):
        """Set the fp8 activation scales from a batch (numpy or a torch tensor on this net's GPU): the graph runs once on the
        bf16 kernels and every e4m3 tensor gets scale = max(absmax, tiny) / 448; accumulate=True keeps the larger of that and
        the scale already there (several calibration batches)."""
        import torch
        if self._is_cuda(x):
            x, _ = self._dev_xy(x, None)
        else:
            x = torch.from_numpy(self._check_x(x)).to(torch.device('cuda', self.device))
        check(lib.ssd_fp8_calibrate_dev(self._h, x.data_ptr(), x.shape[0], int(bool(accumulate))))

    def _fp8_names(self):
        n = C.c_int()
        check(lib.ssd_fp8_num_scales(self._h, C.byref(n)))
        names = []
        for i in range(n.value):
            buf = C.create_string_buffer(128)
            check(lib.ssd_fp8_scale_name(self._h, i, buf, 128))
            names.append(buf.value.decode())
        return names

    @property
    def fp8_scales(self):
        """{tensor name: scale} of an fp8 net, in graph order (0.0 before calibration)."""
        names = self._fp8_names()
        v = np.zeros(len(names), np.float32)
        check(lib.ssd_fp8_get_scales(self._h, np_ptr(v), len(names)))
        return dict(zip(names, (float(s) for s in v)))

    @fp8_scales.setter
    def fp8_scales(self, scales):
        names = self._fp8_names()
        missing = [n for n in names if n not in scales]
        extra = [n for n in scales if n not in names]
        if missing or extra:
            raise ValueError(f'fp8_scales needs exactly {names}; missing {missing}, unknown {extra}')
        v = np.array([scales[n] for n in names], np.float32)
        check(lib.ssd_fp8_set_scales(self._h, np_ptr(v), len(names)))

    def activation(self, name, b):
        H = C.c_int(); W = C.c_int(); Ch = C.c_int()
        check(lib.ssd_activation_shape(self._h, name.encode(), C.byref(H), C.byref(W), C.byref(Ch)))
        a = np.empty((b, H.value, W.value, Ch.value), np.float32)
        check(lib.ssd_activation(self._h, name.encode(), b, np_ptr(a), a.size))
        return a

    def pool_fusion(self):
        """Per 2x2 stride-2 pool of the graph (pool1 ... in graph order): (fused into its producer's forward epilogue, fused into
        its consumer's data gradient).  A fused pool's input / its output gradient are not materialised (activation() refuses)."""
        out = (C.c_int * 8)()
        n = C.c_int()
        check(lib.ssd_pool_fusion(self._h, out, 8, C.byref(n)))
        return [(bool(out[i] & 1), bool(out[i] & 2)) for i in range(n.value)]

    # device-resident steps (torch tensors on this net's GPU)
    def forward_backward_dev(self, x_t, y_t):
        check(lib.ssd_forward_backward_dev(self._h, x_t.data_ptr(), y_t.data_ptr(), x_t.shape[0]))

    def forward_dev(self, x_t, y_t):
        check(lib.ssd_forward_dev(self._h, x_t.data_ptr(), y_t.data_ptr(), x_t.shape[0]))

    def use_torch_wgrad_stream(self):
        """Run the weight gradients on a torch-owned side stream (returned) so collectives can be enqueued
        behind exactly that stream while the data gradients keep running on the current stream."""
        import torch
        if getattr(self, 'wgrad_stream', None) is None:
            self.wgrad_stream = torch.cuda.Stream(device=self.device)
            check(lib.ssd_set_wgrad_stream(self._h, self.wgrad_stream.cuda_stream))
        return self.wgrad_stream

    def backward_staged(self, y_t, b, min_floats, sync_main=True):
        """Generator over (offset, count) ranges of the gradient arena as backward finishes them."""
        check(lib.ssd_backward_begin_dev(self._h, y_t.data_ptr(), b))
        off = C.c_size_t(); cnt = C.c_size_t(); more = C.c_int(1)
        while more.value:
            check(lib.ssd_backward_next_dev(self._h, int(min_floats), int(sync_main), C.byref(off), C.byref(cnt), C.byref(more)))
            if cnt.value:
                yield off.value, cnt.value

    def backward_ranges(self, min_floats):
        """[(offset, count)] exactly as backward_staged(..., min_floats) yields them, without running backward."""
        cap = 128
        while True:
            offs = (C.c_size_t * cap)(); cnts = (C.c_size_t * cap)(); n = C.c_int()
            check(lib.ssd_backward_ranges(self._h, int(min_floats), offs, cnts, cap, C.byref(n)))
            if n.value <= cap:      # (a truncated list would desynchronise the ranks' collectives: ask again with room for all)
                return [(offs[i], cnts[i]) for i in range(n.value)]
            cap = n.value

    def set_loss_normalizer(self, batch):
        """reduce_mean over `batch` samples instead of the step's own b (<= 0 restores the default): data
        parallel shards of unequal size pass global_samples / world (parallel.train_step_dp)."""
        check(lib.ssd_set_loss_normalizer(self._h, float(batch)))

    def set_loss(self, loss='mining', focal_gamma=2.0, focal_alpha=0.25):
        """The loss of the steps from the next one on (ssd_set_loss): 'mining' or 'focal' (build_optimizer)."""
        cfg = loss_config(loss, focal_gamma, focal_alpha)
        check(lib.ssd_set_loss(self._h, C.byref(cfg)))

    def set_loc_loss(self, loc_loss='smooth_l1', loc_weight=1.0):
        """The localization loss of the steps from the next one on (ssd_set_loc_loss): 'smooth_l1' or 'giou' (build_optimizer)."""
        cfg = loc_loss_config(loc_loss, loc_weight)
        check(lib.ssd_set_loc_loss(self._h, C.byref(cfg)))

    def get_loc_loss(self):
        """(name, weight) of the handle's localization loss"""
        cfg = LocLossConfig()
        check(lib.ssd_get_loc_loss(self._h, C.byref(cfg)))
        return [k for k, v in LOC_LOSS_KINDS.items() if v == cfg.kind][0], float(cfg.weight)

    def set_grad_clip(self, clip_norm=0.0):
        """Clip the gradient by its global norm from the next update on (ssd_set_grad_clip): 0 off, > 0 the threshold, inf
        measures only (build_optimizer)."""
        cfg = grad_clip_config(clip_norm)
        check(lib.ssd_set_grad_clip(self._h, C.byref(cfg)))

    def get_grad_clip(self):
        """clip_norm of the handle"""
        cfg = GradClipConfig()
        check(lib.ssd_get_grad_clip(self._h, C.byref(cfg)))
        return float(cfg.max_norm)

    def get_grad_norm_step(self, steps_back=0):
        """(norm, factor) of the last clipped or measured update (0) or of the one 1 / 2 before it, waiting only for THAT update
        (ssd_get_grad_norm_step).  factor 1: not clipped; in (0, 1): clipped; 0: skipped, the gradient was not finite."""
        out = np.zeros(2, np.float32)
        check(lib.ssd_get_grad_norm_step(self._h, int(steps_back), np_ptr(out)))
        return float(out[0]), float(out[1])

    def set_update_rule(self, optimizer='momentum', adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8, adam_decay=0.01):
        """The rule of the updates from the next one on (ssd_set_update_rule; build_optimizer).  Another rule than the handle's
        zeroes the accumulators and the AdamW step count; the same rule with other hyper-parameters keeps them."""
        cfg = update_rule_config(optimizer, adam_beta1, adam_beta2, adam_eps, adam_decay)
        check(lib.ssd_set_update_rule(self._h, C.byref(cfg)))

    def get_update_rule(self):
        """(name, beta1, beta2, eps, decay) of the handle's update rule"""
        cfg = UpdateRuleConfig()
        check(lib.ssd_get_update_rule(self._h, C.byref(cfg)))
        return ([k for k, v in UPDATE_KINDS.items() if v == cfg.kind][0], float(cfg.beta1), float(cfg.beta2), float(cfg.eps),
                float(cfg.decay))

    def get_loss(self):
        """(name, focal_gamma, focal_alpha) of the handle's loss"""
        cfg = LossConfig()
        check(lib.ssd_get_loss(self._h, C.byref(cfg)))
        return [k for k, v in LOSS_KINDS.items() if v == cfg.kind][0], float(cfg.focal_gamma), float(cfg.focal_alpha)

    def null_gradients_dev(self):
        """The gradient arena of a step without samples: weight_decay * filters, zero elsewhere."""
        check(lib.ssd_null_gradients_dev(self._h))

    def apply_gradients_dev(self, grad_scale=1.0):
        check(lib.ssd_apply_gradients_dev(self._h, float(grad_scale)))

    def train_step_dev(self, x_t, y_t):
        check(lib.ssd_train_step_dev(self._h, x_t.data_ptr(), y_t.data_ptr(), x_t.shape[0]))

    def eval_step_dev(self, x_t, y_t):
        check(lib.ssd_eval_step_dev(self._h, x_t.data_ptr(), y_t.data_ptr(), x_t.shape[0]))

    def infer_dev(self, x_t):
        check(lib.ssd_infer_dev(self._h, x_t.data_ptr(), x_t.shape[0]))

    def get_losses(self):
        L = np.zeros(4, np.float32)
        check(lib.ssd_get_losses(self._h, np_ptr(L)))
        return dict(zip(LOSS_NAMES, (float(v) for v in L)))

    def get_losses_step(self, steps_back=0):
        """The losses of the last step (0) or of the step 1 / 2 before it, waiting only for THAT step's forward pass
        (ssd_get_losses_step): a driver books step k - 1 after launching step k instead of stalling on every step."""
        L = np.zeros(4, np.float32)
        check(lib.ssd_get_losses_step(self._h, int(steps_back), np_ptr(L)))
        return dict(zip(LOSS_NAMES, (float(v) for v in L)))

    def set_stream(self, stream_ptr):
        check(lib.ssd_set_stream(self._h, stream_ptr))
        self._stream_ptr = int(stream_ptr or 0)

    def _det_caps(self, cap, mo):
        cap = -1 if cap is None else int(cap)
        mo = -1 if mo is None else int(mo)
        out_cap = self.preset.num_anchors if cap < 0 else max(cap, 1)
        if mo >= 0:
            out_cap = max(min(out_cap, mo), 1)
        return cap, mo, out_cap

    def detect_last_launch(self, b, confidence_threshold=0.5, detections_cap=200, max_out=None, nms=True, decode='argmax',
                           nms_top_k=400, keep_top_k=200, soft_nms=None, soft_nms_iou=0.45, soft_nms_sigma=0.5, soft_nms_min_score=None):
        """Enqueue decode + NMS of the last step's result and the copy of its (small) output; returns a
        ticket whose get() yields what detect_last returns.  Two output slots alternate in the handle, so a
        caller may launch the next batch before it collects this one (infer.py:225-235, pipelined).
        decode='argmax': the reference's decode_boxes + suppress_overlaps (one candidate per anchor).  decode='all': the SSD
        paper's DetectionOutput (ssd_detect_last_all_dev) -- every class of an anchor is a candidate, the best
        nms_top_k per class, NMS per class, the best keep_top_k of the image in global confidence order; detections_cap,
        max_out and nms do not apply and must be left at their defaults.  soft_nms = 'linear' | 'gaussian' (decode='all' only,
        DESIGN.md 38): Soft-NMS in the place of the NMS per class (ssd_detect_last_all_soft_dev; ssdutils.detection_output_batch
        describes the keywords); the boolean `nms` keeps its meaning for the argmax decode."""
        from .ssdutils import soft_nms_params
        soft = soft_nms_params(soft_nms, soft_nms_iou, soft_nms_sigma, soft_nms_min_score, confidence_threshold)
        if soft is not None and decode != 'all':
            raise ValueError("soft_nms needs decode='all': the argmax decode keeps the hard rule")
        count_dev = C.c_void_p(); conf_dev = C.c_void_p(); cls_dev = C.c_void_p(); box_dev = C.c_void_p()
        if decode == 'all':
            if detections_cap != 200 or max_out is not None or nms is not True:
                raise ValueError("decode='all' takes nms_top_k and keep_top_k; detections_cap, max_out and nms do not apply")
            out_cap = max(int(keep_top_k), 1)
            args = (self._h, b, float(confidence_threshold), int(nms_top_k), int(keep_top_k), out_cap, C.byref(count_dev),
                    C.byref(conf_dev), C.byref(cls_dev), None, C.byref(box_dev))
            if soft is None:
                check(lib.ssd_detect_last_all_dev(*args))
            else:
                check(lib.ssd_detect_last_all_soft_dev(*args, C.cast(C.pointer(soft), C.c_void_p)))
        elif decode == 'argmax':
            cap, mo, out_cap = self._det_caps(detections_cap, max_out)
            check(lib.ssd_detect_last_dev(self._h, b, float(confidence_threshold), cap, mo, out_cap, 1 if nms else 0,
                                          C.byref(count_dev), C.byref(conf_dev), C.byref(cls_dev), None, C.byref(box_dev)))
        else:
            raise ValueError("decode must be 'argmax' or 'all' (got %r)" % (decode,))
        self._det_serial = getattr(self, '_det_serial', 0) + 1
        self._det_dev = (self._det_serial, count_dev.value, cls_dev.value, box_dev.value, b, out_cap)      # (annotate_last_launch)
        if not hasattr(self, '_det_views'):
            self._det_views = {}
        return _Detections(self, self._det_serial, b, out_cap, (count_dev.value, conf_dev.value, cls_dev.value, box_dev.value))

    def annotate_last_launch(self, src, src_offs, src_shapes, style, dst_shapes=None, rgb_out=False, keep_device=False, to_host=True):
        """Enqueue, right behind the decode that detect_last_launch has just launched and on the same stream, the drawing of its
        detections (annotate.annotate_batch; the boxes are read from the pass's device-visible slot, nothing waits).  src: a
        torch uint8 or float32 CUDA tensor holding image i as [h][w][3] BGR at byte offset src_offs[i] (src_shapes[i] = (h, w));
        dst_shapes: other output sizes (float32 sources only: cv2.resize first); fewer images than the pass held: its first ones.  Returns a ticket whose get() yields the
        uint8 [h, w, 3] images from pinned host memory; collect it with the pass's detections.  keep_device: the ticket also
        carries the device tensor (`dev`, `offs`, `shapes`, `stream`: what jpeg.encode_launch takes); to_host=False: the pixels are
        not copied to the host at all (get() then raises)."""
        import torch
        from . import annotate as A
        det = getattr(self, '_det_dev', None)
        if det is None or det[0] != self._det_serial:
            raise RuntimeError('annotate_last_launch needs a detect_last_launch right before it')
        _, count_dev, cls_dev, box_dev, b, out_cap = det
        if not 1 <= len(src_shapes) <= b:      # (fewer: the first images of the pass)
            raise ValueError('%d images for a detection pass of %d' % (len(src_shapes), b))
        ptr = getattr(self, '_stream_ptr', 0)
        stream = torch.cuda.ExternalStream(ptr, device=src.device) if ptr else torch.cuda.default_stream(src.device)
        with torch.cuda.stream(stream):
            dst, offs, shapes = A.annotate_batch(src, src_offs, src_shapes, count_dev, cls_dev, box_dev, out_cap, style,
                                                 dst_shapes=dst_shapes, rgb_out=rgb_out, stream=ptr or None)
            host = None
            if to_host:
                host = torch.empty(dst.shape, dtype=dst.dtype, pin_memory=True)
                host.copy_(dst, non_blocking=True)
            done = torch.cuda.Event()
            done.record(stream)
        return _Annotated(host, done, offs, shapes, dst if keep_device else None, stream if keep_device else None)

    def detect_last(self, b, confidence_threshold=0.5, detections_cap=200, max_out=None, nms=True, decode='argmax', nms_top_k=400,
                    keep_top_k=200, soft_nms=None, soft_nms_iou=0.45, soft_nms_sigma=0.5, soft_nms_min_score=None):
        """decode + NMS of the last step's result without leaving the GPU (train.py:275-277); decode='all': see
        detect_last_launch."""
        # (copies: a caller of this synchronous form may keep the result across any number of later passes)
        return [{k: v.copy() for k, v in d.items()}
                for d in self.detect_last_launch(b, confidence_threshold, detections_cap, max_out, nms, decode, nms_top_k, keep_top_k,
                                                 soft_nms, soft_nms_iou, soft_nms_sigma, soft_nms_min_score).get()]

    # ------------------------------------------------------------------ Session.run routing
    def _run(self, fetches, feed):
        x = feed.get(self.image_input)
        if x is None:
            raise ValueError('feed_dict must hold net.image_input')
        y = feed.get(self.labels) if self.labels is not None else None
        want_opt = any(f is self.optimizer for f in fetches if self.optimizer is not None)
        want_loss = any(isinstance(f, dict) or (self.losses and f in self.losses.values()) for f in fetches)
        want_res = any(f is self.result for f in fetches)      # the [b, A, C+5] copy to the host only when fetched
        want_eval = any(f is self.eval_op for f in fetches if getattr(self, 'eval_op', None) is not None)
        if want_opt:
            if y is None:
                raise ValueError('feed_dict must hold net.labels')
            res, L = self.train_step(x, y, want_res, want_loss)
        elif want_loss or want_eval:
            if y is None:
                raise ValueError('feed_dict must hold net.labels')
            res, L = self.eval_step(x, y, want_res, want_loss)
        else:
            res, L = self.infer(x), None
        out = []
        for f in fetches:
            if f is self.result:
                out.append(res)
            elif isinstance(f, dict):
                out.append({k: L[k] for k in f})
            elif self.optimizer is not None and f is self.optimizer:
                out.append(None)
            elif getattr(self, 'eval_op', None) is not None and f is self.eval_op:
                out.append(None)
            elif self.losses and f in self.losses.values():
                out.append(L[[k for k, v in self.losses.items() if v is f][0]])
            else:
                raise ValueError(f'cannot fetch {f!r}')
        return out

    # ------------------------------------------------------------------ names (ssdvgg.py:602-622)
    def __build_names(self):
        self.original_scopes = [
            'conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1', 'conv3_2', 'conv3_3', 'conv4_1', 'conv4_2',
            'conv4_3', 'conv5_1', 'conv5_2', 'conv5_3', 'mod_conv6', 'mod_conv7']
        self.new_scopes = ['conv8_1', 'conv8_2', 'conv9_1', 'conv9_2', 'conv10_1', 'conv10_2', 'conv11_1', 'conv11_2']
        if len(self.preset.maps) == 7:
            self.new_scopes += ['conv12_1', 'conv12_2']
        for i in range(len(self.preset.maps)):
            for j in range(2 + len(self.preset.maps[i].aspect_ratios)):
                self.new_scopes.append('classifiers/classifier{}_{}'.format(i, j))
