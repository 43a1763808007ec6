"""Scalar summaries of the training driver: the counterparts of the reference's LossSummary and
PrecisionSummary (utils.py:151-199, 236-283) with the same tags, accumulation and per-epoch push --
written as JSON lines (`{"tag": ..., "value": ..., "step": ...}`) instead of TensorBoard event files
(there is no TensorFlow here).  ImageSummary (utils.py:201-233) writes its annotated pictures as PNG files next to them; they
are drawn on the GPU (annotate.py)."""
import json
import os


class SummaryWriter:
    """tf.summary.FileWriter stand-in: one scalars.jsonl under `logdir`."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        self.logdir = logdir
        self.path = os.path.join(logdir, 'scalars.jsonl')
        self._f = open(self.path, 'a')

    def add_scalar(self, tag, value, step):
        self._f.write(json.dumps({'tag': tag, 'value': float(value), 'step': int(step)}) + '\n')

    def flush(self):
        self._f.flush()

    def close(self):
        self._f.close()


class LossSummary:
    """utils.py:236-283: sample-weighted sums of the four losses over an epoch, pushed as
    `<sample_name>_<loss>_loss` = sum / num_samples."""
    loss_names = ['total', 'localization', 'confidence', 'l2']

    def __init__(self, writer, sample_name, num_samples):
        self.writer, self.sample_name, self.num_samples = writer, sample_name, num_samples
        self.loss_values = {k: 0.0 for k in self.loss_names}

    def add(self, values, num_samples):
        for loss in self.loss_names:
            self.loss_values[loss] += values[loss] * num_samples

    def push(self, epoch, reduce=None):
        """reduce: optional callable summing a list of floats over the ranks of a data-parallel job."""
        sums = [self.loss_values[k] for k in self.loss_names]
        if reduce is not None:
            sums = reduce(sums)
        means = {k: v / max(self.num_samples, 1) for k, v in zip(self.loss_names, sums)}
        if self.writer is not None:
            for k, v in means.items():
                self.writer.add_scalar(self.sample_name + '_' + k + '_loss', v, epoch)
        self.loss_values = {k: 0.0 for k in self.loss_names}
        return means


class GradNormSummary:
    """The gradient's global norm at every update of an epoch (--clip-norm; no reference site): `grad_norm` per update, at the
    update's number, and per epoch `grad_norm_median`, `grad_norm_max`, `grad_clipped` and `grad_skipped` (how many updates were
    scaled down, and how many were skipped because their gradient was not finite)."""

    def __init__(self, writer, updates=0):
        self.writer = writer
        self.values = []          # (norm, factor) per update since the last push
        self.updates = updates    # updates before the first one booked here (a continued run: the checkpoint's global step)

    def add(self, norm, factor):
        self.updates += 1
        self.values.append((float(norm), float(factor)))
        if self.writer is not None and factor != 0.0:      # (a skipped update has no finite norm to plot; the epoch counts it)
            self.writer.add_scalar('grad_norm', norm, self.updates)

    def push(self, epoch):
        """{median, max (over the finite norms), clipped, skipped, updates} of the epoch"""
        finite = sorted(n for n, f in self.values if f != 0.0)
        m = len(finite)
        median = 0.0 if not m else finite[m // 2] if m % 2 else 0.5 * (finite[m // 2 - 1] + finite[m // 2])
        out = dict(median=median, max=finite[-1] if m else 0.0, clipped=sum(1 for _, f in self.values if 0.0 < f < 1.0),
                   skipped=sum(1 for _, f in self.values if f == 0.0), updates=len(self.values))
        if self.writer is not None and self.values:
            for k in ('median', 'max'):
                self.writer.add_scalar('grad_norm_' + k, out[k], epoch)
            self.writer.add_scalar('grad_clipped', out['clipped'], epoch)
            self.writer.add_scalar('grad_skipped', out['skipped'], epoch)
        self.values = []
        return out


class PrecisionSummary:
    """utils.py:151-199: `<sample_name>_mAP` and `<sample_name>_AP_<label>` per epoch; nothing when no
    AP could be computed."""

    def __init__(self, writer, sample_name, labels):
        self.writer, self.sample_name, self.labels = writer, sample_name, labels

    def push(self, epoch, mAP, APs):
        if not APs or self.writer is None:
            return
        self.writer.add_scalar(self.sample_name + '_mAP', mAP, epoch)
        for label in self.labels:
            if label in APs:
                self.writer.add_scalar(self.sample_name + '_AP_' + label, APs[label], epoch)


class ImageSummary:
    """utils.py:201-233 / train.py:273-281, 298-306, 328-329: up to three annotated samples of an epoch, 512 x 512 RGB, written as
    `<logdir>/<sample_name>_img/e<epoch>_<i>.png`.  The pictures arrive drawn: StepLoop.run_epoch resizes, draws and converts
    them on the GPU from the batch tensor and the decode's output and collects them here with that batch's detections."""
    SIZE = 512
    COUNT = 3

    def __init__(self, writer, sample_name, colors, lid2name):
        self.writer, self.sample_name = writer, sample_name
        self.names = [str(lid2name[i]) for i in range(len(lid2name))]
        from .utils import default_colors
        cmap = {**default_colors(self.names), **dict(colors or {})}
        self.colors = [cmap[n] for n in self.names]
        self.samples = []
        self._reserved = 0
        self._style = None

    def style(self, device):
        if self._style is None:
            from .annotate import Style
            self._style = Style(self.colors, self.names, device)
        return self._style

    def room(self):
        """how many more pictures this epoch takes"""
        return self.COUNT - self._reserved

    def reserve(self, k):
        self._reserved += k

    def add(self, images):
        self.samples.extend(a.copy() for a in images)

    def push(self, epoch, samples=None):
        """samples: [h, w, 3] uint8 RGB arrays (default: the ones collected since the last push); nothing is written when empty"""
        samples = self.samples if samples is None else samples
        if samples and self.writer is not None:
            from .annotate import png_bytes
            d = os.path.join(self.writer.logdir, self.sample_name + '_img')
            os.makedirs(d, exist_ok=True)
            for i, img in enumerate(samples):
                with open(os.path.join(d, 'e%d_%d.png' % (epoch, i)), 'wb') as f:
                    f.write(png_bytes(img))
        self.samples = []
        self._reserved = 0

    def close(self):
        if self._style is not None:
            self._style.close()
            self._style = None
