"""A data source of small JPEG files for the feeder's decoder='gpu' tests (test_feeder_jpeg_cpu.py, test_gpu_feeder_jpeg.py):
`write_dataset` writes files of tests/golden/j1_jpeg.npz and a manifest into a directory, `get_source()` -- what
utils.load_data_source('jpegset') asks for -- reads that manifest back as Sample records, one or two boxes each.  The fixture's
`ok_*_bgr` arrays are libjpeg-turbo's pixels of the `ok_*_jpg` files: handed to TrainingData as `images`, they make the existing
pixel path the reference of every comparison, without Pillow."""
import json
import os

import numpy as np

from ssd_tensorflow_amd.training_data import VOC_NAMES
from ssd_tensorflow_amd.utils import Box, Point, Sample, Size, default_colors

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'j1_jpeg.npz')


def golden():
    return np.load(GOLDEN)


def ok_files(z, min_side=16):
    """[(name, file bytes, bgr pixels)] of the decodable fixture files with both sides >= min_side: all three samplings,
    greyscale, optimised tables, restart intervals"""
    out = []
    for i, name in enumerate(z['ok_names']):
        bgr = z['ok_%d_bgr' % i]
        if min(bgr.shape[:2]) >= min_side:
            out.append(('%02d_%s' % (i, name), z['ok_%d_jpg' % i].tobytes(), bgr))
    return out


def _boxes(k):
    """one or two boxes; every seventh sample's box is so small that few tries of the redraw loop find a positive anchor"""
    if k % 7 == 3:
        return [[k % 20, 0.5, 0.5, 0.07, 0.07]]
    boxes = [[k % 20, 0.5, 0.5, 0.6, 0.6]]
    if k % 2:
        boxes.append([(k + 5) % 20, 0.3, 0.35, 0.3, 0.4])
    return boxes


def write_dataset(root, files, num_valid, npy_beside=False):
    """files: [(name, bytes or uint8 array, (h, w) or pixels)] -- bytes are written as <name>.jpg, an array as <name>.npy; with
    npy_beside the pixels are written as <name>.jpg.npy too (what load_image_bgr prefers to the file: a pixel path without
    Pillow).  The last num_valid files validate.  Returns {filename: pixels} of the entries that came with pixels."""
    root = str(root)
    os.makedirs(root, exist_ok=True)
    entries, images = [], {}
    for k, (name, data, pixels) in enumerate(files):
        if isinstance(data, np.ndarray):
            path = os.path.join(root, name + '.npy')
            np.save(path, data)
            pixels = data
        else:
            path = os.path.join(root, name + '.jpg')
            with open(path, 'wb') as f:
                f.write(data)
        h, w = pixels.shape[:2] if isinstance(pixels, np.ndarray) else pixels
        if isinstance(pixels, np.ndarray):
            images[path] = pixels
            if npy_beside and not path.endswith('.npy'):
                np.save(path + '.npy', pixels)
        entries.append({'file': os.path.basename(path), 'w': int(w), 'h': int(h), 'boxes': _boxes(k),
                        'split': 'valid' if k >= len(files) - num_valid else 'train'})
    with open(os.path.join(root, 'manifest.json'), 'w') as f:
        json.dump(entries, f)
    return images


class JpegSetSource:
    def __init__(self):
        self.num_classes = len(VOC_NAMES)
        self.colors = default_colors(VOC_NAMES)
        self.lid2name = dict(enumerate(VOC_NAMES))
        self.lname2id = {n: i for i, n in self.lid2name.items()}
        self.train_samples, self.valid_samples = [], []
        self.num_train = self.num_valid = 0

    def load_trainval_data(self, data_dir, valid_fraction):
        with open(os.path.join(data_dir, 'manifest.json')) as f:
            entries = json.load(f)
        for e in entries:
            boxes = [Box(self.lid2name[c], c, Point(cx, cy), Size(w, h)) for c, cx, cy, w, h in e['boxes']]
            sample = Sample(os.path.join(data_dir, e['file']), boxes, Size(e['w'], e['h']))
            (self.valid_samples if e['split'] == 'valid' else self.train_samples).append(sample)
        self.num_train, self.num_valid = len(self.train_samples), len(self.valid_samples)


def get_source():
    return JpegSetSource()
