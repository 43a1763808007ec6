"""COCOSource: a data source for detection sets in COCO's annotation format (instances_*.json), with the attributes and
methods PascalVOCSource has.  The standard library's json only.

Layout: <dir>/annotations/instances_{train,val}2017.json and <dir>/{train,val}2017/<file_name>.  The categories are mapped to
0..n-1 in ascending category id (COCO's 80 ids run to 90), their names come from the file, num_classes is their number.  Boxes
are COCO's float [x, y, w, h] in pixels; the image size is the file's width / height.  Training takes train2017 without crowd
regions and without boxes of non-positive width or height (images left without boxes are dropped); validation and testing take
val2017 (the test split has no public annotations) with every box a FlaggedBox that carries the annotation's `area`, crowd
regions as crowd=True: what the COCO evaluation (coco_eval.py) reads.  The validation samples of load_trainval_data drop images
without any box, as PascalVOCSource does (the training pipeline encodes labels from every sample); load_test_data keeps them: a
detection in such an image is a false positive of the evaluation.  image_ids[file name] and category_ids[class id] keep
the file's own ids for a results file; image_ids is keyed by the annotation's file_name as it stands (it may carry a directory)."""
import json
import os

from .utils import FlaggedBox, Box, Sample, Size, abs2prop, default_colors


class COCOSource:
    def __init__(self):
        self.num_classes = 0
        self.colors = {}
        self.lid2name = {}
        self.lname2id = {}
        self.category_ids = {}        # class id -> the file's category id
        self.image_ids = {}           # file name -> the file's image id
        self.num_train = self.num_valid = self.num_test = 0
        self.train_samples, self.valid_samples, self.test_samples = [], [], []

    @staticmethod
    def _annotation_file(data_dir, split):
        return os.path.join(data_dir, 'annotations', 'instances_%s.json' % split)

    def _read(self, data_dir, split):
        fn = self._annotation_file(data_dir, split)
        if not os.path.exists(fn):
            raise RuntimeError('No COCO annotation file ' + fn)
        with open(fn) as f:
            doc = json.load(f)
        for key in ('images', 'annotations', 'categories'):
            if key not in doc:
                raise RuntimeError('%s has no "%s": not an instances file' % (fn, key))
        cats = sorted(doc['categories'], key=lambda c: c['id'])
        names = [str(c['name']) for c in cats]
        ids = {k: c['id'] for k, c in enumerate(cats)}
        if self.category_ids and ids != self.category_ids:
            raise RuntimeError(fn + ' has other categories than the annotation file read before')
        self.category_ids = ids
        self.num_classes = len(cats)
        self.lid2name = dict(enumerate(names))
        self.lname2id = {n: k for k, n in enumerate(names)}
        self.colors = default_colors(names)
        return doc

    def _sample_list(self, data_dir, split, training, require_image=True, keep_empty=False):
        doc = self._read(data_dir, split)
        cat2lid = {cid: k for k, cid in self.category_ids.items()}
        by_image = {}
        for a in doc['annotations']:
            by_image.setdefault(a['image_id'], []).append(a)
        samples = []
        for img in doc['images']:
            filename = os.path.join(data_dir, split, img['file_name'])
            if require_image and not os.path.exists(filename):
                continue
            imgsize = Size(int(img['width']), int(img['height']))
            boxes = []
            for a in by_image.get(img['id'], ()):
                x, y, w, h = (float(v) for v in a['bbox'])
                crowd = bool(a.get('iscrowd', 0))
                if training and (crowd or w <= 0 or h <= 0):
                    continue
                k = cat2lid[a['category_id']]
                center, size = abs2prop(x, x + w, y, y + h, imgsize)
                if training:
                    boxes.append(Box(self.lid2name[k], k, center, size))
                else:
                    boxes.append(FlaggedBox(self.lid2name[k], k, center, size, crowd=crowd, area=float(a.get('area', w * h))))
            if boxes or keep_empty:
                samples.append(Sample(filename, boxes, imgsize))
                self.image_ids[img['file_name']] = img['id']
        return samples

    def load_trainval_data(self, data_dir, valid_fraction, require_image=True):
        """train = train2017, valid = val2017 (valid_fraction only says whether validation samples are required)"""
        self.train_samples = self._sample_list(data_dir, 'train2017', True, require_image)
        if not self.train_samples:
            raise RuntimeError('No training samples found in ' + data_dir)
        if valid_fraction > 0 or os.path.exists(self._annotation_file(data_dir, 'val2017')):
            self.valid_samples = self._sample_list(data_dir, 'val2017', False, require_image)
        else:
            self.valid_samples = []      # (no validation wanted and no file: the training set alone; a broken file is still an error)
        if valid_fraction > 0 and not self.valid_samples:
            raise RuntimeError('No validation samples found in ' + data_dir)
        self.num_train, self.num_valid = len(self.train_samples), len(self.valid_samples)

    def load_test_data(self, data_dir, require_image=True):
        self.test_samples = self._sample_list(data_dir, 'val2017', False, require_image, keep_empty=True)
        if not self.test_samples:
            raise RuntimeError('No testing samples found in ' + data_dir)
        self.num_test = len(self.test_samples)


def get_source():
    return COCOSource()
