"""CPU: the COCO data source on a tiny annotation tree written into tmp_path, the crowd / area attributes of FlaggedBox, and
TrainingData on top of the source."""
import json
import os
import pickle

import pytest

from ssd_tensorflow_amd import transforms as T
from ssd_tensorflow_amd.source_coco import COCOSource, get_source
from ssd_tensorflow_amd.utils import Box, FlaggedBox, Point, Size, Sample, abs2prop, box_like, default_colors, load_data_source, prop2abs

CATEGORIES = [dict(id=90, name='toothbrush'), dict(id=1, name='person'), dict(id=3, name='car')]      # (not in id order)
IMAGES = [dict(id=11, file_name='a.jpg', width=640, height=480), dict(id=7, file_name='b.jpg', width=500, height=375),
          dict(id=42, file_name='none.jpg', width=640, height=427),          # no annotation
          dict(id=5, file_name='crowd.jpg', width=320, height=240),          # only a crowd region
          dict(id=19, file_name='grey.jpg', width=200, height=100)]          # a greyscale file
ANNOTATIONS = [
    dict(id=1, image_id=11, category_id=3, bbox=[10.5, 20.25, 100.0, 50.5], area=2000.75, iscrowd=0),
    dict(id=2, image_id=11, category_id=90, bbox=[300.0, 100.0, 0.0, 40.0], area=0.0, iscrowd=0),      # zero width
    dict(id=3, image_id=11, category_id=1, bbox=[0.0, 0.0, 640.0, 480.0], area=150000.0, iscrowd=1),
    dict(id=4, image_id=7, category_id=1, bbox=[50.0, 60.0, 70.0, 80.0], area=4100.5, iscrowd=0),
    dict(id=5, image_id=5, category_id=1, bbox=[5.0, 5.0, 200.0, 100.0], area=9000.0, iscrowd=1),
    dict(id=6, image_id=19, category_id=90, bbox=[20.0, 10.0, 60.0, 30.0], area=1500.0, iscrowd=0),
]


@pytest.fixture
def tree(tmp_path):
    from PIL import Image
    os.makedirs(tmp_path / 'annotations')
    for split in ('train2017', 'val2017'):
        os.makedirs(tmp_path / split)
        with open(tmp_path / 'annotations' / ('instances_%s.json' % split), 'w') as f:
            json.dump(dict(images=IMAGES, annotations=ANNOTATIONS, categories=CATEGORIES), f)
        for img in IMAGES:
            mode = 'L' if img['file_name'] == 'grey.jpg' else 'RGB'
            Image.new(mode, (img['width'], img['height']), 100 if mode == 'L' else (10, 100, 200)).save(tmp_path / split / img['file_name'])
    return str(tmp_path)


def names(samples):
    return [os.path.basename(s.filename) for s in samples]


def test_class_mapping_and_ids(tree):
    src = get_source()
    assert isinstance(src, COCOSource) and isinstance(load_data_source('coco'), COCOSource)
    src.load_trainval_data(tree, 0.1)
    assert src.num_classes == 3 and src.lid2name == {0: 'person', 1: 'car', 2: 'toothbrush'}
    assert src.lname2id == {'person': 0, 'car': 1, 'toothbrush': 2} and src.category_ids == {0: 1, 1: 3, 2: 90}
    assert src.colors == default_colors(['person', 'car', 'toothbrush'])
    assert src.image_ids['a.jpg'] == 11 and src.image_ids['grey.jpg'] == 19 and src.image_ids['crowd.jpg'] == 5
    assert (src.num_train, src.num_valid) == (len(src.train_samples), len(src.valid_samples)) == (3, 4)


def test_train_rules(tree):
    src = get_source()
    src.load_trainval_data(tree, 0.1)
    assert names(src.train_samples) == ['a.jpg', 'b.jpg', 'grey.jpg']              # none.jpg and crowd.jpg are left without boxes
    a = src.train_samples[0]
    assert a.imgsize == Size(640, 480) and a.filename == os.path.join(tree, 'train2017', 'a.jpg')
    assert len(a.boxes) == 1 and type(a.boxes[0]) is Box                           # the zero-width box and the crowd region are gone
    assert a.boxes[0] == Box('car', 1, *abs2prop(10.5, 110.5, 20.25, 70.75, Size(640, 480)))
    assert a.boxes[0].center == Point(60.5 / 640, 45.5 / 480) and a.boxes[0].size == Size(100.0 / 640, 50.5 / 480)
    assert all(type(b) is Box for s in src.train_samples for b in s.boxes)


def test_valid_rules_flags_and_areas(tree):
    src = get_source()
    src.load_trainval_data(tree, 0.1)
    assert names(src.valid_samples) == ['a.jpg', 'b.jpg', 'crowd.jpg', 'grey.jpg']
    a = src.valid_samples[0]
    assert [b.label for b in a.boxes] == ['car', 'toothbrush', 'person'] and all(type(b) is FlaggedBox for b in a.boxes)
    assert [(b.crowd, b.difficult, b.area) for b in a.boxes] == [(False, False, 2000.75), (False, False, 0.0), (True, True, 150000.0)]
    assert a.boxes[1].size.w == 0.0                                               # the zero-width box stays in the validation set
    only = src.valid_samples[2].boxes
    assert len(only) == 1 and only[0].crowd and only[0].area == 9000.0 and only[0].labelid == 0
    assert src.valid_samples[1].boxes[0].area == 4100.5 != 70.0 * 80.0            # the annotation's area, not the box's
    # pickling keeps the attributes
    back = pickle.loads(pickle.dumps(src.valid_samples))
    assert back == src.valid_samples
    assert [(b.crowd, b.difficult, b.area) for s in back for b in s.boxes] == [(b.crowd, b.difficult, b.area) for s in src.valid_samples for b in s.boxes]
    assert repr(a.boxes[2]).endswith(', difficult=True, crowd=True, area=150000.0)') and repr(a.boxes[0]).endswith(', difficult=False, area=2000.75)')


def test_test_data_keeps_images_without_annotations(tree):
    src = get_source()
    src.load_test_data(tree)
    assert names(src.test_samples) == ['a.jpg', 'b.jpg', 'none.jpg', 'crowd.jpg', 'grey.jpg'] and src.num_test == 5
    assert src.test_samples[2].boxes == [] and src.image_ids['none.jpg'] == 42
    os.remove(os.path.join(tree, 'val2017', 'b.jpg'))
    src2 = get_source()
    src2.load_test_data(tree)
    assert 'b.jpg' not in names(src2.test_samples) and src2.num_test == 4
    src2.load_test_data(tree, require_image=False)
    assert src2.num_test == 5


def test_box_like_and_a_transform_keep_the_attributes(tree):
    src = get_source()
    src.load_trainval_data(tree, 0.1)
    crowd = src.valid_samples[0].boxes[2]
    moved = box_like(crowd, Point(0.4, 0.4), Size(0.2, 0.2))
    assert type(moved) is FlaggedBox and (moved.crowd, moved.difficult, moved.area) == (True, True, 150000.0) and moved.size == Size(0.2, 0.2)
    plain = box_like(src.valid_samples[0].boxes[0], Point(0.4, 0.4), Size(0.2, 0.2))
    assert type(plain) is FlaggedBox and (plain.crowd, plain.difficult, plain.area) == (False, False, 2000.75)
    assert type(box_like(Box('x', 0, Point(0.1, 0.1), Size(0.1, 0.1)), Point(0.4, 0.4), Size(0.2, 0.2))) is Box
    gt = T.transform_gt(src.valid_samples[1], Size(600, 475), 50, 100)           # an expand: the picture at (100, 50) of a larger canvas
    assert len(gt.boxes) == 1 and gt.boxes[0].area == 4100.5 and not gt.boxes[0].crowd and gt.imgsize == Size(600, 475)
    assert prop2abs(gt.boxes[0].center, gt.boxes[0].size, gt.imgsize) == (150, 220, 110, 190)
    r = crowd._replace(center=Point(0.5, 0.5))
    assert (r.crowd, r.area, r.center) == (True, 150000.0, Point(0.5, 0.5)) and crowd._replace(area=None).area is None


def test_training_data_builds_its_sample_lists(tree):
    from ssd_tensorflow_amd.training_data import TrainingData
    td = TrainingData(tree, 'vgg300', data_source='coco', device_tensors=False)
    assert td.num_classes == 3 and td.lid2name == {0: 'person', 1: 'car', 2: 'toothbrush'}
    assert (td.num_train, td.num_valid) == (3, 4) and names(td.train_samples) == ['a.jpg', 'b.jpg', 'grey.jpg']
    assert names(td.valid_samples) == ['a.jpg', 'b.jpg', 'crowd.jpg', 'grey.jpg'] and td.valid_samples[2].boxes[0].crowd
    assert set(td.label_colors) == {'person', 'car', 'toothbrush'}


def test_missing_annotation_file(tree, tmp_path):
    os.remove(os.path.join(tree, 'annotations', 'instances_val2017.json'))
    src = get_source()
    with pytest.raises(RuntimeError, match=r'No COCO annotation file .*instances_val2017\.json'):
        src.load_test_data(tree)
    with pytest.raises(RuntimeError, match=r'No COCO annotation file .*instances_val2017\.json'):
        src.load_trainval_data(tree, 0.1)
    src.load_trainval_data(tree, 0)                                               # no validation wanted: the training set alone
    assert src.num_train == 3 and src.num_valid == 0
    with pytest.raises(RuntimeError, match=r'No COCO annotation file .*instances_train2017\.json'):
        get_source().load_trainval_data(str(tmp_path / 'nowhere'), 0)
    with open(os.path.join(tree, 'annotations', 'instances_val2017.json'), 'w') as f:
        json.dump(dict(images=[]), f)
    with pytest.raises(RuntimeError, match='not an instances file'):
        get_source().load_test_data(tree)
    with pytest.raises(RuntimeError, match='not an instances file'):          # a broken file is an error also where no validation is wanted
        get_source().load_trainval_data(tree, 0)


def test_result_records_keep_the_files_ids(tree):
    """infer.py --coco-results: image_id / category_id of the annotation file, bbox [x, y, w, h] in pixels from the 1000-grid box"""
    from ssd_tensorflow_amd.infer import coco_result_records
    src = get_source()
    src.load_test_data(tree)
    grey = src.test_samples[4]                                                   # 200 x 100
    det = Box('toothbrush', 2, *abs2prop(100, 400, 100, 400, Size(1000, 1000)))
    rec = coco_result_records(src, grey, [(0.75, det), (0.5, det._replace(label='person', labelid=0))])
    assert rec == [dict(image_id=19, category_id=90, bbox=[20.0, 10.0, 60.0, 30.0], score=0.75),
                   dict(image_id=19, category_id=1, bbox=[20.0, 10.0, 60.0, 30.0], score=0.5)]
    assert json.loads(json.dumps(rec)) == rec


def test_result_records_with_a_directory_in_file_name(tmp_path):
    from ssd_tensorflow_amd.infer import coco_image_id, coco_result_records
    os.makedirs(tmp_path / 'annotations')
    images = [dict(id=3, file_name='sub/x.jpg', width=100, height=50), dict(id=4, file_name='other/x.jpg', width=100, height=50)]
    with open(tmp_path / 'annotations' / 'instances_val2017.json', 'w') as f:
        json.dump(dict(images=images, annotations=[], categories=CATEGORIES), f)
    src = get_source()
    src.load_test_data(str(tmp_path), require_image=False)
    assert src.image_ids == {'sub/x.jpg': 3, 'other/x.jpg': 4}
    assert [coco_image_id(src, s.filename) for s in src.test_samples] == [3, 4]
    det = Box('car', 1, *abs2prop(0, 500, 0, 1000, Size(1000, 1000)))
    assert coco_result_records(src, src.test_samples[1], [(0.25, det)]) == [dict(image_id=4, category_id=3, bbox=[0.0, 0.0, 50.0, 50.0], score=0.25)]
    with pytest.raises(RuntimeError, match='no image id'):
        coco_image_id(src, str(tmp_path / 'val2017' / 'y.jpg'))


def test_old_style_flagged_box_is_unchanged():
    c, s = Point(0.5, 0.25), Size(0.2, 0.1)
    old = FlaggedBox('dog', 11, c, s, True)
    assert old == Box('dog', 11, c, s) and hash(old) == hash(Box('dog', 11, c, s)) and tuple(old) == ('dog', 11, c, s)
    assert repr(old) == "FlaggedBox(label='dog', labelid=11, center=Point(x=0.5, y=0.25), size=Size(w=0.2, h=0.1), difficult=True)"
    assert repr(FlaggedBox('dog', 11, c, s)) == "FlaggedBox(label='dog', labelid=11, center=Point(x=0.5, y=0.25), size=Size(w=0.2, h=0.1), difficult=False)"
    assert old.difficult is True and old.crowd is False and old.area is None
    assert old.__reduce__() == (FlaggedBox, ('dog', 11, c, s, True))
    back = pickle.loads(pickle.dumps(old))
    assert type(back) is FlaggedBox and back == old and back.difficult and not back.crowd and back.area is None
    moved = box_like(old, c, s)
    assert type(moved) is FlaggedBox and moved.difficult and repr(moved) == repr(old)
    assert old._replace(labelid=3).difficult and old._replace(labelid=3).labelid == 3 and not old._replace(difficult=False).difficult
    crowd = FlaggedBox('dog', 11, c, s, crowd=True, area=12.5)
    assert crowd.difficult and crowd == old and pickle.loads(pickle.dumps(crowd)).area == 12.5 and pickle.loads(pickle.dumps(crowd)).crowd
    with pytest.raises(TypeError):
        FlaggedBox('dog', 11, c, s, True, True)                                  # crowd and area are keyword attributes
