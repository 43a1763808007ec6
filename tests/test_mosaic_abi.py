"""CPU: the cells entry of the augmentation in the C ABI (ssd_augment_cells_dev / ssd_augment_cells_ws_bytes):
declared, exported and given ctypes signatures; the ctypes mirror of ssd_augment_cell; and every refusal of the contract -- cells
that overlap, a gap, a cell outside its sample, 17 cells in a sample, an INTER_AREA cell that shrinks 15x, a sample without
cells -- returns non-zero with a text before any device work (the device pointers here are addresses that are never
dereferenced and no GPU is needed).  NO call in this file may pass validation: a case that has to get past one check is made
to fail a later one on purpose, and the assertion names that check's text."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20          # a "device pointer": every call below is refused before it could be used
W, H = 96, 80


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_symbols_declared_exported_and_signed():
    from ssd_tensorflow_amd import _lib
    code = re.sub(r'/\*.*?\*/', '', _read('include', 'ssdvgg_hip.h'), flags=re.S)
    assert re.search(r'typedef\s+struct\s*\{\s*int\s+sample\s*;\s*int\s+x0\s*,\s*y0\s*,\s*w\s*,\s*h\s*;\s*\}\s*ssd_augment_cell\s*;', code)
    assert re.search(r'size_t\s+ssd_augment_cells_ws_bytes\s*\(\s*int\s+n_cells\s*,\s*int\s+out_w\s*,\s*int\s+out_h\s*\)', code)
    assert re.search(r'int\s+ssd_augment_cells_dev\s*\(\s*const\s+unsigned\s+char\s*\*\s*images_dev\s*,\s*const\s+ssd_augment_params\s*\*\s*params\s*,'
                     r'\s*const\s+ssd_augment_cell\s*\*\s*cells\s*,\s*int\s+n_cells\s*,\s*int\s+b\s*,\s*int\s+out_w\s*,\s*int\s+out_h\s*,'
                     r'\s*float\s*\*\s*out_dev\s*,\s*void\s*\*\s*ws_dev\s*,\s*void\s*\*\s*stream\s*\)', code)
    for n in ('ssd_augment_cells_ws_bytes', 'ssd_augment_cells_dev'):
        assert hasattr(_lib.lib, n), f'{n} is not exported'
        assert n in _lib.SIGNATURES, f'{n} has no ctypes signature'
    res, args = _lib.SIGNATURES['ssd_augment_cells_dev']
    assert res is C.c_int and len(args) == 10 and all(a is C.c_int for a in args[3:7])
    assert _lib.SIGNATURES['ssd_augment_cells_ws_bytes'] == (C.c_size_t, [C.c_int] * 3)
    # the sibling entry stays as it was
    assert _lib.SIGNATURES['ssd_augment_batch_dev'][0] is C.c_int and len(_lib.SIGNATURES['ssd_augment_batch_dev'][1]) == 8


def test_the_ctypes_mirror_of_the_cell():
    from ssd_tensorflow_amd import transforms as T
    assert [n for n, _ in T._Cell._fields_] == ['sample', 'x0', 'y0', 'w', 'h']
    assert all(t is C.c_int for _, t in T._Cell._fields_) and C.sizeof(T._Cell) == 20
    arr, back = T.cells_array([(0, 0, 0, 5, 7), (1, 2, 3, 4, 6)])
    assert back.dtype == np.int32 and back.shape == (2, 5) and len(arr) == 2
    assert (arr[1].sample, arr[1].x0, arr[1].y0, arr[1].w, arr[1].h) == (1, 2, 3, 4, 6)
    assert C.addressof(arr) == back.ctypes.data          # the rows of the int32 array ARE the structs


def test_workspace_grows_with_the_cells_and_holds_the_siblings():
    from ssd_tensorflow_amd._lib import lib
    one = lib.ssd_augment_cells_ws_bytes(32, 300, 300)
    four = lib.ssd_augment_cells_ws_bytes(128, 300, 300)
    assert one >= lib.ssd_augment_ws_bytes(32, 300, 300) + 32 * 20
    assert four >= lib.ssd_augment_ws_bytes(128, 300, 300) + 128 * 20 and four > one
    assert lib.ssd_augment_cells_ws_bytes(0, 300, 300) == 0


def _params(n, src=(150, 110), alg=1, crop=None, crop_x0=0):
    from ssd_tensorflow_amd import transforms as T
    arr = (T._Params * n)()
    for q in arr:
        q.src_w, q.src_h = src
        cw, ch = crop or src
        q.crop_w, q.crop_h = cw, ch
        q.crop_x0 = crop_x0
        q.reorder[0], q.reorder[1], q.reorder[2] = 0, 1, 2
        q.clip_x1, q.clip_y1 = src
        q.resize_alg = alg
        q.mean[0], q.mean[1], q.mean[2] = 104, 117, 123
    return arr


def _call(cells, b, params=None):
    from ssd_tensorflow_amd import transforms as T
    from ssd_tensorflow_amd._lib import lib, last_error
    carr, keep = T.cells_array(cells)
    params = params if params is not None else _params(len(cells))
    rc = lib.ssd_augment_cells_dev(FAKE, C.cast(params, C.c_void_p), C.cast(carr, C.c_void_p), len(cells), b, W, H, FAKE, FAKE, None)
    return rc, last_error()


def _quad(s, mx=48, my=40):
    return [(s, 0, 0, mx, my), (s, mx, 0, W - mx, my), (s, 0, my, mx, H - my), (s, mx, my, W - mx, H - my)]


def test_overlapping_cells_are_refused():
    cells = _quad(0)
    cells[1] = (0, 47, 0, W - 48, 40)                    # one column to the left: overlaps the top-left cell, same total area
    rc, text = _call(cells, 1)
    assert rc != 0 and 'overlap' in text and 'sample 0' in text


def test_a_gap_is_refused():
    cells = _quad(0)
    cells[3] = (0, 48, 40, W - 48, H - 41)               # the last row of the bottom-right cell is missing
    rc, text = _call(cells, 1)
    assert rc != 0 and 'gap' in text and str(W * H) in text
    rc, text = _call(_quad(0)[:3], 1)                    # a whole cell is missing
    assert rc != 0 and 'gap' in text


def test_a_cell_outside_its_sample_is_refused():
    for bad in [(0, 48, 40, W - 47, H - 40), (0, -1, 0, 49, 40), (0, 0, 41, 48, 40), (0, 0, 0, 0, 40), (0, 0, 0, 48, -3)]:
        cells = _quad(0)
        cells[0 if bad[1] <= 0 and bad[2] <= 0 else 3] = bad
        rc, text = _call(cells, 1)
        assert rc != 0 and ('outside' in text or 'empty' in text), (bad, text)
    rc, text = _call(_quad(0) + _quad(2), 2)             # a sample index past the batch
    assert rc != 0 and 'sample 2' in text


def test_seventeen_cells_in_one_sample_are_refused():
    cells = [(0, 0, y, W, 1) for y in range(16)] + [(0, 0, 16, W, H - 16)]          # 17 row strips that tile the sample
    assert sum(c[3] * c[4] for c in cells) == W * H
    rc, text = _call(cells, 1)
    assert rc != 0 and '16' in text and 'cells' in text
    # the limit is per SAMPLE: 17 strips in sample 0 and a quad in sample 1 are 21 cells for 2 samples, inside 16 x b
    rc, text = _call(cells + _quad(1), 2)
    assert rc != 0 and 'sample 0 has more than 16 cells' in text
    cells = [(0, 0, y, W, 1) for y in range(15)] + [(0, 0, 15, W, H - 15)]          # 16 are a sample's limit, not past it
    rc, text = _call(cells + _quad(1)[:3], 2)
    assert rc != 0 and 'gap' in text and 'sample 1' in text                          # (refused for the OTHER sample's gap)


def test_an_inter_area_cell_that_shrinks_15x_is_refused():
    # 150 x 110 into a 10-pixel wide cell: 15x along x; INTER_AREA's tap table ends at 14x
    cells = _quad(0, mx=10)
    rc, text = _call(cells, 1, _params(4, alg=3))
    assert rc != 0 and 'INTER_AREA' in text and '14' in text
    # 14x is inside the limit: the call gets past this check and is refused by the next one, on purpose -- a 140-pixel crop
    # that starts at column 20 of the 150-pixel frame
    rc, text = _call(cells, 1, _params(4, alg=3, crop=(140, 110), crop_x0=20))
    assert rc != 0 and 'crop window outside the frame' in text and 'INTER_AREA' not in text
    # the same picture as a whole sample is fine for the limit: it is the CELL's size that counts
    rc, text = _call([(0, 0, 0, W, H)] + _quad(1)[:3], 2, _params(4, alg=3))
    assert rc != 0 and 'gap' in text


def test_a_sample_without_cells_and_an_empty_call_are_refused():
    rc, text = _call(_quad(0) + _quad(2), 3)
    assert rc != 0 and 'sample 1' in text and 'no cell' in text
    from ssd_tensorflow_amd._lib import lib, last_error
    assert lib.ssd_augment_cells_dev(FAKE, FAKE, FAKE, 0, 1, W, H, FAKE, FAKE, None) != 0 and 'no cells' in last_error()
    assert lib.ssd_augment_cells_dev(None, None, None, 4, 1, W, H, None, None, None) != 0 and last_error() == 'null argument'


def test_the_per_struct_checks_apply_to_every_cell():
    p = _params(4)
    p[2].resize_alg = 7
    rc, text = _call(_quad(0), 1, p)
    assert rc != 0 and 'image 2' in text and 'resize algorithm' in text
    p = _params(4)
    p[3].crop_w = 151
    rc, text = _call(_quad(0), 1, p)
    assert rc != 0 and 'image 3' in text and 'crop window' in text


def test_python_names_and_defaults(capsys):
    from ssd_tensorflow_amd import train, transforms as T
    from ssd_tensorflow_amd.training_data import TrainingData
    p = inspect.signature(TrainingData.__init__).parameters
    assert p['mosaic'].default == 0.0 and p['mosaic_center'].default == (0.3, 0.7) and p['mosaic_off_epochs'].default == 0
    assert inspect.signature(T.plan_params).parameters['cells'].default is None
    assert callable(T.augment_cells) and callable(T.mosaic_layout) and callable(T.mosaic_draw) and callable(T.mosaic_box)
    with pytest.raises(SystemExit):
        train.main(['--help'])
    out = capsys.readouterr().out
    assert '--mosaic ' in out and '--mosaic-center LO HI' in out and '--mosaic-off-epochs' in out and 'DESIGN.md 39' in out


def test_mosaic_without_the_transform_path_is_a_loud_error(capsys):
    from ssd_tensorflow_amd import train
    assert train.main(['--mosaic', '0.5', '--epochs', '1', '--name', os.path.join(os.sep, 'nonexistent', 'run')]) == 1
    assert '--mosaic needs the transform path' in capsys.readouterr().out
