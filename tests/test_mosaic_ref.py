"""CPU: the mosaic's host half against tests/mosaic_ref.py -- the layout of a centre tiles the sample, the box
mapping keeps a box's pixel rectangle, and the decision / partner / centre draws are a pure function of (seed, epoch, index)."""
import random

import numpy as np
import pytest

import mosaic_ref as mr
from ssd_tensorflow_amd import transforms as T
from ssd_tensorflow_amd.utils import Box, Point, Size, abs2prop, prop2abs

W, H = 96, 80
CENTRES = [(48, 40), (1, 1), (W - 1, H - 1), (37, 53), (1, H - 1), (W - 1, 1)]


@pytest.mark.parametrize('centre', CENTRES, ids=str)
def test_the_four_cells_of_a_centre_tile_the_sample(centre):
    cells = T.mosaic_layout(centre[0], centre[1], W, H)
    assert [tuple(c) for c in cells] == mr.layout(centre[0], centre[1], W, H)
    assert (mr.coverage(cells, W, H) == 1).all()
    assert sum(c[2] * c[3] for c in cells) == W * H
    # the order: top-left, top-right, bottom-left, bottom-right
    assert cells[0][:2] == (0, 0) and cells[1][1] == 0 and cells[2][0] == 0 and cells[3][:2] == tuple(centre)


@pytest.mark.parametrize('centre', [(0, 40), (48, 0), (W, 40), (48, H), (-1, 3)], ids=str)
def test_a_centre_that_leaves_a_cell_empty_is_refused(centre):
    with pytest.raises(ValueError, match='mosaic centre'):
        T.mosaic_layout(centre[0], centre[1], W, H)


def test_a_box_keeps_its_pixel_rectangle():
    """Rectangles whose bounds lie at half pixels of the cell (the truncation of prop2abs is then far from a rounding error):
    cell pixels + (x0, y0) = sample pixels, and the product's Python floats equal the float64 oracle."""
    rng = np.random.default_rng(5)
    for centre in CENTRES:
        for cell in mr.layout(centre[0], centre[1], W, H):
            x0, y0, cw, ch = cell
            for _ in range(20):
                xa, xb = sorted(rng.integers(0, cw + 1, 2)); ya, yb = sorted(rng.integers(0, ch + 1, 2))
                c, s = abs2prop(xa + 0.5, xb + 0.5, ya + 0.5, yb + 0.5, Size(cw, ch))
                box = Box('c', 1, c, s)
                in_cell = prop2abs(box.center, box.size, Size(cw, ch))
                assert in_cell == (xa, xb, ya, yb)
                m = T.mosaic_box(box, cell, W, H)
                assert m.label == 'c' and m.labelid == 1
                got = (m.center.x, m.center.y, m.size.w, m.size.h)
                want = mr.map_box((c.x, c.y, s.w, s.h), cell, W, H)
                assert got == tuple(float(v) for v in want)
                in_sample = prop2abs(m.center, m.size, Size(W, H))
                assert in_sample == (xa + x0, xb + x0, ya + y0, yb + y0)
                # and back: the sample's rectangle minus the cell's origin, proportional to the cell
                c2, s2 = abs2prop(in_sample[0] - x0 + 0.5, in_sample[1] - x0 + 0.5, in_sample[2] - y0 + 0.5, in_sample[3] - y0 + 0.5, Size(cw, ch))
                assert prop2abs(c2, s2, Size(cw, ch)) == in_cell


def test_the_draws_are_a_pure_function_of_their_arguments():
    seeds = [(1234 << 96) | (e << 32) | i for e in range(3) for i in range(40)]
    state = random.getstate()
    first = [T.mosaic_draw(s, 0.5, 100, 300, 300) for s in seeds]
    assert random.getstate() == state                     # a private generator: the module's stream is untouched
    random.seed(99); random.random()
    assert [T.mosaic_draw(s, 0.5, 100, 300, 300) for s in reversed(seeds)] == first[::-1]
    took = [d for d in first if d is not None]
    assert 30 < len(took) < 90                            # p = 0.5 of 120
    for partners, (mx, my) in took:
        assert len(partners) == 3 and all(0 <= p < 100 for p in partners)
        assert 90 <= mx <= 210 and 90 <= my <= 210        # round(0.3 * 300) .. round(0.7 * 300)
    assert len({tuple(d[0]) for d in took}) > len(took) // 2 and len({d[1] for d in took}) > len(took) // 2
    # the decision is the first draw: with p = 1 the same samples draw the same partners and centres, the others theirs
    every = [T.mosaic_draw(s, 1.0, 100, 300, 300) for s in seeds]
    assert all(e is not None for e in every)
    assert all(d == e for d, e in zip(first, every) if d is not None)
    assert all(T.mosaic_draw(s, 0.0, 100, 300, 300) is None for s in seeds)
    # the centre's range: whole pixels of [round(lo W), round(hi W)], ends included, never a cell without a pixel
    xs = {T.mosaic_draw(s, 1.0, 7, 10, 10, (0.3, 0.4))[1] for s in range(400)}
    assert {x for x, _ in xs} == {3, 4} and {y for _, y in xs} == {3, 4}
    edge = {T.mosaic_draw(s, 1.0, 7, 10, 10, (0.01, 0.99))[1] for s in range(400)}
    assert min(x for x, _ in edge) == 1 and max(x for x, _ in edge) == 9
    assert any(len(set(T.mosaic_draw(s, 1.0, 2, 10, 10)[0])) < 3 for s in range(20))      # partners may repeat


def test_recipe_sources_follow_seed_epoch_and_index():
    """_Recipe.sources: what the parent computes without running a transform; no function of the batch a sample arrives in,
    switched off for validation and in the last mosaic_off_epochs epochs."""
    from ssd_tensorflow_amd.training_data import TrainingData
    kw = dict(num_train=30, num_valid=6, augment=True, device_tensors=False)
    td = TrainingData(None, 'vgg300', mosaic=0.5, mosaic_off_epochs=2, epochs=5, **kw)
    other = TrainingData(None, 'vgg300', mosaic=0.5, seed=4321, **kw)
    try:
        r = td._recipes['train']
        whole = r.sources(1, list(range(30)))
        assert whole == [r.sources(1, [i])[0] for i in range(30)]
        assert whole[::-1] == r.sources(1, list(range(29, -1, -1)))
        assert all(s[0][0] == i and len(s[0]) in (1, 4) and (s[1] is None) == (len(s[0]) == 1) for i, s in enumerate(whole))
        assert 5 < sum(len(s[0]) == 4 for s in whole) < 25
        assert all(0 <= p < 30 for s in whole for p in s[0])
        assert whole != r.sources(2, list(range(30))) and whole != other._recipes['train'].sources(1, list(range(30)))
        for e in (3, 4):                                  # the last two of five epochs
            assert all(len(s[0]) == 1 for s in r.sources(e, list(range(30))))
        assert all(len(s[0]) == 1 for s in td._recipes['valid'].sources(1, list(range(6))))
    finally:
        td.close(); other.close()


def test_switches_are_checked():
    from ssd_tensorflow_amd.training_data import TrainingData
    with pytest.raises(ValueError, match='transform path'):
        TrainingData(None, 'vgg300', num_train=4, num_valid=2, mosaic=0.5)
    with pytest.raises(ValueError, match='probability'):
        TrainingData(None, 'vgg300', num_train=4, num_valid=2, augment=True, mosaic=1.5)
    with pytest.raises(ValueError, match='mosaic_center'):
        TrainingData(None, 'vgg300', num_train=4, num_valid=2, augment=True, mosaic=0.5, mosaic_center=(0.7, 0.3))
    with pytest.raises(ValueError, match='epochs'):
        TrainingData(None, 'vgg300', num_train=4, num_valid=2, augment=True, mosaic=0.5, mosaic_off_epochs=2)
