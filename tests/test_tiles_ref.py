"""CPU: tile planning (ssd_tensorflow_amd.tiling.plan_tiles) against the formulas and against tests/tiles_ref.py, and the
numpy merge yardstick itself: identity on a one-tile picture, and a planted scene where the cross-tile suppression and the
edge drop each remove records."""
import math

import numpy as np
import pytest

from oracle import boxes as ob
import tiles_ref as R
from ssd_tensorflow_amd import tiling


def _cases(n=60, seed=3):
    rng = np.random.default_rng(seed)
    out = [(1000, 700, 400, 0.25), (400, 400, 400, 0.25), (401, 399, 400, 0.0), (4000, 3000, 512, 0.25), (33, 2000, 32, 0.9),
           (1200, 1200, 400, 0.25), (700, 1000, 400, 0.25), (100, 90, 400, 0.5)]
    for _ in range(n):
        out.append((int(rng.integers(1, 1500)), int(rng.integers(1, 1500)), int(rng.integers(32, 600)), float(rng.integers(0, 91)) / 100))
    return out


def test_cover_and_inside():
    for w, h, tile, ov in _cases():
        for whole in (True, False):
            tiles = tiling.plan_tiles(w, h, tile, ov, whole)
            seen = np.zeros((h, w), bool)
            for t in tiles:
                assert t.x0 >= 0 and t.y0 >= 0 and t.w >= 1 and t.h >= 1 and t.x0 + t.w <= w and t.y0 + t.h <= h, (w, h, tile, ov, t)
                if not (len(tiles) > 1 and t is tiles[-1] and whole):
                    seen[t.y0:t.y0 + t.h, t.x0:t.x0 + t.w] = True
            assert seen.all(), (w, h, tile, ov)


def _count(n, tile, ov):
    if n <= tile:
        return 1
    return math.ceil((n - tile) / max(1, int(tile * (1 - ov)))) + 1


def test_count_order_interior_whole():
    for w, h, tile, ov in _cases():
        kx, ky = _count(w, tile, ov), _count(h, tile, ov)
        windows = tiling.plan_tiles(w, h, tile, ov, whole=False)
        assert len(windows) == kx * ky
        assert [(t.y0, t.x0) for t in windows] == sorted((t.y0, t.x0) for t in windows)         # row-major, y outer
        assert len({(t.x0, t.y0) for t in windows}) == len(windows)
        for t in windows:
            assert t.w == min(tile, w) and t.h == min(tile, h)                                  # shifted back, never clipped
            assert t.interior == (1 * (t.x0 > 0) | 2 * (t.x0 + t.w < w) | 4 * (t.y0 > 0) | 8 * (t.y0 + t.h < h))
        assert windows[-1].x0 + windows[-1].w == w and windows[-1].y0 + windows[-1].h == h
        with_whole = tiling.plan_tiles(w, h, tile, ov, whole=True)
        if kx * ky > 1:
            assert with_whole[:-1] == windows and with_whole[-1] == tiling.Tile(0, 0, w, h, 0)
        else:
            assert with_whole == windows == [tiling.Tile(0, 0, w, h, 0)]                        # a single window: the whole picture


def test_plan_matches_ref():
    for w, h, tile, ov in _cases():
        for whole in (True, False):
            assert [tuple(t) for t in tiling.plan_tiles(w, h, tile, ov, whole)] == R.plan_tiles_ref(w, h, tile, ov, whole)
    assert [tuple(t) for t in tiling.plan_tiles(1000, 700, 400)] == R.plan_tiles_ref(1000, 700, 400, 0.25, True)
    assert len(tiling.plan_tiles(1000, 700, 400)) == 7 and len(tiling.plan_tiles(300, 300, 400)) == 1


@pytest.mark.parametrize('tile, ov', [(31, 0.25), (0, 0.25), (400, -0.01), (400, 0.91), (400, 1.0)])
def test_value_errors(tile, ov):
    with pytest.raises(ValueError):
        tiling.plan_tiles(1000, 700, tile, ov)
    with pytest.raises(ValueError):
        R.plan_tiles_ref(1000, 700, tile, ov)


@pytest.fixture(scope='module')
def scene():
    return R.planted_scene()


def test_one_tile_is_detect(scene):
    pred, tiles, anch = scene
    for t in (0, 4, len(tiles) - 1):
        for thr, cap, mo in ((0.3, 200, None), (0.01, 50, 5), (0.3, 1, 200)):
            want = ob.detect(pred[t], anch, thr, cap, mo)
            got = R.merge_ref([ob.decode(pred[t], anch, thr, cap)], [(0, 0, 640, 480, 0)], (640, 480), edge_margin=2, max_out=mo)
            assert len(want['idx']) > 0
            for k in ('idx', 'cls', 'conf', 'box'):
                assert np.array_equal(got[k], want[k]), (t, thr, cap, mo, k)
            assert not got['tile'].any()


def test_planted_scene_suppression_and_edge_drop(scene):
    pred, tiles, anch = scene
    W, H = 1000, 700
    dets = R.decode_tiles(pred, anch, 0.3, 200)
    per_tile = sum(len(ob.suppress(d)) for d in dets)
    keep_all = R.candidates_ref(dets, tiles, (W, H), edge_margin=-1)
    dropped = R.candidates_ref(dets, tiles, (W, H), edge_margin=2)
    merged_all = R.merge_ref(dets, tiles, (W, H), edge_margin=-1)
    merged = R.merge_ref(dets, tiles, (W, H), edge_margin=2)
    print('candidates', len(keep_all['idx']), '->', len(merged_all['idx']), 'survivors; with the edge drop', len(dropped['idx']), '->',
          len(merged['idx']), '; per-tile NMS survivors', per_tile)
    assert len(keep_all['idx']) == sum(len(d['idx']) for d in dets)
    assert len(merged_all['idx']) < per_tile                     # the cross-tile NMS removes what per-tile NMS cannot see
    assert len(dropped['idx']) < len(keep_all['idx'])            # the edge drop removes records
    assert 0 < len(merged['idx']) <= len(merged_all['idx'])
    # ties exist, within and across tiles
    c = keep_all['conf']
    assert (c[1:] == c[:-1]).any() and ((c[1:] == c[:-1]) & (keep_all['tile'][1:] != keep_all['tile'][:-1])).any()
    # the order of the union: confidence descending, ties by tile, then anchor
    key = list(zip(-keep_all['conf'].astype(np.float64), keep_all['tile'], keep_all['idx']))
    assert key == sorted(key)
    # every mapped box lies on the picture's grid
    assert keep_all['box'].min() >= 0 and keep_all['box'].max() <= 999
