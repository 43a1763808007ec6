"""CPU: the tiled DetectionOutput entry points are exported with the signatures include/ssdvgg_hip.h declares,
ssd_detout_tiles_ws_bytes follows the formula the header documents, and every limit is refused on the host, before the first HIP
call, with a message that names the entry point."""
import ctypes as C

import pytest

from test_detection_output_abi import prototypes, ctype_of, align256
from ssd_tensorflow_amd import _lib, tiling
from ssd_tensorflow_amd._lib import lib, last_error

NEW = ['ssd_detout_tiles_ws_bytes', 'ssd_detout_tiles_add_dev', 'ssd_detout_tiles_merge_dev', 'ssd_detout_tiles']


@pytest.mark.parametrize('name', NEW)
def test_symbol_and_signature(name):
    protos = prototypes()
    assert name in protos, name + ' is not declared in include/ssdvgg_hip.h'
    assert hasattr(lib, name), name + ' is not exported'
    ret, args = protos[name]
    res, argtypes = _lib.SIGNATURES[name]
    assert res is {'int': _lib.i32, 'size_t': _lib.sz}[ret]
    assert len(argtypes) == len(args), (args, argtypes)
    for decl, t in zip(args, argtypes):
        assert t is ctype_of(decl.replace('const ssd_tile*', 'const void*')), (name, decl, t)


def ws_formula(n_tiles, n_images, C_, k):
    def lists(n):
        return align256(4 * n) + align256(8 * n * k) + align256(16 * n * k)
    return align256(4 * (8 * n_tiles + n_images + 1)) + lists(n_tiles * C_) + lists(n_images * C_)


@pytest.mark.parametrize('pname', ['vgg300', 'vgg512'])
@pytest.mark.parametrize('ncls,nt,ni,k', [(1, 1, 1, 1), (20, 7, 1, 400), (80, 160, 8, 400), (127, 4096, 16, 1024), (3, 10, 10, 7)])
def test_ws_bytes_formula(pname, ncls, nt, ni, k):
    want = ws_formula(nt, ni, ncls, k)
    assert lib.ssd_detout_tiles_ws_bytes(pname.encode(), ncls, nt, ni, k) == want
    assert want <= 32 * (nt + ni) * ncls * k + 40 * nt + 4096                   # O((n_tiles + n_images) C nms_top_k)


def test_ws_bytes_of_the_documented_setting():
    assert 128e6 < lib.ssd_detout_tiles_ws_bytes(b'vgg300', 80, 160, 8, 400) < 131e6


@pytest.mark.parametrize('args', [(b'vgg999', 3, 1, 1, 400), (b'vgg300', 0, 1, 1, 400), (b'vgg300', 128, 1, 1, 400), (b'vgg300', 3, 0, 1, 400),
                                  (b'vgg300', 3, 4097, 1, 400), (b'vgg300', 3, 1, 0, 400), (b'vgg300', 3, 1, 2, 400), (b'vgg300', 3, 1, 1, 0),
                                  (b'vgg300', 3, 1, 1, 1025), (None, 3, 1, 1, 400)])
def test_ws_bytes_is_zero_on_bad_arguments(args):
    assert lib.ssd_detout_tiles_ws_bytes(*args) == 0
    assert last_error()


def _tiles(n=2, image=None, **kw):
    out = []
    for i in range(n):
        t = dict(x0=100 * i, y0=0, w=100, h=100, interior=0, W=100 * n, H=100, image=0 if image is None else image[i])
        t.update(kw.get('t%d' % i, {}))
        out.append((t['image'], tiling.Tile(t['x0'], t['y0'], t['w'], t['h'], t['interior']), (t['W'], t['H'])))
    return out


Z = (C.c_int * 64)()
P = C.addressof(Z)          # never dereferenced: every call below is refused first


def _add(tiles, ncls=3, first=0, b=None, thr=0.01, k=400, ws_bytes=1 << 40, pname=b'vgg300', n_tiles=None):
    n = len(tiles) if n_tiles is None else n_tiles
    return lib.ssd_detout_tiles_add_dev(pname, ncls, P, P, C.cast(tiling.tile_structs(tiles), C.c_void_p), n, first,
                                        len(tiles) if b is None else b, thr, k, 2, P, ws_bytes, None)


def _merge(tiles, ncls=3, n_images=None, k=400, keep=200, out_cap=200, ws_bytes=1 << 40):
    ni = (max(t[0] for t in tiles) + 1) if n_images is None else n_images
    return lib.ssd_detout_tiles_merge_dev(ncls, C.cast(tiling.tile_structs(tiles), C.c_void_p), len(tiles), ni, k, keep, out_cap, P, P, P, P, P, P,
                                          P, ws_bytes, None)


def _host(tiles, ncls=3, n_images=None, thr=0.01, k=400, keep=200, out_cap=200):
    ni = (max(t[0] for t in tiles) + 1) if n_images is None else n_images
    return lib.ssd_detout_tiles(b'vgg300', ncls, 0, P, C.cast(tiling.tile_structs(tiles), C.c_void_p), len(tiles), ni, thr, k, keep, 2, out_cap,
                                P, P, P, P, P, P)


BAD_TABLES = [
    (_tiles(2, image=[1, 0]), 'ascend'), (_tiles(3, image=[0, 2, 2]), 'ascend'), (_tiles(2, image=[1, 1]), 'ascend'),
    (_tiles(257), 'at most 256'), (_tiles(2, t1=dict(x0=150)), 'leaves'), (_tiles(2, t0=dict(w=0)), 'leaves'),
    (_tiles(2, t1=dict(W=300)), 'disagree'), (_tiles(2, t0=dict(interior=16)), 'interior'), (_tiles(1, t0=dict(W=1000001, w=1000001)), 'outside'),
]


@pytest.mark.parametrize('k', range(len(BAD_TABLES)))
def test_tile_tables_are_refused_by_every_entry_point(k):
    tiles, word = BAD_TABLES[k]
    ni = tiles[-1][0] + 1
    for call, name in ((lambda: _add(tiles), 'ssd_detout_tiles_add_dev'), (lambda: _merge(tiles, n_images=ni), 'ssd_detout_tiles_merge_dev'),
                       (lambda: _host(tiles, n_images=ni), 'ssd_detout_tiles')):
        assert call() != 0
        assert last_error().startswith(name + ':') and word in last_error(), (name, word, last_error())


def test_scalar_limits_are_refused_before_a_launch():
    ok = _tiles(2)
    for kw, word in ((dict(ncls=0), 'num_classes'), (dict(ncls=128), 'num_classes'), (dict(k=0), 'nms_top_k'), (dict(k=1025), 'nms_top_k'),
                     (dict(thr=-0.5), 'threshold'), (dict(thr=float('nan')), 'threshold'), (dict(thr=float('inf')), 'threshold'),
                     (dict(first=-1), 'outside'), (dict(first=1, b=2), 'outside'), (dict(b=0), 'outside'), (dict(n_tiles=0), 'tile'),
                     (dict(n_tiles=4097), 'tiles'), (dict(ws_bytes=lib.ssd_detout_tiles_ws_bytes(b'vgg300', 3, 2, 1, 400) - 1), 'workspace')):
        assert _add(ok, **kw) != 0
        assert last_error().startswith('ssd_detout_tiles_add_dev:') and word in last_error(), (kw, last_error())
    assert _add(ok, pname=b'vgg999') != 0 and 'preset' in last_error()
    for kw, word in ((dict(ncls=128), 'num_classes'), (dict(k=1025), 'nms_top_k'), (dict(keep=0), 'keep_top_k'), (dict(keep=1025), 'keep_top_k'),
                     (dict(out_cap=0), 'out_cap'), (dict(n_images=2), 'ascend'), (dict(n_images=0), 'pictures'),
                     (dict(ws_bytes=lib.ssd_detout_tiles_ws_bytes(b'vgg300', 3, 2, 1, 400) - 1), 'workspace')):
        assert _merge(ok, **kw) != 0
        assert last_error().startswith('ssd_detout_tiles_merge_dev:') and word in last_error(), (kw, last_error())
    for kw, word in ((dict(ncls=0), 'num_classes'), (dict(k=0), 'nms_top_k'), (dict(keep=1025), 'keep_top_k'), (dict(thr=-1.0), 'threshold'),
                     (dict(out_cap=0), 'out_cap'), (dict(n_images=2), 'ascend')):
        assert _host(ok, **kw) != 0
        assert last_error().startswith('ssd_detout_tiles:') and word in last_error(), (kw, last_error())


def test_python_surface_refuses_on_the_host():
    import numpy as np
    from ssd_tensorflow_amd import ssdutils as su
    tl = _tiles(2)
    pred = np.zeros((2, 8732, 8), np.float32)
    p = su.get_preset_by_name('vgg300')
    with pytest.raises(ValueError, match='decode'):
        su.detect_tiles(pred, p, tl, 0.5, decode='best')
    with pytest.raises(ValueError, match='tile_cap'):
        su.detect_tiles(pred, p, tl, 0.5, tile_cap=50, decode='all')
    with pytest.raises(ValueError, match='max_out'):
        su.detect_tiles(pred, p, tl, 0.5, max_out=None, decode='all')
    with pytest.raises(ValueError, match='argmax'):
        su.merge_tile_lists(tl, *[np.zeros(1)] * 5, tile_cap=1, decode='all')
    with pytest.raises(ValueError, match='tile_cap'):
        tiling.TiledDetector(None, 400, tile_cap=50, decode='all')
    with pytest.raises(ValueError, match='max_out'):
        tiling.TiledDetector(None, 400, max_out=7, decode='all')
    with pytest.raises(ValueError, match='decode'):
        tiling.TiledDetector(None, 400, decode='every')
    assert tiling.TiledDetector(None, 400).decode == 'argmax'
    d = tiling.TiledDetector(None, 400, decode='all', nms_top_k=8, keep_top_k=5)
    assert (d.decode, d.nms_top_k, d.keep_top_k) == ('all', 8, 5)


@pytest.mark.parametrize('driver', ['infer', 'detect'])
def test_driver_flags(driver, capsys):
    import importlib
    mod = importlib.import_module('ssd_tensorflow_amd.' + driver)
    base = ['--name', 'nowhere'] if driver == 'infer' else ['--model', 'nowhere.npz', 'x.jpg']
    with pytest.raises(SystemExit) as e:
        mod.main(base + ['--tile-decode', 'all'])
    assert e.value.code == 2 and '--tile-decode all needs --tile' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        mod.main(base + ['--tile', '400', '--tile-decode', 'all', '--nms-top-k', '1025'])
    assert e.value.code == 2 and '--nms-top-k must be in 1..1024' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        mod.main(base + ['--tile', '400', '--tile-decode', 'every'])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:                                        # (the earlier refusal stands)
        mod.main(base + ['--tile', '400', '--decode', 'all'])
    assert e.value.code == 2 and '--decode all does not apply to --tile' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mod.main(['--help'])
    assert "names the untiled pass's decode" in ' '.join(capsys.readouterr().out.split())
