"""CPU: the host half of the JPEG decoder (csrc/jpeg.hip: marker parser + Huffman decoder) against
tests/golden/j1_jpeg.npz -- JPEG bytes and the pixels Pillow / libjpeg-turbo decodes them to (tools/make_jpeg_golden.py).
The back half (dequantise, IDCT, upsampling, colour) is the numpy oracle tests/jpeg_ref.py here; tests/test_gpu_jpeg.py runs
the kernels against the same pixels."""
import ctypes as C
import hashlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'j1_jpeg.npz')


@pytest.fixture(scope='module')
def g():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _list(g, kind):
    return [(str(n), g['%s_%d_jpg' % (kind, i)]) for i, n in enumerate(g['%s_names' % kind])]


def test_entropy_stage_plus_reference_back_half_equals_libjpeg(g):
    """1 (and 7: no supported file may fall back or be skipped): every byte of every supported file"""
    from ssd_tensorflow_amd import jpeg
    ok = _list(g, 'ok')
    assert len(ok) >= 40
    seen = set()
    for i, (name, data) in enumerate(ok):
        w, h, comps, sampling, st = jpeg.info(data)
        want = g['ok_%d_bgr' % i]
        assert st == jpeg.OK and (h, w) == want.shape[:2], name
        st, d, coef = jpeg.entropy_decode(data)
        assert st == jpeg.OK and 0 < d.max_l1 <= jpeg.MAX_L1, name
        assert coef.size * 2 == jpeg.lib.ssd_jpeg_coef_bytes(data.ctypes.data, data.size)
        got = jpeg_ref.decode_planes(coef, d)
        assert got.shape == want.shape and np.array_equal(got, want), '%s: %d bytes differ' % (name, int((got != want).sum()))
        seen.add((comps, sampling))
    assert seen == {(1, 0x11), (3, 0x11), (3, 0x21), (3, 0x22)}
    for name in g['voc_names']:
        st, d, coef = jpeg.entropy_decode(g['voc_%s_jpg' % name])
        assert st == jpeg.OK
        got = jpeg_ref.decode_planes(coef, d)
        assert got.shape[:2] == tuple(g['voc_%s_shape' % name])
        rows = got.astype(np.int64).sum(1)
        wrong = np.nonzero((rows != g['voc_%s_rowsums' % name]).any(1))[0]
        assert wrong.size == 0, '%s: rows %s differ' % (name, wrong[:8])
        assert hashlib.sha256(got.tobytes()).hexdigest() == str(g['voc_%s_sha256' % name])


def test_fixture_equals_a_live_pillow_decode(g):
    """2: a fixture that went stale with a libjpeg change shows here"""
    Image = pytest.importorskip('PIL.Image')
    for i, (name, data) in enumerate(_list(g, 'ok')):
        with Image.open(io.BytesIO(data.tobytes())) as im:
            assert np.array_equal(np.asarray(im.convert('RGB'))[:, :, ::-1], g['ok_%d_bgr' % i]), name
    for name in g['voc_names']:
        with Image.open(io.BytesIO(g['voc_%s_jpg' % name].tobytes())) as im:
            px = np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])
        assert hashlib.sha256(px.tobytes()).hexdigest() == str(g['voc_%s_sha256' % name])


def test_unsupported_files_get_the_status_and_no_error_text(g):
    """3"""
    from ssd_tensorflow_amd import jpeg, _lib
    names = [n for n, _ in _list(g, 'unsup')]
    assert names == ['progressive', 'cmyk', 'luma_1x2', 'luma_4x1', 'chroma_2x1', 'precision_12', 'arithmetic_sof9', 'adobe_transform_0']
    assert jpeg.info(g['ok_0_jpg'])[4] == jpeg.OK
    for name, data in _list(g, 'unsup'):
        _lib.lib.ssd_preset_info(b'nope', None, None, None, None)           # leaves an error text behind ...
        marker = _lib.last_error()
        assert marker
        assert jpeg.info(data)[4] == jpeg.UNSUPPORTED, name
        st, d, coef = jpeg.entropy_decode(data)
        assert st == jpeg.UNSUPPORTED and coef is None, name
        assert _lib.last_error() == marker, name                            # ... that these calls did not replace
    # the header decides: the patched files differ from a good file in the header only, so a scan cut short changes nothing
    data = g['unsup_2_jpg']
    assert jpeg.info(data[:len(data) * 2 // 3])[4] == jpeg.UNSUPPORTED


def test_corrupt_files_are_errors_with_a_message(g):
    """4, first half"""
    from ssd_tensorflow_amd import jpeg, _lib
    bad = _list(g, 'bad')
    assert [n for n, _ in bad] == ['truncated_10', 'truncated_50', 'truncated_99', 'dht_counts_past_256', 'sos_before_sof',
                                   'segment_length_past_end', 'stuffing_removed', 'restart_wrong_index']
    assert jpeg.entropy_decode(g['bad_source_jpg'])[0] == jpeg.OK           # they derive from a good file
    for name, data in bad:
        d, st = jpeg.Desc(), C.c_int(-1)
        coef = np.zeros(1 << 16, np.int16)
        rc = _lib.lib.ssd_jpeg_entropy_decode(data.ctypes.data, data.size, coef.ctypes.data, coef.nbytes, C.byref(d), st)
        assert rc != 0 and st.value == jpeg.ERROR and _lib.last_error().startswith('jpeg: '), name
        with pytest.raises(jpeg.JpegError, match='jpeg: '):
            jpeg.entropy_decode(data)
    with pytest.raises(jpeg.JpegError, match='no SOI'):
        jpeg.info(b'\x89PNG\r\n\x1a\n' + bytes(32))


_CHILD = r'''
import ctypes as C, mmap, sys
import numpy as np
lib = C.CDLL(sys.argv[1])
lib.ssd_last_error.restype = C.c_char_p
lib.ssd_jpeg_info.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 5
lib.ssd_jpeg_coef_bytes.restype = C.c_size_t
lib.ssd_jpeg_coef_bytes.argtypes = [C.c_void_p, C.c_size_t]
lib.ssd_jpeg_entropy_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
libc = C.CDLL(None, use_errno=True)
libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
PAGE = mmap.PAGESIZE
g = np.load(sys.argv[2])
good = g['bad_source_jpg'].tobytes()
cases = [(str(n), g['bad_%d_jpg' % i].tobytes(), 2) for i, n in enumerate(g['bad_names'])]
cases += [('cut_%d' % k, good[:k], None) for k in list(range(0, 700)) + list(range(700, len(good), 5))]       # any status, no fault
cases += [(str(n), g['unsup_%d_jpg' % i].tobytes(), 1) for i, n in enumerate(g['unsup_names'])]
cases += [('good', good, 0)]
pages = max(len(c[1]) for c in cases) // PAGE + 2
mm = mmap.mmap(-1, pages * PAGE)
base = C.addressof(C.c_char.from_buffer(mm))
assert libc.mprotect(base + (pages - 1) * PAGE, PAGE, 0) == 0, C.get_errno()      # PROT_NONE behind the input
end = (pages - 1) * PAGE
coef = np.zeros(1 << 18, np.int16)
desc = (C.c_char * 1024)()
w = [C.c_int() for _ in range(5)]
st = C.c_int()
for name, data, want in cases:
    n = len(data)
    mm[end - n:end] = data
    ptr = base + end - n
    lib.ssd_jpeg_info(ptr, n, *[C.byref(x) for x in w])
    lib.ssd_jpeg_coef_bytes(ptr, n)
    rc = lib.ssd_jpeg_entropy_decode(ptr, n, coef.ctypes.data, coef.nbytes, desc, C.byref(st))
    if want is not None:
        assert st.value == want and (rc != 0) == (want == 2), (name, rc, st.value)
        assert want != 2 or lib.ssd_last_error(), name
print('checked', len(cases))
'''


def test_corrupt_files_never_read_past_their_last_byte(g, tmp_path):
    """4, second half: each input ends at the last byte in front of an inaccessible page; the child (ctypes, numpy and the
    library only -- it never opens the GPU) must live through the corrupt list, every cut of the good file, the unsupported
    list and the good file itself."""
    script = tmp_path / 'child.py'
    script.write_text(_CHILD)
    lib_path = os.path.join(ROOT, 'ssd_tensorflow_amd', 'libssdvgg_hip.so')
    r = subprocess.run([sys.executable, str(script), lib_path, GOLDEN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, 'exit status %s\n%s' % (r.returncode, r.stderr[-3000:])
    assert r.stdout.startswith('checked ')


@pytest.mark.parametrize('threads', [1, 3, 8])
def test_batch_equals_one_by_one(g, threads):
    """5: supported, unsupported and corrupt files in one batch; a bad file spoils its own slot only"""
    from ssd_tensorflow_amd import jpeg
    ok, unsup, bad = _list(g, 'ok'), _list(g, 'unsup'), _list(g, 'bad')
    mixed = []
    for i in range(max(len(ok), len(unsup), len(bad))):
        mixed += [lst[i] for lst in (ok, bad, unsup) if i < len(lst)]
    datas = [d for _, d in mixed]
    coef, offs, descs, status, err = jpeg.entropy_decode_batch(datas, threads=threads)
    first_bad = next(i for i, (n, _) in enumerate(mixed) if n in dict(bad))
    assert err.startswith('file %d: jpeg: ' % first_bad)
    for i, (name, data) in enumerate(mixed):
        if name in dict(bad):
            assert status[i] == jpeg.ERROR, name
            continue
        st, d, c = jpeg.entropy_decode(data)
        assert status[i] == st, name
        if st != jpeg.OK:
            assert offs[i + 1] == offs[i]
            continue
        assert offs[i + 1] - offs[i] == c.nbytes and offs[i] % 16 == 0
        assert np.array_equal(coef[offs[i] // 2:offs[i + 1] // 2], c), name
        e = descs[i]
        assert (e.width, e.height, e.components, e.hs, e.vs, e.mcus_x, e.mcus_y, e.max_l1) == \
               (d.width, d.height, d.components, d.hs, d.vs, d.mcus_x, d.mcus_y, d.max_l1)
        assert [e.coef_off[k] - offs[i] // 2 for k in range(e.components)] == [d.coef_off[k] for k in range(d.components)]
        assert bytes(e.qt) == bytes(d.qt)


def test_range_guard_on_the_host(g):
    """8, host half: the block with L1 norm 15000 is accepted, the one with 15001 is reported unsupported"""
    from ssd_tensorflow_amd import jpeg
    st, d, coef = jpeg.entropy_decode(g['guard_inside_jpg'])
    assert st == jpeg.OK and d.max_l1 == jpeg.MAX_L1 == 15000 and np.array_equal(coef[:64], g['guard_inside_coefs'])
    st, d, coef = jpeg.entropy_decode(g['guard_beyond_jpg'])
    assert st == jpeg.UNSUPPORTED and d.max_l1 == 15001
    assert jpeg.info(g['guard_beyond_jpg'])[4] == jpeg.OK          # the header is fine; the scan decides
