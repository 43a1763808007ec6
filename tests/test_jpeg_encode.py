"""CPU: the host half of the JPEG encoder (csrc/jpeg_enc.hip: Huffman coder + file framing) and the numpy oracle of
its device half (tests/jpeg_enc_ref.py) against tests/golden/j2_jpeg_encode.npz -- source pixels and the files Pillow /
libjpeg-turbo encodes them to (tools/make_jpeg_encode_golden.py).  tests/test_gpu_jpeg_encode.py runs the kernel against the
same oracle."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeg_enc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'j2_jpeg_encode.npz')


@pytest.fixture(scope='module')
def g():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def cases(g):
    """[(name, BGR pixels, quality, sampling, Pillow's file as a uint8 array)]"""
    return [(str(n), g['src_%d_bgr' % g['case_src'][i]], int(g['case_quality'][i]), str(g['case_sampling'][i]), g['case_%d_jpg' % i])
            for i, n in enumerate(g['case_names'])]


def same_desc(d, e):
    return ((d.width, d.height, d.components, d.hs, d.vs, d.mcus_x, d.mcus_y) == (e.width, e.height, e.components, e.hs, e.vs, e.mcus_x, e.mcus_y)
            and [int(v) for v in d.coef_off] == [int(v) for v in e.coef_off] and [list(t) for t in d.qt] == [list(t) for t in e.qt])


def scan(data):
    """the entropy-coded segment: the first byte behind the SOS header through EOI"""
    b = bytes(data)
    p = b.index(b'\xff\xda')
    return b[p + 2 + ((b[p + 2] << 8) | b[p + 3]):]


def test_fixture_covers_what_it_should(g):
    cs = cases(g)
    assert len(cs) >= 400
    assert {q for _, _, q, _, _ in cs} == {1, 30, 75, 95, 100} and {s for _, _, _, s, _ in cs} == {'4:4:4', '4:2:2', '4:2:0'}
    shapes = {px.shape[:2] for _, px, _, _, _ in cs}
    assert {h % 16 for h, _ in shapes} >= {0, 1, 8, 15} and {w % 16 for _, w in shapes} >= {0, 1, 8, 15}
    assert min(min(s) for s in shapes) == 1 and max(max(s) for s in shapes) >= 144
    assert {n.split('_')[0] for n in g['src_names']} == {'smooth', 'noise', 'edges', 'primaries'}
    assert str(g['pillow_version']) and str(g['libjpeg_turbo_version'])


def test_oracle_equals_libjpeg_block_for_block(g):
    """the oracle's coefficients and tables == what the entropy decoder reads from Pillow's file, padding blocks included: pins
    the arithmetic, the edge replication and the dummy-block rule against libjpeg-turbo itself"""
    from ssd_tensorflow_amd import jpeg
    for name, px, q, s, data in cases(g):
        st, d, coef = jpeg.entropy_decode(data)
        assert st == jpeg.OK, name
        e, want = jpeg_enc_ref.encode_planes(px, q, s)
        assert same_desc(d, e), name
        assert want.shape == coef.shape and np.array_equal(want, coef), '%s: %d coefficients differ' % (name, int((want != coef).sum()))


def test_quant_tables_equal_the_files(g):
    from ssd_tensorflow_amd import jpeg, _lib
    seen = set()
    for name, px, q, s, data in cases(g):
        if q in seen:
            continue
        seen.add(q)
        d = jpeg.entropy_decode(data)[1]
        luma, chroma = jpeg.quant_tables(q)
        assert list(luma) == list(d.qt[0]) and list(chroma) == list(d.qt[1]) == list(d.qt[2]), q
        ol, oc = jpeg_enc_ref.quant_tables(q)
        assert list(ol) == list(luma) and list(oc) == list(chroma)
    assert seen == {1, 30, 75, 95, 100}
    for q in (0, 101, -5):
        with pytest.raises(jpeg.JpegError, match='quality'):
            jpeg.quant_tables(q)
    for q in range(1, 101):                                       # baseline: every entry of every quality in 1..255
        luma, chroma = jpeg.quant_tables(q)
        assert 1 <= min(luma.min(), chroma.min()) and max(luma.max(), chroma.max()) <= 255


def test_host_stage_writes_libjpegs_file(g):
    """coefficients read from Pillow's file -> our file: the same bytes, header included (SOI, APP0 JFIF 1.01, DQT x 2, SOF0,
    DHT x 4, SOS, scan, EOI is the order libjpeg writes), and it reads back to the same descriptor and coefficients"""
    from ssd_tensorflow_amd import jpeg
    for name, px, q, s, data in cases(g):
        st, d, coef = jpeg.entropy_decode(data)
        ours = jpeg.entropy_encode(coef, d)
        assert scan(ours) == scan(data), name
        assert ours == data.tobytes(), name
        st2, d2, coef2 = jpeg.entropy_decode(ours)
        assert st2 == jpeg.OK and same_desc(d2, d) and d2.max_l1 == d.max_l1 and np.array_equal(coef2, coef), name


def test_pillow_reads_our_files(g):
    Image = pytest.importorskip('PIL.Image')
    from ssd_tensorflow_amd import jpeg
    for name, px, q, s, data in cases(g)[::7]:
        st, d, coef = jpeg.entropy_decode(data)
        with Image.open(io.BytesIO(jpeg.entropy_encode(coef, d))) as im:
            assert im.format == 'JPEG' and im.size == (px.shape[1], px.shape[0])
            ours = np.asarray(im.convert('RGB'))[:, :, ::-1]
        with Image.open(io.BytesIO(data.tobytes())) as im:
            theirs = np.asarray(im.convert('RGB'))[:, :, ::-1]
        assert np.array_equal(ours, theirs), name


def test_fixture_equals_a_live_pillow_encode(g):
    """a fixture that went stale with a libjpeg change shows here"""
    Image = pytest.importorskip('PIL.Image')
    for name, px, q, s, data in cases(g)[::5]:
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(px[:, :, ::-1])).save(buf, 'JPEG', quality=q, subsampling=s)
        assert buf.getvalue() == data.tobytes(), name


def _batch(g, picks):
    """the coefficients of several files in one buffer, descriptors relative to it"""
    from ssd_tensorflow_amd import jpeg
    datas = [c[4] for c in picks]
    coef, offs, descs, status, _ = jpeg.entropy_decode_batch(datas, threads=2)
    assert status == [jpeg.OK] * len(picks)
    return coef, descs, [d.tobytes() for d in datas]


@pytest.mark.parametrize('threads', [1, 3, 8])
def test_batch_equals_one_by_one(g, threads):
    from ssd_tensorflow_amd import jpeg
    picks = cases(g)[3::11]
    assert len(picks) >= 30
    coef, descs, want = _batch(g, picks)
    got = jpeg.entropy_encode_batch(coef, descs, threads=threads)
    assert len(got) == len(want)
    for (name, *_), a, b in zip(picks, got, want):
        assert a == b, name


def test_refusals_have_a_message(g):
    from ssd_tensorflow_amd import jpeg, _lib
    picks = cases(g)[200:203]
    coef, descs, want = _batch(g, picks)
    assert jpeg.entropy_encode_batch(coef, descs) == want

    def refused(text, coef=coef, descs=descs, threads=2):
        with pytest.raises(jpeg.JpegError, match=text):
            jpeg.entropy_encode_batch(coef, descs, threads=threads)

    for field, value, text in (('components', 1, 'components'), ('components', 4, 'components'), ('hs', 1, 'MCUs'), ('hs', 4, 'sampling'),
                               ('vs', 3, 'sampling'), ('width', 0, 'size'), ('height', 16385, 'size'), ('mcus_x', 0, 'MCUs'),
                               ('mcus_y', descs[1].mcus_y + 1, 'MCUs')):
        keep = getattr(descs[1], field)
        setattr(descs[1], field, value)
        refused('image 1: .*' + text)
        setattr(descs[1], field, keep)
    keep = descs[2].coef_off[2]
    descs[2].coef_off[2] = coef.size - 63                          # the last block would end one coefficient past the buffer
    refused('image 2: coefficient plane 2')
    descs[2].coef_off[2] = keep
    refused('image 2: coefficient plane', coef=coef[:-1])
    keep = descs[0].qt[1][5]
    for value, text in ((0, 'quantiser'), (256, 'quantiser'), (254 if keep == 255 else keep + 1, 'share one')):
        descs[0].qt[1][5] = value
        refused('image 0: .*' + text)
    descs[0].qt[1][5] = keep
    refused('threads', threads=0)
    refused('threads', threads=65)
    # a coefficient baseline Huffman cannot code: AC magnitude category 11, DC difference category 12
    bad = coef.copy()
    bad[descs[1].coef_off[0] + 9] = 1024
    refused('image 1: jpeg: AC coefficient 1024', coef=bad)
    bad[descs[1].coef_off[0] + 9] = -1023                          # category 10: coded
    assert jpeg.entropy_decode(jpeg.entropy_encode_batch(bad, descs)[1])[2][9] == -1023
    bad = coef.copy()
    bad[descs[1].coef_off[0]] = 2048
    refused('image 1: jpeg: DC difference 2048', coef=bad)
    assert jpeg.entropy_encode_batch(coef, descs) == want           # nothing above changed what a good call gives


_CHILD = r'''
import ctypes as C, mmap, sys
import numpy as np
lib = C.CDLL(sys.argv[1])
lib.ssd_last_error.restype = C.c_char_p
lib.ssd_jpeg_coef_bytes.restype = C.c_size_t
lib.ssd_jpeg_coef_bytes.argtypes = [C.c_void_p, C.c_size_t]
lib.ssd_jpeg_entropy_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
lib.ssd_jpeg_file_bound.restype = C.c_size_t
lib.ssd_jpeg_file_bound.argtypes = [C.c_void_p]
lib.ssd_jpeg_entropy_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
lib.ssd_jpeg_entropy_encode_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
libc = C.CDLL(None, use_errno=True)
libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
PAGE = mmap.PAGESIZE
g = np.load(sys.argv[2])
picks = list(range(0, len(g['case_names']), 9))
pages = max(g['case_%d_jpg' % i].size for i in picks) // PAGE + 2
mm = mmap.mmap(-1, pages * PAGE)
base = C.addressof(C.c_char.from_buffer(mm))
assert libc.mprotect(base + (pages - 1) * PAGE, PAGE, 0) == 0, C.get_errno()      # PROT_NONE behind the output
end = (pages - 1) * PAGE
checked = 0
for i in picks:
    data = g['case_%d_jpg' % i]
    coef = np.zeros(max(lib.ssd_jpeg_coef_bytes(data.ctypes.data, data.size) // 2, 8), np.int16)
    desc = (C.c_char * 1024)()
    st = C.c_int()
    assert lib.ssd_jpeg_entropy_decode(data.ctypes.data, data.size, coef.ctypes.data, coef.nbytes, desc, C.byref(st)) == 0 and st.value == 0
    n = data.size
    assert lib.ssd_jpeg_file_bound(desc) >= n
    size = C.c_size_t()
    # the exact capacity: the file, its last byte in front of the inaccessible page
    assert lib.ssd_jpeg_entropy_encode(coef.ctypes.data, coef.nbytes, desc, base + end - n, n, C.byref(size)) == 0, lib.ssd_last_error()
    assert size.value == n and mm[end - n:end] == data.tobytes()
    for cap in sorted({n - 1, n - 2, n - 3, n // 2, 700, 625, 624, 623, 100, 1, 0}):
        if 0 <= cap < n:
            rc = lib.ssd_jpeg_entropy_encode(coef.ctypes.data, coef.nbytes, desc, base + end - cap, cap, C.byref(size))
            assert rc != 0 and size.value == 0 and b'too small' in lib.ssd_last_error(), (i, cap, rc)
            checked += 1
    offs = (C.c_ulonglong * 2)(0, n - 1)
    sizes = (C.c_ulonglong * 1)()
    rc = lib.ssd_jpeg_entropy_encode_batch(coef.ctypes.data, coef.nbytes, desc, 1, 1, base + end - (n - 1), n - 1, offs, sizes)
    assert rc != 0 and lib.ssd_last_error().startswith(b'image 0: jpeg: the output buffer is too small'), lib.ssd_last_error()
    offs = (C.c_ulonglong * 2)(0, n)
    assert lib.ssd_jpeg_entropy_encode_batch(coef.ctypes.data, coef.nbytes, desc, 1, 1, base + end - n, n - 1, offs, sizes) != 0      # offsets past out_bytes
    assert b'past the' in lib.ssd_last_error()
print('checked', checked)
'''


def test_output_never_written_past_its_capacity(g, tmp_path):
    """each output buffer ends at the last byte in front of an inaccessible page; the child (ctypes, numpy and the library only --
    it never opens the GPU) writes every picked file at its exact size and is refused, with a message, at every smaller capacity,
    one byte short included"""
    script = tmp_path / 'child.py'
    script.write_text(_CHILD)
    lib_path = os.path.join(ROOT, 'ssd_tensorflow_amd', 'libssdvgg_hip.so')
    r = subprocess.run([sys.executable, str(script), lib_path, GOLDEN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, 'exit status %s\n%s' % (r.returncode, r.stderr[-3000:])
    assert r.stdout.startswith('checked ') and int(r.stdout.split()[1]) >= 300


def test_int32_bound_and_reciprocal_of_the_kernel():
    """every int32 value of the forward DCT stays below 2^31 for 8-bit samples, and umulhi(n, floor(2^32 / d) + 1)
    is n // d for every divisor d = 8 q, q in 1..255, over more than the reachable range of n"""
    rows, cols = jpeg_enc_ref.fdct_bounds()
    assert rows < cols < 2 ** 31
    reach = (cols >> 15) + 4 * 255 + 1                            # the largest column-pass output + half the largest divisor
    assert reach < 2 ** 16
    n = np.arange(2 ** 16, dtype=np.uint64)
    for q in range(1, 256):
        d = np.uint64(8 * q)
        m = np.uint64(2 ** 32 // (8 * q) + 1)
        assert m < 2 ** 32 and np.array_equal((n * m) >> np.uint64(32), n // d), q
