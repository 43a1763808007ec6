"""CPU: the host half of the device Huffman decoder (csrc/jpeg.hip's scan plan) and the chain itself, restated in
plain Python (tests/huffdec_ref.py), against the host stage on tests/golden/j1_jpeg.npz.  tests/test_gpu_jpeg_huffdec.py runs the
kernels against the same files."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import huffdec_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'j1_jpeg.npz')


@pytest.fixture(scope='module')
def g():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _list(g, kind):
    return [(str(n), g['%s_%d_jpg' % (kind, i)].tobytes()) for i, n in enumerate(g['%s_names' % kind])]


def _good(g):
    return _list(g, 'ok') + [(str(n), g['voc_%s_jpg' % n].tobytes()) for n in g['voc_names']]


def test_symbols_and_argument_checks():
    """1: the entry points exist; an unknown entropy stage is refused before torch or the GPU is touched"""
    from ssd_tensorflow_amd import jpeg, _lib
    for name in ('ssd_jpeg_scan_segments', 'ssd_jpeg_scan_plan', 'ssd_jpeg_huffdec_ws_bytes', 'ssd_jpeg_huffdec_batch_dev'):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert jpeg.TO_HOST == 3
    with pytest.raises(ValueError, match="entropy must be 'host' or 'gpu'"):
        jpeg.decode_batch([b'\xff\xd8\xff'], entropy='nope')
    with pytest.raises(ValueError, match="entropy must be 'host' or 'gpu'"):
        jpeg.decode(b'\xff\xd8\xff', entropy='nope')


def _marker_scan(data, pos, interval, mcus):
    """independent of the library: the segments of the scan that starts at `pos`, by walking the bytes"""
    segs, p, n = [], pos, len(data)
    want = math.ceil(mcus / interval) if interval else 1
    while len(segs) < want:
        begin = p
        while p < n and not (data[p] == 0xFF and (p + 1 >= n or data[p + 1] != 0)):
            p += 2 if data[p] == 0xFF else 1
        segs.append((begin, min(p, n)))
        while p + 1 < n and data[p + 1] == 0xFF:
            p += 1
        p += 2                                                # the marker
    return segs


def test_scan_plan_of_every_supported_file(g):
    """2, first half"""
    from ssd_tensorflow_amd import jpeg
    intervals = set()
    for name, data in _good(g):
        st, d, plan = jpeg.scan_plan(data)
        st2, d2, _ = jpeg.entropy_decode(data)
        assert st == st2 == jpeg.OK, name
        assert d.max_l1 == 0
        d.max_l1 = d2.max_l1
        assert bytes(d) == bytes(d2), name
        mcus = d.mcus_x * d.mcus_y
        want = math.ceil(mcus / plan.restart_interval) if plan.restart_interval else 1
        assert plan.segments == want == jpeg.lib.ssd_jpeg_scan_segments(data, len(data)), name
        assert plan.file_bytes == len(data)
        got = [(plan.seg[s].begin, plan.seg[s].end) for s in range(plan.segments)]
        assert got == _marker_scan(data, plan.scan_pos, plan.restart_interval, mcus), name
        assert data[plan.scan_pos - 3:plan.scan_pos] == b'\x00\x3f\x00'            # the end of the SOS header
        intervals.add(plan.restart_interval > 0)
    assert intervals == {False, True}


def test_scan_plan_of_unsupported_and_corrupt_files(g):
    """2, second half"""
    from ssd_tensorflow_amd import jpeg, _lib
    for name, data in _list(g, 'unsup'):
        _lib.lib.ssd_preset_info(b'nope', None, None, None, None)           # leaves an error text behind ...
        marker = _lib.last_error()
        st, d, plan = jpeg.scan_plan(data)
        assert st == jpeg.UNSUPPORTED and _lib.last_error() == marker, name    # ... that the plan did not replace
        assert jpeg.lib.ssd_jpeg_scan_segments(data, len(data)) == 0
    for name, data in _list(g, 'bad'):
        with pytest.raises(jpeg.JpegError) as host:
            jpeg.entropy_decode(data)
        try:
            st = jpeg.scan_plan(data)[0]
        except jpeg.JpegError as e:
            assert str(e) == str(host.value), name
            continue
        assert st in (jpeg.OK, jpeg.TO_HOST), name         # OK: the plan does not judge the bits; the device stage hands it over
        if name == 'restart_wrong_index':
            assert st == jpeg.TO_HOST


_CHILD = r'''
import ctypes as C, mmap, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from ssd_tensorflow_amd import jpeg
lib = jpeg.lib
libc = C.CDLL(None, use_errno=True)
libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
PAGE = mmap.PAGESIZE
g = np.load(sys.argv[2])
good = g['bad_source_jpg'].tobytes()
cases = [g['bad_%d_jpg' % i].tobytes() for i in range(len(g['bad_names']))]
cases += [good[:k] for k in list(range(0, 700)) + list(range(700, len(good), 5))]
cases += [g['unsup_%d_jpg' % i].tobytes() for i in range(len(g['unsup_names']))]
cases += [g['ok_%d_jpg' % i].tobytes() for i in range(len(g['ok_names']))]
cases += [c[:-2] for c in cases[-72:]] + [c[:-1] for c in cases[-72:]]                  # the scan runs into the end of the input
pages = max(len(c) for c in cases) // PAGE + 2
mm = mmap.mmap(-1, pages * PAGE)
base = C.addressof(C.c_char.from_buffer(mm))
assert libc.mprotect(base + (pages - 1) * PAGE, PAGE, 0) == 0, C.get_errno()      # PROT_NONE behind the input
end = (pages - 1) * PAGE
segs = (jpeg.Segment * 70000)()
st = C.c_int()
for data in cases:
    n = len(data)
    mm[end - n:end] = data
    ptr = base + end - n
    lib.ssd_jpeg_scan_segments(ptr, n)
    plan, desc = jpeg.Plan(), jpeg.Desc()
    plan.seg, plan.seg_cap = segs, 70000
    lib.ssd_jpeg_scan_plan(ptr, n, C.byref(desc), C.byref(plan), C.byref(st))
    if st.value == 0:
        assert all(plan.seg[s].begin <= plan.seg[s].end <= n for s in range(plan.segments))
print('checked', len(cases))
'''


def test_scan_plan_never_reads_past_the_last_byte(g, tmp_path):
    """2, last item: each input ends at the last byte in front of an inaccessible page (the arrangement of tests/test_jpeg.py;
    the child never opens the GPU)"""
    script = tmp_path / 'child.py'
    script.write_text(_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, GOLDEN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, 'exit status %s\n%s' % (r.returncode, r.stderr[-3000:])
    assert r.stdout.startswith('checked ')


def test_reference_chain_equals_the_host_stage(g):
    """3: subsequences of 16 bytes whose exit states travel one subsequence per round, so even small files have long chains"""
    from ssd_tensorflow_amd import jpeg
    small = [(n, d) for n, d in _list(g, 'ok') if len(d) <= 3000]
    assert len(small) >= 30
    failed_at_one = 0
    for name, data in small:
        st, d, plan = jpeg.scan_plan(data)
        _, d2, coef = jpeg.entropy_decode(data)
        ok, got, max_l1 = huffdec_ref.decode(data, d, plan, subseq=16, group=1, max_rounds=256)
        assert ok and np.array_equal(got, coef) and max_l1 == d2.max_l1, name
        failed_at_one += not huffdec_ref.decode(data, d, plan, subseq=16, group=1, max_rounds=1)[0]
    assert failed_at_one >= 1                                 # the write pass's re-check is live


ROUNDS = {}


def _rounds(name, data):
    from ssd_tensorflow_amd import jpeg
    if name not in ROUNDS:
        st, d, plan = jpeg.scan_plan(data)
        ROUNDS[name] = huffdec_ref.rounds_needed(data, d, plan)
    return ROUNDS[name]


def _generated():
    """test 7's pictures (tests/test_gpu_jpeg_huffdec.py), the ones Pillow writes"""
    Image = pytest.importorskip('PIL.Image')
    import io
    rng = np.random.default_rng(716)
    noise = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)
    smooth = np.clip(np.add.outer(np.arange(375), np.arange(500))[:, :, None] * np.array([0.2, 0.25, 0.3]) + rng.normal(0, 6, (375, 500, 3)), 0, 255)

    def save(img, **kw):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG', **kw)
        return buf.getvalue()
    return [('noise_q100_444', save(noise, quality=100, subsampling=0)), ('noise_q100_420', save(noise, quality=100, subsampling=2)),
            ('flat_512', save(np.full((512, 512, 3), (90, 140, 200), np.uint8), quality=90)),
            ('grey_144x96', save(noise[:96, :144, 0], quality=85)), ('rst1_500x375', save(smooth.astype(np.uint8), quality=85, restart_marker_blocks=1))]


def test_default_round_budget_is_twice_what_any_file_needs(g):
    """4: with the kernel's own subsequence and group size.  (The largest files run once here: a few seconds of Python.)"""
    assert (huffdec_ref.KERNEL_SUBSEQ, huffdec_ref.KERNEL_GROUP) == (64, 256)
    needed = {name: _rounds(name, data) for name, data in _good(g) + _generated()}
    assert None not in needed.values()
    worst = max(needed.values())
    print('rounds needed: %d at most (%s); default budget %d' % (worst, [n for n, r in needed.items() if r == worst][:4], huffdec_ref.KERNEL_DEFAULT_ROUNDS))
    assert huffdec_ref.KERNEL_DEFAULT_ROUNDS >= 2 * worst
    src = open(os.path.join(ROOT, 'ssd_tensorflow_amd', 'csrc', 'jpeg_huffdec.hip')).read()
    for key, value in (('SUBSEQ', 64), ('GROUP', 256), ('DEFAULT_ROUNDS', huffdec_ref.KERNEL_DEFAULT_ROUNDS)):
        assert 'constexpr int %s = %d;' % (key, value) in src, key
