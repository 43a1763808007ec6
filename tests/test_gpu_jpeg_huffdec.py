"""GPU: the device Huffman decoder (csrc/jpeg_huffdec.hip) against the host stage it replaces
(ssd_jpeg_entropy_decode): coefficient slots byte for byte, max_l1, and -- for damaged input -- the same exception or the same
pixels through decode_batch.  Damaged bytes do reach these kernels: every read is guarded by the segment's end and every write by
the image's block count, which the guard bands around the slots check.  Reads only files of this repository."""
import ctypes as C
import filecmp
import io
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'j1_jpeg.npz')
GUARD = 256                                  # bytes of guard band in front of, between and behind the coefficient slots
PATTERN = 0x5A


@pytest.fixture(scope='module')
def g():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


_HOST = {}


def host_stage(data):
    """the reference, computed once per input: (status, Desc, coefficients) or the JpegError's text"""
    from ssd_tensorflow_amd import jpeg
    if data not in _HOST:
        try:
            _HOST[data] = jpeg.entropy_decode(data)
        except jpeg.JpegError as e:
            _HOST[data] = str(e)
    return _HOST[data]


def _ok(g):
    return [(str(n), g['ok_%d_jpg' % i].tobytes(), g['ok_%d_bgr' % i]) for i, n in enumerate(g['ok_names'])]


def _voc(g):
    return [(str(n), g['voc_%s_jpg' % n].tobytes()) for n in g['voc_names']]


def huffdec(datas, max_rounds=0, fill=None, bufs=None):
    """ssd_jpeg_huffdec_batch_dev on a list of files whose plan is OK: (records [(status, max_l1)], [coefficient slot as int16
    array], guard bands intact?).  fill: byte to pre-fill workspace and coefficient buffer with; bufs: dict that keeps the
    device buffers from one call to the next."""
    import torch
    from ssd_tensorflow_amd import jpeg, _lib
    n = len(datas)
    dev = torch.device('cuda', 0)
    plans, descs, keep = (jpeg.Plan * n)(), (jpeg.Desc * n)(), []
    foff, coff, fbytes, cbytes = [], [], 0, GUARD
    for k, data in enumerate(datas):
        st, d, plan = jpeg.scan_plan(data, plans[k])
        assert st == jpeg.OK
        keep.append(plan._segs)
        C.memmove(C.byref(descs[k]), C.byref(d), C.sizeof(jpeg.Desc))
        plans[k].file_off = fbytes
        foff.append(fbytes)
        fbytes += (len(data) + 15) // 16 * 16
        nbytes = _lib.lib.ssd_jpeg_coef_bytes(data, len(data))
        coff.append((cbytes, nbytes))
        for c in range(3):
            descs[k].coef_off[c] += cbytes // 2
        cbytes += nbytes + GUARD
    files = np.zeros(fbytes, np.uint8)
    for k, data in enumerate(datas):
        files[foff[k]:foff[k] + len(data)] = np.frombuffer(data, np.uint8)
    files_dev = torch.from_numpy(files).to(dev)
    ws_bytes = _lib.lib.ssd_jpeg_huffdec_ws_bytes(plans, descs, n)
    assert ws_bytes > 0, _lib.last_error()
    bufs = {} if bufs is None else bufs
    if 'ws' not in bufs:
        bufs['ws'] = torch.zeros((ws_bytes,), dtype=torch.uint8, device=dev)
        bufs['coef'] = torch.zeros((cbytes,), dtype=torch.uint8, device=dev)
    ws, coef = bufs['ws'], bufs['coef']
    assert ws.numel() == ws_bytes and coef.numel() == cbytes
    if fill is not None:
        ws.fill_(fill)
    coef.fill_(PATTERN)
    if fill is not None:
        for off, nbytes in coff:
            coef[off:off + nbytes] = fill
    recs = torch.full((n * 2,), -1, dtype=torch.int32, device=dev)
    rc = _lib.lib.ssd_jpeg_huffdec_batch_dev(files_dev.data_ptr(), fbytes, plans, descs, n, coef.data_ptr(), cbytes, recs.data_ptr(),
                                             ws.data_ptr(), ws_bytes, max_rounds, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    host = coef.cpu().numpy()
    r = recs.cpu().numpy().reshape(n, 2)
    guards = np.ones(cbytes, bool)
    for off, nbytes in coff:
        guards[off:off + nbytes] = False
    intact = bool((host[guards] == PATTERN).all())
    return [(int(a), int(b)) for a, b in r], [host[off:off + nbytes].view(np.int16) for off, nbytes in coff], intact


def check_equal_to_host(names, datas, recs, slots, handoffs=()):
    from ssd_tensorflow_amd import jpeg
    for name, data, rec, slot in zip(names, datas, recs, slots):
        st, d, coef = host_stage(data)
        if name in handoffs:
            assert rec[0] == jpeg.TO_HOST, name
            continue
        assert rec[0] == jpeg.OK, '%s: handed to the host stage' % name
        assert st == jpeg.OK or (st == jpeg.UNSUPPORTED and d.max_l1 > jpeg.MAX_L1), name
        assert rec[1] == d.max_l1, (name, rec, d.max_l1)
        assert slot.size == coef.size and np.array_equal(slot, coef), '%s: %d coefficients differ' % (name, int((slot != coef[:slot.size]).sum()))


def test_fixture_files_alone_and_in_one_shuffled_batch(g):
    """5: every coefficient slot equals the host stage's, zeros and padding blocks included; no file is handed to the host"""
    files = [(n, d) for n, d, _ in _ok(g)] + _voc(g)
    assert len(files) == 74
    for name, data in files:
        recs, slots, intact = huffdec([data])
        check_equal_to_host([name], [data], recs, slots)
        assert intact, name
    random.Random(5).shuffle(files)
    recs, slots, intact = huffdec([d for _, d in files])
    check_equal_to_host([n for n, _ in files], [d for _, d in files], recs, slots)
    assert intact


def test_repeatable_into_a_dirty_workspace(g):
    """6: the same batch twice into one workspace, and once into a workspace and coefficient buffer full of FF"""
    files = [(n, d) for n, d, _ in _ok(g)][::3] + _voc(g)
    datas = [d for _, d in files]
    bufs = {}
    first = huffdec(datas, bufs=bufs)
    check_equal_to_host([n for n, _ in files], datas, first[0], first[1])
    for fill in (None, 0xFF):
        again = huffdec(datas, fill=fill, bufs=bufs)
        assert again[0] == first[0] and again[2]
        assert all(np.array_equal(a, b) for a, b in zip(again[1], first[1]))


def _pillow(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def _crafted(blocks, qt=1, w=8, h=8):
    """a 4:4:4 file of given luma blocks ([n][64] natural order; chroma blocks EOB only) through jpeg.entropy_encode"""
    from ssd_tensorflow_amd import jpeg
    mx, my = (w + 7) // 8, (h + 7) // 8
    assert len(blocks) == mx * my
    d = jpeg.Desc()
    d.width, d.height, d.components, d.hs, d.vs, d.mcus_x, d.mcus_y = w, h, 3, 1, 1, mx, my
    coef = np.zeros(3 * mx * my * 64, np.int16)
    coef[:mx * my * 64] = np.asarray(blocks, np.int16).reshape(-1)
    for c in range(3):
        d.coef_off[c] = c * mx * my * 64
        for k in range(64):
            d.qt[c][k] = qt
    return jpeg.entropy_encode(coef, d)


def _guard_block(dc):
    """test_range_guard's recipe: alternating sign in all 64 positions, L1 norm 14742 + dc at q = 1"""
    coefs = [234 * (1 if i % 2 == 0 else -1) for i in range(64)]
    coefs[0] = dc
    return coefs


@pytest.fixture(scope='module')
def shapes():
    """7: shapes where the chain can go wrong (seeded)"""
    pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(716)
    noise = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)
    out = [('noise_q100_444', _pillow(noise, quality=100, subsampling=0)), ('noise_q100_420', _pillow(noise, quality=100, subsampling=2)),
           ('flat_512', _pillow(np.full((512, 512, 3), (90, 140, 200), np.uint8), quality=90)),
           ('1x1', _pillow(noise[:1, :1], quality=90)), ('8x8', _pillow(noise[:8, :8], quality=90)),
           ('grey_144x96', _pillow(noise[:96, :144, 0], quality=85))]
    smooth = np.clip(np.add.outer(np.arange(375), np.arange(500))[:, :, None] * np.array([0.2, 0.25, 0.3]) + rng.normal(0, 6, (375, 500, 3)), 0, 255)
    from ssd_tensorflow_amd import jpeg
    rst = _pillow(smooth.astype(np.uint8), quality=85, restart_marker_blocks=1)
    if jpeg.scan_plan(rst)[2].restart_interval == 1:             # (a Pillow without restart_marker_blocks ignores the keyword)
        out.append(('rst1_500x375', rst))
    longest = np.array([[0] + [1023 * (1 if i % 2 else -1) for i in range(1, 64)]] * 4)
    out.append(('ac_category_10', _crafted(longest, w=16, h=16)))
    out.append(('eob_only', _crafted(np.zeros((64, 64), int), w=64, h=64)))
    out.append(('l1_15000', _crafted([_guard_block(258)])))
    out.append(('l1_15001', _crafted([_guard_block(259)])))
    return out


def test_shapes_where_the_chain_can_go_wrong(shapes):
    """7: coefficients equal the host stage's everywhere, no hand-offs; 15000 is accepted, 15001 falls back in decode_batch"""
    from ssd_tensorflow_amd import jpeg
    names, datas = [n for n, _ in shapes], [d for _, d in shapes]
    recs, slots, intact = huffdec(datas)
    check_equal_to_host(names, datas, recs, slots)
    assert intact
    assert recs[names.index('l1_15000')][1] == 15000 and recs[names.index('l1_15001')][1] == 15001
    assert recs[names.index('ac_category_10')][1] == 63 * 1023
    for name, data in shapes:
        recs, slots, intact = huffdec([data])
        check_equal_to_host([name], [data], recs, slots)
    picks = [datas[names.index(n)] for n in ('l1_15000', 'l1_15001', 'ac_category_10', '8x8')]
    got, want = jpeg.decode_batch(picks, entropy='gpu'), jpeg.decode_batch(picks, entropy='host')
    assert got[3] == want[3] == [1, 2] and got[1:3] == want[1:3]


def _pixels(result):
    dst, offs, sizes, fallbacks = result
    host = dst.cpu().numpy()
    return [host[o:o + h * w * 3].tobytes() for o, (h, w) in zip(offs, sizes)]


def test_one_round_is_caught_by_the_write_pass(g):
    """8: with a budget of one round the VOC files' chains cannot have settled: SSD_JPEG_TO_HOST, the neighbours intact, and
    decode_batch still returns the fixture's pixels (through the host stage)"""
    import hashlib
    from ssd_tensorflow_amd import jpeg
    ok, voc = _ok(g), _voc(g)
    files = [(ok[3][0], ok[3][1]), voc[0], (ok[40][0], ok[40][1]), voc[1], (ok[11][0], ok[11][1])]
    names, datas = [n for n, _ in files], [d for _, d in files]
    recs, slots, intact = huffdec(datas, max_rounds=1)
    check_equal_to_host(names, datas, recs, slots, handoffs=[n for n, _ in voc])
    assert intact
    result = jpeg.decode_batch(datas, entropy='gpu', _max_rounds=1)
    assert result[3] == []
    px = _pixels(result)
    for i in (0, 2, 4):
        assert px[i] == ok[(3, 0, 40, 0, 11)[i]][2].tobytes()
    for i, (name, _) in ((1, voc[0]), (3, voc[1])):
        assert hashlib.sha256(px[i]).hexdigest() == str(g['voc_%s_sha256' % name])


def _damaged(g, kind):
    names = [str(n) for n in g['ok_names']]
    if kind == 'bad':
        return [(str(n), g['bad_%d_jpg' % i].tobytes()) for i, n in enumerate(g['bad_names'])]
    if kind == 'cuts_small':
        i = next(i for i, n in enumerate(names) if '420_small_16x16' in n)
        data = g['ok_%d_jpg' % i].tobytes()
        assert len(data) == 740
        return [('cut_%d' % k, data[:k]) for k in range(len(data))]
    if kind == 'cuts_source':
        data = g['bad_source_jpg'].tobytes()
        return [('cut_%d' % k, data[:k]) for k in range(0, len(data), 37)]
    i = next(i for i, n in enumerate(names) if '444_noise_40x24' in n)
    data = g['ok_%d_jpg' % i].tobytes()
    from ssd_tensorflow_amd import jpeg
    scan = jpeg.scan_plan(data)[2].scan_pos
    rng = random.Random(512)
    out = []
    for _ in range(512):
        bit = rng.randrange(scan * 8, (len(data) - 2) * 8)
        b = bytearray(data)
        b[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append(('flip_%d' % bit, bytes(b)))
    return out


def _outcome(items, **kw):
    from ssd_tensorflow_amd import jpeg
    try:
        result = jpeg.decode_batch(items, **kw)
    except Exception as e:                                   # JpegError, or whatever the fallback raises for bytes it cannot open
        return (type(e).__name__, re.sub(r'0x[0-9a-f]+', '0x', str(e)))      # (Pillow's text names an object's address)
    return ('ok', result[1], result[2], result[3], _pixels(result))


@pytest.mark.parametrize('kind', ['bad', 'cuts_small', 'cuts_source', 'flips'])
def test_equivalence_under_damage(g, kind):
    """9: for every damaged input, between two good files, decode_batch(entropy='gpu') raises or returns exactly what
    entropy='host' does; at ABI level the inputs whose plan is usable run as one batch between good files and guard bands"""
    pytest.importorskip('PIL.Image')                         # (the fallback of a bytes item is Pillow)
    from ssd_tensorflow_amd import jpeg
    ok = _ok(g)
    good = [ok[7], ok[30]]
    cases = _damaged(g, kind)
    accepted = 0
    for name, data in cases:
        items = [good[0][1], data, good[1][1]]
        got, want = _outcome(items, entropy='gpu'), _outcome(items, entropy='host', threads=1)
        assert got == want, (name, got[:2], want[:2])
        if got[0] == 'ok':
            accepted += 1
            assert got[4][0] == good[0][2].tobytes() and got[4][2] == good[1][2].tobytes(), name
    # ABI level: every input with a usable plan, good files interleaved, guard bands around every slot
    batch = []
    for name, data in cases:
        try:
            if jpeg.scan_plan(data)[0] == jpeg.OK:
                batch += [(name, data), good[len(batch) // 2 % 2][:2]]
        except jpeg.JpegError:
            pass
    handoffs = 0
    if batch:
        recs, slots, intact = huffdec([d for _, d in batch])
        assert intact
        for (name, data), rec, slot in zip(batch, recs, slots):
            ref = host_stage(data)
            if rec[0] == jpeg.OK:                            # accepted: then with the host stage's outcome, nothing else
                assert not isinstance(ref, str), (name, ref)
                st, d, coef = ref
                assert st == jpeg.OK or (st == jpeg.UNSUPPORTED and d.max_l1 > jpeg.MAX_L1), name
                assert rec[1] == d.max_l1 and np.array_equal(slot, coef), name
            else:
                assert rec[0] == jpeg.TO_HOST, (name, rec)
                handoffs += 1
        for (name, data), rec in zip(batch[1::2], recs[1::2]):
            assert rec[0] == jpeg.OK, name
    print('%s: %d inputs, %d decode to pixels, %d with a usable plan, %d handed to the host stage'
          % (kind, len(cases), accepted, len(batch) // 2, handoffs))


def test_mixed_lists_through_decode_batch(g, tmp_path):
    """10: all 72 supported files equal their fixture pixels; a list of supported and unsupported files, a PNG, a .npy file and
    an array returns what entropy='host' returns"""
    Image = pytest.importorskip('PIL.Image')
    from ssd_tensorflow_amd import jpeg
    ok = _ok(g)
    result = jpeg.decode_batch([d for _, d, _ in ok], entropy='gpu')
    assert result[3] == []
    for (name, _, want), px in zip(ok, _pixels(result)):
        assert px == want.tobytes(), name
    assert np.array_equal(jpeg.decode(ok[5][1], entropy='gpu'), ok[5][2])
    png, npy, jpg = str(tmp_path / 'a.png'), str(tmp_path / 'b.npy'), str(tmp_path / 'c.jpg')
    Image.fromarray(ok[2][2][:, :, ::-1]).save(png)
    np.save(npy, ok[9][2])
    open(jpg, 'wb').write(ok[20][1])
    items = [ok[0][1], g['unsup_0_jpg'].tobytes(), png, jpg, npy, ok[12][2], g['unsup_3_jpg'].tobytes(), ok[33][1], g['guard_beyond_jpg'].tobytes()]
    got, want = _outcome(items, entropy='gpu'), _outcome(items, entropy='host')
    assert got[0] == 'ok' and got == want
    assert got[3] == [1, 2, 4, 5, 6, 8]


def test_entry_point_refusals(g):
    """11: each refusal comes with a message and before any launch (the buffers stay as they were)"""
    import torch
    from ssd_tensorflow_amd import jpeg, _lib
    datas = [g['ok_%d_jpg' % i].tobytes() for i in (0, 1, 2)]
    n = 3
    dev = torch.device('cuda', 0)
    plans, descs, keep = (jpeg.Plan * n)(), (jpeg.Desc * n)(), []
    fbytes = cbytes = 0
    for k, data in enumerate(datas):
        st, d, plan = jpeg.scan_plan(data, plans[k])
        keep.append(plan._segs)
        C.memmove(C.byref(descs[k]), C.byref(d), C.sizeof(jpeg.Desc))
        plans[k].file_off = fbytes
        fbytes += (len(data) + 15) // 16 * 16
        for c in range(3):
            descs[k].coef_off[c] += cbytes // 2
        cbytes += _lib.lib.ssd_jpeg_coef_bytes(data, len(data))
    files = np.zeros(fbytes + 16, np.uint8)
    for k, data in enumerate(datas):
        files[plans[k].file_off:plans[k].file_off + len(data)] = np.frombuffer(data, np.uint8)
    files_dev = torch.from_numpy(files).to(dev)
    ws_bytes = _lib.lib.ssd_jpeg_huffdec_ws_bytes(plans, descs, n)
    assert ws_bytes > 0
    ws = torch.zeros((ws_bytes + 16,), dtype=torch.uint8, device=dev)
    coef = torch.full((cbytes + 16,), PATTERN, dtype=torch.uint8, device=dev)
    recs = torch.full((n * 2,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream

    def run(files_bytes=fbytes, coef_bytes=cbytes, ws_b=ws_bytes, count=n, files_ptr=0, coef_ptr=0, ws_ptr=0, rounds=0):
        return _lib.lib.ssd_jpeg_huffdec_batch_dev(files_dev.data_ptr() + files_ptr, files_bytes, plans, descs, count, coef.data_ptr() + coef_ptr,
                                                   coef_bytes, recs.data_ptr(), ws.data_ptr() + ws_ptr, ws_b, rounds, s)

    for kw, text in ((dict(files_bytes=int(plans[2].file_off) + len(datas[2]) - 1), 'outside the'), (dict(coef_bytes=cbytes - 128), 'coefficients at offset'),
                     (dict(ws_b=ws_bytes - 256), 'workspace'), (dict(count=0), 'empty batch'), (dict(files_ptr=4), 'aligned'),
                     (dict(coef_ptr=2), 'aligned'), (dict(ws_ptr=8), 'aligned'), (dict(rounds=-1), 'max_rounds'), (dict(rounds=65), 'max_rounds')):
        assert run(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    # a segment range past the file, a segment count that contradicts the descriptor, a coefficient plane out of place
    keep_end = plans[1].seg[0].end
    plans[1].seg[0].end = plans[1].file_bytes + 1
    assert run() != 0 and 'outside the file' in _lib.last_error()
    assert _lib.lib.ssd_jpeg_huffdec_ws_bytes(plans, descs, n) == 0
    plans[1].seg[0].end = keep_end
    for obj, field, value, text in ((plans[1], 'segments', plans[1].segments + 1, 'segments'),
                                    (plans[0], 'file_off', 8, 'outside the'), (descs[1], 'mcus_x', 0, 'MCUs'), (descs[1], 'hs', 3, 'sampling'),
                                    (descs[2], 'width', 0, 'size')):
        old = getattr(obj, field)
        setattr(obj, field, value)
        assert run() != 0 and text in _lib.last_error(), (field, _lib.last_error())
        setattr(obj, field, old)
    old = descs[1].coef_off[1]
    descs[1].coef_off[1] = old + 64
    assert run() != 0 and 'does not follow' in _lib.last_error()
    descs[1].coef_off[1] = old
    torch.cuda.synchronize()
    assert bool((coef == PATTERN).all()) and bool((recs == -1).all())          # the refused calls launched nothing
    assert run() == 0
    torch.cuda.synchronize()
    assert recs.cpu().numpy().reshape(n, 2)[:, 0].tolist() == [jpeg.OK] * n


def _child(args, seconds=600):
    r = subprocess.run([sys.executable, '-m'] + args, cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    assert r.returncode == 0, '%s\n%s\n%s' % (args, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def _same_dirs(a, b, count):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) == count, (names, sorted(os.listdir(b)))
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


def test_detect_with_both_entropy_stages(g, tmp_path):
    """12: detect.py on four fixture files as a child process, --decoder-entropy gpu and host: the same annotated pictures and
    the same .txt files"""
    pytest.importorskip('PIL.Image')
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    names = [str(n) for n in g['ok_names']]
    picks = [n for n in names if n.endswith(('104x88', '144x96', '80x81', '95x65', '47x63'))][:3]
    files = []
    for n in picks:
        files.append(str(tmp_path / (n + '.jpg')))
        open(files[-1], 'wb').write(g['ok_%d_jpg' % names.index(n)].tobytes())
    files.append(str(tmp_path / 'voc.jpg'))
    open(files[-1], 'wb').write(_voc(g)[0][1])
    model = str(tmp_path / 'model.npz')
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 3, max_batch=4)
        net.build_optimizer()
        net.save_checkpoint(model, class_names=['class_%d' % i for i in range(3)])
    out = {}
    for ent in ('gpu', 'host'):
        out[ent] = str(tmp_path / ('detect_' + ent))
        _child(['ssd_tensorflow_amd.detect', '--model', model, '--output-dir', out[ent], '--batch-size', '4', '--decoder', 'gpu',
                '--decoder-entropy', ent] + files)
    _same_dirs(out['gpu'], out['host'], 8)
