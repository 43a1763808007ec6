"""GPU: Huffman coding and file framing on the GPU (csrc/jpeg_huff.hip) against the host stage
(jpeg.entropy_encode), which tests/test_jpeg_encode.py pins against libjpeg-turbo's own files; jpeg.encode_batch(entropy='gpu')
end to end against Pillow's files (tests/golden/j2_jpeg_encode.npz); the drivers' --jpeg-entropy gpu.  Reads only files of this
repository.  Everything is exact: no tolerance, no case left out.  Nothing here sends bad arguments to a kernel: the entry point
refuses them before it launches, and a coefficient baseline Huffman cannot code is a reported status, not a fault."""
import ctypes as C
import filecmp
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import huff_ref
import jpeg_enc_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'j2_jpeg_encode.npz')
QUALITIES = [1, 30, 75, 95, 100]
SAMPLINGS = ['4:4:4', '4:2:2', '4:2:0']
FILL = 0x5a


@pytest.fixture(scope='module')
def g():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def pictures(g):
    return [g['src_%d_bgr' % j] for j in range(len(g['src_names']))]


def pillow_file(g, j, q, s):
    i = next(i for i in range(len(g['case_names'])) if (int(g['case_src'][i]), int(g['case_quality'][i]), str(g['case_sampling'][i])) == (j, q, s))
    return g['case_%d_jpg' % i].tobytes()


class Batch:
    """images' coefficients in one buffer, one image after the other, and their descriptors"""
    def __init__(self):
        self.parts, self.descs, self.size = [], [], 0

    def add(self, coef, width=8, height=8, hs=1, vs=1, quality=95):
        d, n = huff_ref.make_desc(width, height, hs, vs, quality, base=self.size)
        coef = np.ascontiguousarray(coef, np.int16).reshape(-1)
        assert coef.size == n
        self.parts.append(coef)
        self.descs.append(d)
        self.size += n
        return len(self.descs) - 1

    def add_picture(self, bgr, quality, subsampling):
        """the coefficients of a picture, from the numpy oracle of the device stage"""
        e, coef = jpeg_enc_ref.encode_planes(bgr, quality, subsampling)
        i = self.add(coef, e.width, e.height, e.hs, e.vs, quality)
        d = self.descs[i]
        assert (d.mcus_x, d.mcus_y) == (e.mcus_x, e.mcus_y) and [list(t) for t in d.qt] == e.qt
        assert [int(d.coef_off[c]) - int(d.coef_off[0]) for c in range(3)] == e.coef_off
        return i

    def coef(self):
        return np.concatenate(self.parts)

    def host_files(self):
        from ssd_tensorflow_amd import jpeg
        coef = self.coef()
        return [jpeg.entropy_encode(coef, d) for d in self.descs]


class Stage:
    """ssd_jpeg_huffman_batch_dev on a batch: buffers of exactly the declared sizes in front of a guard, all pre-filled"""
    GUARD = 4096

    def __init__(self, batch):
        import torch
        from ssd_tensorflow_amd import jpeg, _lib
        self.lib, self.n = _lib.lib, len(batch.descs)
        self.descs = (jpeg.Desc * self.n)(*batch.descs)
        dev = torch.device('cuda', 0)
        self.coef = torch.from_numpy(batch.coef()).to(dev)
        self.coef_bytes = self.coef.numel() * 2
        self.ws_bytes, self.out_bytes = self.lib.ssd_jpeg_huff_ws_bytes(self.descs, self.n), self.lib.ssd_jpeg_huff_out_bytes(self.descs, self.n)
        assert self.ws_bytes > 0 and self.out_bytes > 0, _lib.last_error()
        self.ws = torch.full((self.ws_bytes + self.GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.out = torch.full((self.out_bytes + self.GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.recs = torch.full(((self.n + 4) * C.sizeof(jpeg.FileRec),), FILL, dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def call(self, **kw):
        a = dict(coef=self.coef.data_ptr(), coef_bytes=self.coef_bytes, descs=self.descs, n=self.n, out=self.out.data_ptr(), out_bytes=self.out_bytes,
                 recs=self.recs.data_ptr(), ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(kw)
        return self.lib.ssd_jpeg_huffman_batch_dev(a['coef'], a['coef_bytes'], a['descs'], a['n'], a['out'], a['out_bytes'], a['recs'], a['ws'],
                                                   a['ws_bytes'], self.stream)

    def run(self):
        """(records, files or None): one launch, the guards checked"""
        import torch
        from ssd_tensorflow_amd import jpeg, _lib
        assert self.call() == 0, _lib.last_error()
        torch.cuda.synchronize()
        raw = self.recs.cpu().numpy()
        out = self.out.cpu().numpy()
        size = self.n * C.sizeof(jpeg.FileRec)
        assert (raw[size:] == FILL).all() and (out[self.out_bytes:] == FILL).all() and bool((self.ws[self.ws_bytes:] == FILL).all())
        recs = (jpeg.FileRec * self.n).from_buffer_copy(raw[:size].tobytes())
        at = 0
        for r in recs:
            assert r.offset == at and r.reserved == 0 and (r.size == 0) == (r.status != 0)
            at += (r.size + 15) // 16 * 16
        assert at <= self.out_bytes
        return recs, [out[r.offset:r.offset + r.size].tobytes() if r.status == 0 else None for r in recs]


def check(batch, names=None):
    recs, files = Stage(batch).run()
    want = batch.host_files()
    for i, (got, w) in enumerate(zip(files, want)):
        assert recs[i].status == 0, (i, recs[i].status)
        assert got == w, '%s: %d bytes against the host stage\'s %d, first difference at byte %s' % (
            names[i] if names else i, len(got), len(w), next((k for k in range(min(len(got), len(w))) if got[k] != w[k]), 'the end'))
    return files


# ---------------------------------------------------------------------------------------------------------------- 1. the fixture
@pytest.mark.parametrize('subsampling', SAMPLINGS)
def test_fixture_files_equal_pillow_and_the_host_stage(g, subsampling):
    from ssd_tensorflow_amd import jpeg
    pics = pictures(g)
    names = [str(n) for n in g['src_names']]
    single = [j for j, n in enumerate(names) if n.endswith(('_1x1', '_8x8', '_144x96'))]
    assert len(single) == 6
    for q in QUALITIES:
        files = jpeg.encode_batch(pics, quality=q, subsampling=subsampling, entropy='gpu')
        assert files == [pillow_file(g, j, q, subsampling) for j in range(len(pics))], (q, subsampling)
        assert files == jpeg.encode_batch(pics, quality=q, subsampling=subsampling, entropy='host')
        for j in single:
            assert jpeg.encode_batch([pics[j]], quality=q, subsampling=subsampling, entropy='gpu') == [files[j]], (names[j], q)
    if subsampling == '4:2:0':
        assert jpeg.encode(pics[5], entropy='gpu') == pillow_file(g, 5, 95, '4:2:0')
        with pytest.raises(ValueError):
            jpeg.encode_batch(pics[:2], entropy='device')


# ------------------------------------------------------------------------------------------------- 2. crafted coefficients
def block(dc=0, ac=()):
    """a natural-order block from a DC and (zigzag position, value) pairs"""
    b = np.zeros(64, np.int16)
    b[0] = dc
    for pos, v in ac:
        b[huff_ref.ZIGZAG[pos]] = v
    return b


def test_crafted_blocks():
    batch, names = Batch(), []

    def add(name, *blocks, **kw):
        names.append(name)
        return batch.add(np.concatenate(blocks), **kw)

    zero = block()
    z = add('all zero', zero, zero, zero)
    for pos in (63, 62, 1):
        for v in (1, -1, 1023, -1023, 512, -512):
            add('only zigzag %d = %d' % (pos, v), block(0, [(pos, v)]), block(5, [(pos, -v)]), block(-5, [(pos, v)]))
    for run in (15, 16, 17, 31, 32, 33, 47, 48, 49, 62):
        add('run %d from the DC' % run, block(3, [(run + 1, 7)]), block(0, [(run + 1, -7)]), block(-1, [(run + 1, 1)]))
        if run + 6 <= 63:
            add('run %d behind zigzag 5' % run, block(3, [(5, -2), (run + 6, 7)]), block(0, [(5, 300), (run + 6, -7)]), block(0, [(5, 1), (run + 6, 1), (63, -1)]))
    # every DC category, both signs: differences 0, +-1, +-(2^c - 1), +-2^(c-1) ... up to +-2047, the DCs stay in 0..2047
    diffs = [2047, -2047, 0]
    for c in range(1, 12):
        diffs += [(1 << c) - 1, -((1 << c) - 1), 1 << (c - 1), -(1 << (c - 1))]
    dcs = np.cumsum(diffs)
    assert dcs.min() == 0 and dcs.max() == 2047 and {abs(int(x)).bit_length() for x in diffs} == set(range(12))
    m = len(dcs)
    add('DC categories', *([block(int(v)) for v in dcs] + [block(-int(v), [(1, 1)]) for v in dcs] + [block(int(v) - 1024) for v in dcs]), width=8 * m, height=8)
    add('DC +2047 from 0', block(2047), block(-2047), block(2047, [(63, 1)]))
    dense = [(k, 1023 if k % 2 else -1023) for k in range(1, 64)]
    add('AC +-1023 everywhere', block(0, dense), block(1, [(k, -v) for k, v in dense]), block(-1, dense))
    files = check(batch, names)
    assert files[z][huff_ref.HEADER:-2] == b'\x28\x03' and huff_ref.scan_bits(batch.coef(), batch.descs[z]) == 14


def test_saturated_blocks():
    """32 x 32 4:2:0, 24 blocks of the longest codes there are: 258 bytes per block, dense with stuffed bytes"""
    d, n = huff_ref.make_desc(32, 32, 2, 2, 100)
    coef = np.zeros(n, np.int16)
    for b in range(n // 64):
        for k in range(64):
            coef[b * 64 + k] = (1023 if (b + k) % 2 else -1023) if k else (-1024 if b % 2 == 0 else 1023)
    batch = Batch()
    batch.add(coef, 32, 32, 2, 2, 100)
    batch.add(np.zeros(192, np.int16))
    other = -coef
    other[0::64] = -coef[0::64] - 1                                   # (the DCs: -1024 <-> 1023)
    batch.add(other, 32, 32, 2, 2, 100)
    files = check(batch)
    assert n == 24 * 64 and len(files[0]) - huff_ref.HEADER - 2 == 6199
    assert huff_ref.scan_bits(batch.coef(), batch.descs[0]) == 37792


def test_seeded_family_in_one_batch():
    """320 three-block images in one launch: every padding length, scans that end in a stuffed byte, stuffed bytes in a row"""
    from ssd_tensorflow_amd import jpeg
    batch = Batch()
    for coef in huff_ref.family(320):
        batch.add(coef)
    want = batch.host_files()
    lengths = huff_ref.dht_lengths(want[0])
    coef = batch.coef()
    bits = [huff_ref.scan_bits(coef, d, lengths) for d in batch.descs]
    scans = [w[huff_ref.HEADER:-2] for w in want]
    for b, s in zip(bits, scans):
        assert (b + 7) // 8 + s.count(b'\xff\x00') == len(s)
    assert {b % 8 for b in bits} == set(range(8))
    assert any(s.endswith(b'\xff\x00') for s in scans) and any(b'\xff\x00\xff\x00' in s for s in scans)
    recs, files = Stage(batch).run()
    assert [r.status for r in recs] == [0] * 320
    assert files == want


# --------------------------------------------------------------------------------------------------------- 3. not codeable
def test_not_codeable_images_are_reported_and_spoil_only_themselves():
    from ssd_tensorflow_amd import jpeg
    rng = np.random.default_rng(2)
    d0, n = huff_ref.make_desc(40, 24, 2, 2)
    good = (rng.integers(-60, 61, n) * (rng.random(n) < 0.3)).astype(np.int16)
    batch = Batch()
    batch.add(good, 40, 24, 2, 2)
    for at, v in ((17 * 64 + 9, 1024), (3 * 64 + 63, -1024), (64 * (n // 64 - 1), None)):
        bad = good.copy()
        if v is None:                                                 # the last Cr block: a DC difference of -2048
            bad[at - 64], bad[at] = 1024, -1024
        else:
            bad[at] = v
        batch.add(bad, 40, 24, 2, 2)
    stage = Stage(batch)
    recs, files = stage.run()
    assert [r.status for r in recs] == [0, 2, 2, 1]
    coef = batch.coef()
    assert files[0] == jpeg.entropy_encode(coef, batch.descs[0])
    for i, text in ((1, 'AC coefficient 1024'), (2, 'AC coefficient -1024'), (3, 'DC difference -2048')):
        with pytest.raises(jpeg.JpegError, match=text):
            jpeg.entropy_encode(coef, batch.descs[i])
    again, files2 = stage.run()                                       # the same buffers, uncleared
    assert [r.status for r in again] == [0, 2, 2, 1] and files2[0] == files[0]
    # a 16-bit extreme is a status like any other
    worst = Batch()
    worst.add(np.full(192, -32768, np.int16))
    worst.add(np.zeros(192, np.int16))
    worst.add(np.concatenate([block(32767), block(-32768), block(0, [(63, 32767)])]))
    recs, files = Stage(worst).run()
    assert [r.status for r in recs] == [2, 0, 2] and files[1][huff_ref.HEADER:-2] == b'\x28\x03'


# ------------------------------------------------------------------------- 4. several workgroups per image, mixed sizes
def test_mixed_sizes_in_one_launch_and_an_unclean_workspace():
    from ssd_tensorflow_amd import jpeg
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'j1_jpeg.npz')) as z:
        voc = jpeg.decode(z['voc_000232_jpg'].tobytes())
    assert voc.shape == (375, 500, 3)
    rng = np.random.default_rng(5)
    strip_w, strip_h = rng.integers(0, 256, (1, 16384, 3)).astype(np.uint8), rng.integers(0, 256, (16384, 1, 3)).astype(np.uint8)
    dot = np.full((1, 1, 3), 200, np.uint8)
    y, x = np.mgrid[0:144, 0:144]
    smooth = np.stack([(x * 3 + y) % 256, (x + y * 2) % 256, (x * y // 64) % 256], 2).astype(np.uint8)
    batch, names = Batch(), []
    for name, pic, q, s in (('dot', dot, 95, '4:2:0'), ('144x144', smooth, 90, '4:4:4'), ('voc', voc, 95, '4:2:0'), ('dot 4:4:4', dot, 75, '4:4:4'),
                            ('16384x1', strip_w, 100, '4:2:2'), ('1x16384', strip_h, 100, '4:2:0'), ('noise', rng.integers(0, 256, (96, 144, 3)).astype(np.uint8), 100, '4:4:4'),
                            ('dot 4:2:2', dot, 1, '4:2:2')):
        names.append(name)
        batch.add_picture(pic, q, s)
    blocks = [d.mcus_x * d.mcus_y * (d.hs * d.vs + 2) for d in batch.descs]
    assert blocks[1] == 972 and blocks[2] == 4608
    want = batch.host_files()
    assert len(want[2]) == 87556
    stage = Stage(batch)
    recs, files = stage.run()
    for name, got, w in zip(names, files, want):
        assert got == w, name
    assert [r.offset for r in recs] == [sum((len(w) + 15) // 16 * 16 for w in want[:i]) for i in range(len(want))]
    recs2, files2 = stage.run()                                       # the workspace as the first launch left it
    assert files2 == files and [(r.offset, r.size) for r in recs2] == [(r.offset, r.size) for r in recs]
    stage.ws[:stage.ws_bytes].fill_(0xff)                             # (the guard behind it keeps its fill)
    assert stage.run()[1] == files


# ----------------------------------------------------------------------------------------------- 5. refusals before launch
def test_entry_point_refuses_before_it_launches():
    """every refused call below would stay inside the real buffers if it were launched: the declared sizes are what is wrong"""
    import torch
    from ssd_tensorflow_amd import jpeg, _lib
    batch = Batch()
    rng = np.random.default_rng(9)
    for w, h, hs, vs in ((40, 24, 2, 2), (8, 8, 1, 1), (33, 17, 2, 1)):
        n = huff_ref.make_desc(w, h, hs, vs)[1]
        batch.add((rng.integers(-30, 31, n) * (rng.random(n) < 0.3)).astype(np.int16), w, h, hs, vs)
    stage = Stage(batch)
    recs, good = stage.run()
    assert good == batch.host_files()
    stage.out.fill_(FILL)
    stage.recs.fill_(FILL)

    def descs(i, **kw):
        arr = (jpeg.Desc * stage.n)(*batch.descs)
        for k, v in kw.items():
            if k == 'coef_off':
                arr[i].coef_off[2] = v
            elif k == 'qt':
                arr[i].qt[0][5] = v
            else:
                setattr(arr[i], k, v)
        return arr

    for kw, text in ((dict(out_bytes=stage.out_bytes - 16), 'output buffer'), (dict(ws_bytes=stage.ws_bytes - 256), 'workspace'),
                     (dict(coef_bytes=stage.coef_bytes - 2), 'coefficient plane'), (dict(coef=stage.coef.data_ptr() + 2), 'aligned'),
                     (dict(out=stage.out.data_ptr() + 8), 'aligned'), (dict(ws=stage.ws.data_ptr() + 4), 'aligned'),
                     (dict(recs=stage.recs.data_ptr() + 8), 'aligned'), (dict(n=0), 'empty batch'), (dict(out=0), 'null'),
                     (dict(descs=descs(1, components=1)), 'components'), (dict(descs=descs(0, hs=1, vs=2)), 'sampling'),
                     (dict(descs=descs(2, qt=0)), 'quantiser'), (dict(descs=descs(0, mcus_x=2)), 'MCUs'), (dict(descs=descs(2, width=16385)), 'size'),
                     (dict(descs=descs(1, coef_off=int(batch.descs[1].coef_off[2]) + 4)), 'aligned'),
                     (dict(descs=descs(2, coef_off=int(batch.descs[2].coef_off[2]) + 64)), 'coefficient plane')):
        assert stage.call(**kw) != 0, kw
        assert re.search(text, _lib.last_error()), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((stage.out == FILL).all()) and bool((stage.recs == FILL).all())        # the refused calls wrote nothing
    assert stage.run()[1] == good


# ------------------------------------------------------------------------------------------------------------ 6. the drivers
def _child(args, seconds=600):
    r = subprocess.run([sys.executable, '-m'] + args, cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    assert r.returncode == 0, '%s\n%s\n%s' % (args, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def test_drivers_with_the_gpu_entropy_stage(g, tmp_path):
    """detect.py --encoder gpu --jpeg-entropy gpu writes the files of --jpeg-entropy host, and the same .txt files"""
    from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
    names = [str(n) for n in g['src_names']]
    picks = [j for j, n in enumerate(names) if n.endswith(('144x96', '104x88', '81x80', '95x65', '47x63'))][:5]
    assert len(picks) == 5
    files = []
    for k, j in enumerate(picks):
        files.append(str(tmp_path / (names[j] + ('.jpeg' if k == 1 else '.jpg'))))
        with open(files[-1], 'wb') as f:
            f.write(pillow_file(g, j, 95, '4:4:4'))
    model = str(tmp_path / 'model.npz')
    with Session(0) as sess:
        net = SSDVGG(sess, 'vgg300')
        net.build_from_vgg(None, 3, max_batch=4)
        net.build_optimizer()
        net.save_checkpoint(model, class_names=['class_%d' % i for i in range(3)])
    out = {}
    for ent in ('host', 'gpu'):
        out[ent] = str(tmp_path / ('detect_' + ent))
        _child(['ssd_tensorflow_amd.detect', '--model', model, '--output-dir', out[ent], '--batch-size', '4', '--encoder', 'gpu', '--jpeg-entropy', ent] + files)
    listing = sorted(os.listdir(out['gpu']))
    assert listing == sorted(os.listdir(out['host'])) and len(listing) == 10, listing
    assert sum(n.endswith(('.jpg', '.jpeg')) for n in listing) == 5 and sum(n.endswith('.txt') for n in listing) == 5
    match, mismatch, errors = filecmp.cmpfiles(out['gpu'], out['host'], listing, shallow=False)
    assert not mismatch and not errors and len(match) == 10, (mismatch, errors)
