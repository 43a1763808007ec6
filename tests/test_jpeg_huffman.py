"""CPU: the host side of the Huffman stage on the GPU (csrc/jpeg_huff.hip): the shared header writer, the size
functions' refusals, and the bit counter tests/huff_ref.py against the host stage.  Everything is exact."""
import ctypes as C

import numpy as np
import pytest

import huff_ref


def test_file_header_is_the_front_of_the_host_stages_file():
    from ssd_tensorflow_amd import jpeg
    for hs, vs in ((1, 1), (2, 1), (2, 2)):
        for q in (1, 95, 100):
            d, n = huff_ref.make_desc(37, 21, hs, vs, q)
            data = jpeg.entropy_encode(np.zeros(n, np.int16), d)
            head = jpeg.file_header(d)
            assert len(head) == huff_ref.HEADER and data[:huff_ref.HEADER] == head, (hs, vs, q)
            assert head[-14:-12] == b'\xff\xda' and data[-2:] == b'\xff\xd9'
    d, n = huff_ref.make_desc(37, 21, 1, 2)
    with pytest.raises(jpeg.JpegError, match='sampling'):
        jpeg.file_header(d)


def test_size_functions_refuse_bad_descriptors_and_grow_with_the_blocks():
    from ssd_tensorflow_amd import jpeg
    from ssd_tensorflow_amd._lib import lib, last_error

    def sizes(descs, n=None):
        arr = (jpeg.Desc * len(descs))(*descs)
        return lib.ssd_jpeg_huff_ws_bytes(arr, len(descs) if n is None else n), lib.ssd_jpeg_huff_out_bytes(arr, len(descs) if n is None else n)

    good = [huff_ref.make_desc(8, 8)[0], huff_ref.make_desc(500, 375, 2, 2)[0]]
    ws, out = sizes(good)
    assert ws > 0 and out == sum((lib.ssd_jpeg_file_bound(C.byref(d)) + 15) // 16 * 16 for d in good)
    last = (ws, out)
    for side in (16, 64, 144, 1000):
        now = sizes([huff_ref.make_desc(side, side)[0]] + good)
        assert now[0] > last[0] and now[1] > last[1], side
        last = now
    assert sizes(good + good)[1] == 2 * out

    def broken(**kw):
        d = huff_ref.make_desc(40, 24, 2, 2)[0]
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    zero_q = broken()
    zero_q.qt[1][7] = zero_q.qt[2][7] = 0
    for descs, n, text in (([good[0]], 0, 'empty batch'), ([good[0], broken(components=1)], None, 'components'), ([broken(hs=1, vs=2, mcus_x=5, mcus_y=2)], None, 'sampling'),
                           ([zero_q], None, 'quantiser'), ([good[1], broken(mcus_x=4)], None, 'MCUs'), ([broken(mcus_y=1)], None, 'MCUs'),
                           ([broken(width=0)], None, 'size')):
        assert sizes(descs, n) == (0, 0), text
        assert text in last_error(), (text, last_error())
    assert sizes(good) == (ws, out)


def test_scan_bits_against_the_host_stage():
    """ceil(bits / 8) + count(FF 00) == len(scan) on the seeded family; the family holds what the GPU test relies on"""
    from ssd_tensorflow_amd import jpeg
    d, n = huff_ref.make_desc(8, 8)
    lengths = None
    residues, ends, doubles = set(), 0, 0
    for coef in huff_ref.family(1000):
        data = jpeg.entropy_encode(coef, d)
        lengths = lengths or huff_ref.dht_lengths(data)
        scan = data[huff_ref.HEADER:-2]
        bits = huff_ref.scan_bits(coef, d, lengths)
        assert (bits + 7) // 8 + scan.count(b'\xff\x00') == len(scan)
        assert b'\xff' not in scan.replace(b'\xff\x00', b'')
        residues.add(bits % 8)
        ends += scan.endswith(b'\xff\x00')
        doubles += b'\xff\x00\xff\x00' in scan
    assert residues == set(range(8)) and ends > 0 and doubles > 0
    assert sorted(lengths) == [0x00, 0x01, 0x10, 0x11] and [len(lengths[k]) for k in sorted(lengths)] == [12, 12, 162, 162]
    # larger layouts: interleaving and DC prediction across MCUs
    rng = np.random.default_rng(3)
    for hs, vs in ((1, 1), (2, 1), (2, 2)):
        d, n = huff_ref.make_desc(40, 24, hs, vs)
        coef = (rng.integers(-40, 41, n) * (rng.random(n) < 0.2)).astype(np.int16)
        scan = jpeg.entropy_encode(coef, d)[huff_ref.HEADER:-2]
        assert (huff_ref.scan_bits(coef, d) + 7) // 8 + scan.count(b'\xff\x00') == len(scan)
    # an all-zero 8 x 8 4:4:4 image: three DC codes of category 0 and three EOBs, 14 bits
    d, n = huff_ref.make_desc(8, 8)
    assert huff_ref.scan_bits(np.zeros(n, np.int16), d) == 14 and jpeg.entropy_encode(np.zeros(n, np.int16), d)[huff_ref.HEADER:-2] == b'\x28\x03'
