"""What the quantised entry points of the C ABI refuse, and with which words: the five convolutions (fp8, fp8_bigk,
mxfp8, mxfp8_bigk, mxfp6), the three quantisers, the two filter quantisers and the three pools.  tests/golden/quant_refusals.json is
the table: for every call of _cases() below its return code and the complete ssd_last_error() text, recorded from the library as it stood BEFORE the
kernels under these entry points were merged (`python tests/test_quant_refusals.py` rewrites it from whatever library SSD_LIB
names).  A refusal happens on the host before any HIP call, so no GPU is needed.

Safety: a case the library wrongly accepted would launch a kernel.  The cases of NULL_CASES pass null for every pointer -- the shape
check precedes the pointer checks, so the worst outcome is a "null ..." refusal.  The cases of DUMMY_CASES need a non-null pointer
to reach their check (made-up addresses, never dereferenced on the host); they run only where no GPU is visible.

Not in the table: "a scale tensor of this layer exceeds the 32-bit offsets".  The check in front of it bounds B * H * W * C below
2^31 - 16, which bounds B * H * W * (C / 32) + 8 far below it: no shape reaches that text."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'quant_refusals.json')
P = 0x10000            # a made-up address, aligned to everything asked for
BF16, F32, E4M3, BF16_E4M3, MX, BF16_MX = range(6)


def _geom(**kw):
    g = dict(b=1, hi=8, wi=8, ci=64, ho=8, wo=8, co=64, kh=3, kw=3, stride=1, dil=1, pad_h=1, pad_w=1)
    g.update(kw)
    return [g[k] for k in ('b', 'hi', 'wi', 'ci', 'ho', 'wo', 'co', 'kh', 'kw', 'stride', 'dil', 'pad_h', 'pad_w')]


def _fp8(entry, mode=BF16, x=0, w=0, s_in=1.0, s_w=0, y=0, y8=0, s_out=1.0, **g):
    return ['ssd_op_conv2d_fwd_' + entry, x, w, s_in, s_w, 0, y, y8, mode, s_out] + _geom(**g) + [1, 0]


def _mx(entry, mode=BF16, x=0, xs=0, w=0, s_w=0, y=0, y8=0, ys=0, **g):      # (mxfp6: s_w is wscales)
    return ['ssd_op_conv2d_fwd_' + entry, x, xs, w, s_w, 0, y, y8, ys, mode] + _geom(**g) + [1, 0]


def _conv(entry, **kw):
    return (_fp8 if entry.startswith('fp8') else _mx)(entry, **kw)


def _pool(fmt, x=P, y=P, **kw):
    g = dict(b=1, hi=8, wi=8, c=64, ho=4, wo=4, k=2, stride=2, pad_h=0, pad_w=0)
    g.update(kw)
    ptrs = [x, y] if fmt == 'fp8' else [x, x and P, y, y and P]
    return ['ssd_op_maxpool_fwd_' + fmt] + ptrs + [g[k] for k in ('b', 'hi', 'wi', 'c', 'ho', 'wo', 'k', 'stride', 'pad_h', 'pad_w')] + [0]


def _cases():
    """name -> [entry point, arguments ...]; pointers are integers (0 = null)"""
    c = {}
    big = dict(kh=5, kw=5, pad_h=2, pad_w=2)
    for e in ('fp8', 'fp8_bigk', 'mxfp8', 'mxfp8_bigk', 'mxfp6'):
        k = big if e.endswith('bigk') else {}
        own8 = E4M3 if e.startswith('fp8') else MX
        c[e + ':ci96'] = _conv(e, ci=96, **k)
        c[e + ':ci32'] = _conv(e, ci=32, **k)
        c[e + ':co20'] = _conv(e, co=20, **k)
        c[e + ':taps25'] = _conv(e, **big)
        c[e + ':taps9'] = _conv(e)
        c[e + ':kh12'] = _conv(e, kh=12, kw=1)
        c[e + ':kh0'] = _conv(e, kh=0)
        c[e + ':stride0'] = _conv(e, stride=0, **k)
        c[e + ':dil0'] = _conv(e, dil=0, **k)
        c[e + ':b0'] = _conv(e, b=0, **k)
        c[e + ':tensor_2G'] = _conv(e, b=128, hi=512, wi=512, **k)
        c[e + ':output_2G'] = _conv(e, b=128, ho=512, wo=512, **k)
        c[e + ':filter_2G'] = _conv(e, ci=16384, co=16384, **k)
        c[e + ':mode7'] = _conv(e, mode=7, **k)
        c[e + ':mode_minus1'] = _conv(e, mode=-1, **k)
        c[e + ':other_formats_mode'] = _conv(e, mode=MX if e.startswith('fp8') else E4M3, **k)
        c[e + ':other_formats_mode_bf16'] = _conv(e, mode=BF16_MX if e.startswith('fp8') else BF16_E4M3, **k)
        c[e + ':mx_out_co40'] = _conv(e, mode=MX, co=40, **k)
        c[e + ':bf16_mx_out_co40'] = _conv(e, mode=BF16_MX, co=40, **k)
        c[e + ':null_output'] = _conv(e, **k)
        c[e + ':null_output_f32'] = _conv(e, mode=F32, **k)
        c[e + ':coded_out_without_buffers'] = _conv(e, mode=own8, **k)
        c[e + ':bf16_coded_out_without_buffers'] = _conv(e, mode=own8 + 1, **k)
        # ---- from here on a pointer is non-null
        c[e + ':null_operand'] = _conv(e, y=P, **k)
        c[e + ':null_operand_coded_out'] = _conv(e, mode=own8, y8=P, ys=P, **k) if own8 == MX else _conv(e, mode=own8, y8=P, **k)
        c[e + ':one_null_operand'] = _conv(e, y=P, x=P, w=P, **k)
    for e in ('fp8', 'fp8_bigk'):
        k = big if e.endswith('bigk') else {}
        c[e + ':s_in0'] = _conv(e, y=P, x=P, w=P, s_w=P, s_in=0.0, **k)
        c[e + ':s_out0'] = _conv(e, mode=E4M3, y8=P, s_out=0.0, **k)
        c[e + ':s_out0_bf16_e4m3'] = _conv(e, mode=BF16_E4M3, y=P, y8=P, s_out=0.0, **k)
    for e in ('mxfp8', 'mxfp8_bigk', 'mxfp6'):
        k = big if e.endswith('bigk') else {}
        c[e + ':mx_out_without_scales'] = _conv(e, mode=MX, y8=P, **k)
        c[e + ':odd_scale_address'] = _conv(e, y=P, x=P, xs=P + 1, w=P, s_w=P, **k)
    c['mxfp6:odd_filter_scale_address'] = _conv('mxfp6', y=P, x=P, xs=P, w=P, s_w=P + 1)
    c['mxfp6:codes_at_4'] = _conv('mxfp6', y=P, x=P + 4, xs=P, w=P, s_w=P)
    c['mxfp6:filter_codes_at_4'] = _conv('mxfp6', y=P, x=P, xs=P, w=P + 4, s_w=P)
    c['mxfp6:output_codes_at_4'] = _conv('mxfp6', mode=MX, y8=P + 4, ys=P, x=P, xs=P, w=P, s_w=P)

    # quantisers: x, x_f32, n, scale, y8, stream / x, x_f32, rows, c, y, ys, stream
    c['quantize_fp8:null'] = ['ssd_op_quantize_fp8', 0, 1, 64, 1.0, 0, 0]
    c['quantize_fp8:null_y'] = ['ssd_op_quantize_fp8', P, 1, 64, 1.0, 0, 0]
    c['quantize_fp8:scale0'] = ['ssd_op_quantize_fp8', P, 1, 64, 0.0, P, 0]
    c['quantize_fp8:n0'] = ['ssd_op_quantize_fp8', P, 0, 0, 1.0, P, 0]
    for f in ('mxfp8', 'mxfp6'):
        q = 'ssd_op_quantize_' + f
        c['quantize_%s:null' % f] = [q, 0, 1, 4, 64, 0, 0, 0]
        c['quantize_%s:null_scales' % f] = [q, P, 1, 4, 64, P, 0, 0]
        c['quantize_%s:c24' % f] = [q, P, 1, 4, 24, P, P, 0]
        c['quantize_%s:c0' % f] = [q, P, 0, 4, 0, P, P, 0]
        c['quantize_%s:c_minus32' % f] = [q, P, 0, 4, -32, P, P, 0]
        c['quantize_%s:x_at_8' % f] = [q, P + 8, 0, 4, 64, P, P, 0]
        c['quantize_%s:y_at_4' % f] = [q, P, 1, 4, 64, P + 4, P, 0]
        c['quantize_%s:rows0' % f] = [q, P, 1, 0, 64, P, P, 0]
    # filter quantisers: w, w8 / w6, s_w / wscales, taps, ci, co, stream
    for f in ('fp8', 'mxfp6'):
        q = 'ssd_op_quantize_filter_' + f
        c['quantize_filter_%s:null' % f] = [q, 0, 0, 0, 9, 64, 64, 0]
        c['quantize_filter_%s:taps0' % f] = [q, P, P, P, 0, 64, 64, 0]
        c['quantize_filter_%s:co0' % f] = [q, P, P, P, 9, 64, 0, 0]
    c['quantize_filter_mxfp6:ci48'] = ['ssd_op_quantize_filter_mxfp6', P, P, P, 9, 48, 64, 0]
    c['quantize_filter_mxfp6:ci16'] = ['ssd_op_quantize_filter_mxfp6', P, P, P, 9, 16, 64, 0]
    c['quantize_filter_mxfp6:codes_at_4'] = ['ssd_op_quantize_filter_mxfp6', P, P + 4, P, 9, 64, 64, 0]
    # pools
    for f in ('fp8', 'mxfp8', 'mxfp6'):
        p = 'maxpool_%s:' % f
        c[p + 'null'] = _pool(f, x=0, y=0)
        c[p + 'null_y'] = _pool(f, y=0)
        c[p + 'c24'] = _pool(f, c=24)
        c[p + 'c16'] = _pool(f, c=16, k=0)      # (accepted by the e4m3 pool: k = 0 stops it there)
        c[p + 'c0'] = _pool(f, c=0)
        c[p + 'k0'] = _pool(f, k=0)
        c[p + 'stride0'] = _pool(f, stride=0)
        c[p + 'b0'] = _pool(f, b=0)
        c[p + 'wo0'] = _pool(f, wo=0)
        c[p + 'pad_is_k'] = _pool(f, pad_h=2)
        c[p + 'window_below_image'] = _pool(f, ho=6)
        c[p + 'window_right_of_image'] = _pool(f, wo=5)
        if f != 'fp8':
            c[p + 'x_at_4'] = _pool(f, x=P + 4)
            c[p + 'y_at_4'] = _pool(f, y=P + 4)
    return c


def _is_pointer(fn, i):
    from ssd_tensorflow_amd._lib import SIGNATURES, vp
    return SIGNATURES[fn][1][i] is vp


def _needs_dummy(call):
    return any(_is_pointer(call[0], i) and a for i, a in enumerate(call[1:]))


def _run(call):
    from ssd_tensorflow_amd._lib import lib, last_error
    rc = getattr(lib, call[0])(*[(a or None) if _is_pointer(call[0], i) else a for i, a in enumerate(call[1:])])
    return {'rc': rc, 'error': last_error() if rc != 0 else None}


def _gpu_visible():
    import torch
    return torch.cuda.device_count() > 0


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_table_is_the_table_of_this_file():
    g = _golden()
    assert sorted(g) == sorted(_cases())
    texts = {v['error'] for v in g.values()}
    assert len(g) > 200 and len(texts) > 60 and sum(v['rc'] == 0 for v in g.values()) == 3      # n = 0 and rows = 0 twice


def test_refusals_with_null_pointers():
    g, c = _golden(), _cases()
    names = [k for k in c if not _needs_dummy(c[k])]
    assert len(names) > 120
    for k in names:
        assert _run(c[k]) == g[k], k


def test_refusals_behind_the_pointer_checks():
    if _gpu_visible():
        pytest.skip('made-up addresses: only where a wrongly accepted call cannot launch')
    g, c = _golden(), _cases()
    names = [k for k in c if _needs_dummy(c[k])]
    assert len(names) > 80
    for k in names:
        assert _run(c[k]) == g[k], k


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert not _gpu_visible(), 'record where no GPU is visible'
    table = {k: _run(v) for k, v in _cases().items()}
    with open(GOLDEN, 'w') as f:
        f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(table[k], sort_keys=True)) for k in sorted(table)) + '\n}\n')
    print(len(table), 'calls,', len({v['error'] for v in table.values()}), 'distinct texts ->', GOLDEN)
