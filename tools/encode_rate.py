#!/usr/bin/env python3
"""Measures the two ways from uint8 BGR pixels on the GPU to JPEG files' bytes, in one process, interleaved rounds:

  (a) today's path: one device-to-host copy of the pixels per batch + Image.save(quality=95) per picture (Pillow, 4:2:0)
  (b) jpeg.encode_batch with threads = 1, 4, 8, 16: DCT and quantisation on the GPU, Huffman coding on host threads
  (c) jpeg.encode_batch(entropy='gpu'): Huffman coding and the file framing on the GPU as well

on N device-resident pictures of VOC shape: the 500 x 375 fixture picture shifted by a different offset each.  Per path: images/s
by wall clock, CPU seconds per image (time.process_time: all threads of the process), device-to-host bytes per image; the two
device stages alone from events on the stream, with the bytes they must move.  With --detect: detect.py end to end with both
encoders and both entropy settings instead (child processes; batch 32, bf16, .jpg outputs).

    python tools/encode_rate.py [--files 512] [--rounds 5] [--batch 32] [--out profiles/jpeg_encode_rate.txt] [--detect]
"""
import argparse
import io
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_pictures(n):
    """n uint8 [375, 500, 3] BGR pictures"""
    from ssd_tensorflow_amd import jpeg
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'j1_jpeg.npz')) as g:
        data = g['voc_000232_jpg'].tobytes()
    st, d, coef = jpeg.entropy_decode(data)
    assert st == jpeg.OK
    bgr = jpeg.decode(data)
    big = np.pad(bgr, ((0, 32), (0, 32), (0, 0)), mode='reflect')
    return [np.ascontiguousarray(big[(i // 32) % 32:(i // 32) % 32 + 375, i % 32:i % 32 + 500]) for i in range(n)]


def upload(pics, batch, dev):
    """[(device tensor, offsets, shapes)] per batch"""
    import torch
    from ssd_tensorflow_amd.annotate import pack_offsets
    out = []
    for o in range(0, len(pics), batch):
        part = pics[o:o + batch]
        shapes = [p.shape[:2] for p in part]
        offs, total = pack_offsets(shapes, 1)
        host = np.zeros(total, np.uint8)
        for p, off in zip(part, offs):
            host[off:off + p.size] = p.reshape(-1)
        out.append((torch.from_numpy(host).to(dev), offs, shapes))
    return out


def pillow_path(batches):
    import torch
    from PIL import Image
    from ssd_tensorflow_amd.annotate import unpack
    size = 0
    for src, offs, shapes in batches:
        host = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
        host.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        for img in unpack(host.numpy(), offs, shapes):
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(buf, 'JPEG', quality=95)
            size += buf.tell()
    return size


def gpu_path(batches, threads, entropy='host', copied=None):
    """copied: a one-element list that receives the bytes entropy='gpu' brings to the host (the records and the files, each but a
    batch's last rounded up to 16), from the returned sizes"""
    from ssd_tensorflow_amd import jpeg
    size = 0
    for src, offs, shapes in batches:
        files = jpeg.encode_batch(src, offs, shapes, threads=threads, entropy=entropy)
        size += sum(len(f) for f in files)
        if copied is not None:
            copied[0] += 24 * len(files) + sum((len(f) + 15) // 16 * 16 for f in files[:-1]) + len(files[-1])
    return size


def kernel_time(pics, batch, dev, reps=20):
    """(median ms, min ms, bytes moved) of the device stage for one batch"""
    import ctypes as C
    import torch
    from ssd_tensorflow_amd import jpeg
    from ssd_tensorflow_amd._lib import lib, last_error
    pics = (pics * (batch // len(pics) + 1))[:batch]
    src, offs, shapes = upload(pics, batch, dev)[0]
    n = len(pics)
    shp = (C.c_int * (2 * n))(*[int(v) for hw in shapes for v in hw])
    so = (C.c_ulonglong * n)(*offs)
    coef_bytes, ws_bytes = lib.ssd_jpeg_enc_coef_bytes(shp, n, 0x22), lib.ssd_jpeg_enc_ws_bytes(shp, n, 0x22)
    coef = torch.empty((coef_bytes // 2,), dtype=torch.int16, device=dev)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    descs = (jpeg.Desc * n)()
    s = torch.cuda.current_stream(dev).cuda_stream
    times = []
    for r in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if lib.ssd_jpeg_encode_batch_dev(src.data_ptr(), src.numel(), so, shp, n, 95, 0x22, coef.data_ptr(), coef_bytes, descs, ws.data_ptr(), ws_bytes, s):
            raise RuntimeError(last_error())
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            times.append(e0.elapsed_time(e1))
    moved = sum(p.size for p in pics) + coef_bytes                      # pixels read once (3 B), coefficients written (2 B each)
    return statistics.median(times), min(times), moved


def huffman_time(pics, batch, dev, reps=20):
    """(median ms, min ms, bytes moved) of the Huffman stage (seven launches, descriptor copy included) for one batch"""
    import ctypes as C
    import torch
    from ssd_tensorflow_amd import jpeg
    from ssd_tensorflow_amd._lib import lib, last_error
    pics = (pics * (batch // len(pics) + 1))[:batch]
    src, offs, shapes = upload(pics, batch, dev)[0]
    n = len(pics)
    shp = (C.c_int * (2 * n))(*[int(v) for hw in shapes for v in hw])
    so = (C.c_ulonglong * n)(*offs)
    coef_bytes, ws_bytes = lib.ssd_jpeg_enc_coef_bytes(shp, n, 0x22), lib.ssd_jpeg_enc_ws_bytes(shp, n, 0x22)
    coef = torch.empty((coef_bytes // 2,), dtype=torch.int16, device=dev)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    descs = (jpeg.Desc * n)()
    s = torch.cuda.current_stream(dev).cuda_stream
    if lib.ssd_jpeg_encode_batch_dev(src.data_ptr(), src.numel(), so, shp, n, 95, 0x22, coef.data_ptr(), coef_bytes, descs, ws.data_ptr(), ws_bytes, s):
        raise RuntimeError(last_error())
    hws_bytes, out_bytes = lib.ssd_jpeg_huff_ws_bytes(descs, n), lib.ssd_jpeg_huff_out_bytes(descs, n)
    hws = torch.empty((hws_bytes,), dtype=torch.uint8, device=dev)
    out = torch.empty((out_bytes,), dtype=torch.uint8, device=dev)
    recs = torch.empty((n * C.sizeof(jpeg.FileRec),), dtype=torch.uint8, device=dev)
    times = []
    for r in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if lib.ssd_jpeg_huffman_batch_dev(coef.data_ptr(), coef_bytes, descs, n, out.data_ptr(), out_bytes, recs.data_ptr(), hws.data_ptr(), hws_bytes, s):
            raise RuntimeError(last_error())
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            times.append(e0.elapsed_time(e1))
    host = (jpeg.FileRec * n).from_buffer_copy(recs.cpu().numpy().tobytes())
    files = sum(int(r.size) for r in host)
    # coefficients read by count and by emit; the unstuffed stream (at most the files' bytes) written once and read by the FF count
    # and by the writer; the files written
    moved = 2 * coef_bytes + 3 * files + files
    return statistics.median(times), min(times), moved, files


def detect_rate(files, encoder, model, outdir, entropy='host'):
    def run(part, tag):
        t0 = time.perf_counter()
        subprocess.run([sys.executable, '-m', 'ssd_tensorflow_amd.detect', '--model', model, '--output-dir', os.path.join(outdir, encoder + entropy + tag),
                        '--batch-size', '32', '--dtype', 'bf16', '--encoder', encoder, '--jpeg-entropy', entropy] + part, cwd=ROOT, check=True, timeout=900,
                       stdout=subprocess.DEVNULL)
        return time.perf_counter() - t0
    small, full = run(files[:32], '_32'), run(files * 4, '_all')      # (each file four times: a window of seconds, not of one)
    return (4 * len(files) - 32) / (full - small), small, full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out', default=None)
    ap.add_argument('--detect', action='store_true', help='measure detect.py end to end instead (appends to --out)')
    args = ap.parse_args()
    import torch
    dev = torch.device('cuda', 0)
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    pics = make_pictures(args.files)
    n = len(pics)
    if not args.detect:
        batches = upload(pics, args.batch, dev)
        say('# tools/encode_rate.py: %d device-resident pictures of 500 x 375, quality 95, 4:2:0, batches of %d, %d interleaved rounds, %s'
            % (n, args.batch, args.rounds, torch.cuda.get_device_name(0)))
        paths = [('host: copy of the pixels + Image.save per picture', lambda: pillow_path(batches))]
        for t in (1, 4, 8, 16):
            paths.append(('gpu:  jpeg.encode_batch threads=%d' % t, lambda t=t: gpu_path(batches, t)))
        copied = [0]
        paths.append(("gpu:  jpeg.encode_batch entropy='gpu'", lambda: gpu_path(batches, None, 'gpu')))
        sizes = [fn() for _, fn in paths[:2]] + [gpu_path(batches, None, 'gpu', copied)]   # warm-up: allocator, pinned pool, code objects
        assert sizes[0] == sizes[1] == sizes[2], sizes                 # (the same files)
        coef_per_image = ((375 + 15) // 16) * ((500 + 15) // 16) * 6 * 128   # 4:2:0: MCUs of six [64] int16 blocks
        d2h = {name: coef_per_image for name, _ in paths}
        d2h[paths[0][0]] = 500 * 375 * 3
        d2h[paths[-1][0]] = copied[0] / n
        wall = {name: [] for name, _ in paths}
        cpu = {name: [] for name, _ in paths}
        for r in range(args.rounds):
            for name, fn in paths:
                c0, t0 = time.process_time(), time.perf_counter()
                fn()
                wall[name].append((time.perf_counter() - t0) / n)
                cpu[name].append((time.process_time() - c0) / n)
        say('# files of %.1f KB each, the same bytes on both paths' % (sizes[0] / n / 1e3))
        say('# %-52s %10s %22s %24s %16s' % ('path', 'images/s', 'wall ms/image (min..max)', 'CPU ms/image (min..max)', 'D2H bytes/image'))
        for name, _ in paths:
            w, c = wall[name], cpu[name]
            say('  %-52s %10.0f %9.3f (%.3f..%.3f) %11.3f (%.3f..%.3f) %16.0f' % (name, 1 / statistics.median(w), statistics.median(w) * 1e3, min(w) * 1e3,
                                                                             max(w) * 1e3, statistics.median(c) * 1e3, min(c) * 1e3, max(c) * 1e3, d2h[name]))
        a, b = paths[0][0], paths[1][0]
        say('# CPU seconds per image, gpu threads=1 / host: %.3f (per round: %s)'
            % (statistics.median(cpu[b]) / statistics.median(cpu[a]), ' '.join('%.3f' % (x / y) for x, y in zip(cpu[b], cpu[a]))))
        for k in (args.batch, 4 * args.batch):
            ms, ms_min, moved = kernel_time(pics, k, dev)
            say('# device stage (jpeg_fdct, descriptor copy included, batch of %d): median %.3f ms, min %.3f ms = %.2f us/image; %.1f MB to move -> %.0f GB/s'
                % (k, ms, ms_min, ms / k * 1e3, moved / 1e6, moved / ms / 1e6))
            ms, ms_min, moved, files = huffman_time(pics, k, dev)
            say('# Huffman stage (7 launches, descriptor copy included, batch of %d): median %.3f ms, min %.3f ms = %.2f us/image; files of %.1f MB, %.1f MB to move -> %.0f GB/s'
                % (k, ms, ms_min, ms / k * 1e3, files / 1e6, moved / 1e6, moved / ms / 1e6))
    else:
        from ssd_tensorflow_amd import jpeg
        from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
        with tempfile.TemporaryDirectory() as tmp:
            files = []
            for o in range(0, n, args.batch):
                for k, data in enumerate(jpeg.encode_batch(pics[o:o + args.batch], quality=90)):
                    files.append(os.path.join(tmp, '%06d.jpg' % (o + k)))
                    with open(files[-1], 'wb') as f:
                        f.write(data)
            model = os.path.join(tmp, 'model.npz')
            with Session(0) as sess:
                net = SSDVGG(sess, 'vgg300')
                net.build_from_vgg(None, 20, max_batch=32)
                net.build_optimizer()
                net.save_checkpoint(model)
            for enc, ent in (('pillow', 'host'), ('gpu', 'host'), ('gpu', 'gpu')) * 2:
                rate, small, full = detect_rate(files, enc, model, tmp, ent)
                say('  detect.py --encoder %-6s --jpeg-entropy %-4s --dtype bf16 --batch-size 32 (.jpg outputs): %6.0f images/s (%d files %.1f s, 32 files %.1f s)'
                    % (enc, ent, rate, 4 * n, full, small))
    if args.out:
        with open(args.out, 'a' if args.detect else 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
