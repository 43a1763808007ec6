#!/usr/bin/env python3
"""Measures the two ways from JPEG files to uint8 BGR pixels on the GPU, in one process, interleaved rounds:

  (a) the host path: transforms.load_image_bgr (Pillow) per file + plan_params packing + one upload per batch
  (b) jpeg.decode_batch with threads = 1, 4, 8, 16: Huffman decoding on the host, the rest on the GPU

on N files of VOC shape: the 500 x 375 fixture picture, shifted by a different offset each and re-encoded by Pillow at quality 90,
4:2:0.  Per path: images/s by wall clock, CPU seconds per image (time.process_time: all threads of the process), host-to-device
bytes per image; for (b) also the two decode kernels' time per image from events on the stream, with the bytes they must move.
Then detect.py end to end with both decoders (child processes; batch 32, bf16).

--entropy-gpu adds (c) jpeg.decode_batch(entropy='gpu'), the Huffman stage on the GPU too, beside the rows above in
the same rounds, the Huffman launches alone from stream events, and detect.py --decoder-entropy host / gpu alternating.

    python tools/decode_rate.py [--files 512] [--rounds 5] [--batch 32] [--out profiles/jpeg_decode_rate.txt] [--no-detect]
    python tools/decode_rate.py --entropy-gpu --out profiles/jpeg_huffdec_rate.txt
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


def make_files(directory, n):
    from PIL import Image
    from ssd_tensorflow_amd import transforms as T
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'j1_jpeg.npz')) as g:
        data = g['voc_000232_jpg'].tobytes()
    with Image.open(io.BytesIO(data)) as im:
        rgb = np.asarray(im.convert('RGB'))
    big = np.pad(rgb, ((0, 32), (0, 32), (0, 0)), mode='reflect')
    files = []
    for i in range(n):
        y, x = (i // 32) % 32, i % 32
        path = os.path.join(directory, '%06d.jpg' % i)
        Image.fromarray(big[y:y + 375, x:x + 500]).save(path, 'JPEG', quality=90, subsampling=2)
        files.append(path)
    assert T.load_image_bgr(files[0]).shape == (375, 500, 3)
    return files


def host_path(files, batch, dev):
    import torch
    from ssd_tensorflow_amd import transforms as T
    h2d = 0
    for o in range(0, len(files), batch):
        plans = []
        for f in files[o:o + batch]:
            p = T.ImagePlan(T.load_image_bgr(f))
            p.resize = (300, 300, T.INTER_LINEAR)
            plans.append(p)
        _, packed = T.plan_params(plans, 300, 300)
        torch.from_numpy(packed).to(dev)
        h2d += packed.nbytes
    torch.cuda.synchronize()
    return h2d


def gpu_path(files, batch, threads, entropy='host'):
    import torch
    from ssd_tensorflow_amd import jpeg
    for o in range(0, len(files), batch):
        _, _, _, fallbacks = jpeg.decode_batch(files[o:o + batch], threads=threads, entropy=entropy)
        assert fallbacks == []
    torch.cuda.synchronize()
    return 0


def kernel_time(files, batch, dev, reps=20):
    """(median ms per batch of the two decode launches, bytes they must move, host-to-device bytes) for one batch"""
    import torch
    from ssd_tensorflow_amd import jpeg
    from ssd_tensorflow_amd._lib import lib, last_error
    datas = [open(f, 'rb').read() for f in files[:batch]]
    coef, offs, descs, status, _ = jpeg.entropy_decode_batch(datas, threads=8)
    assert status == [jpeg.OK] * len(datas)
    off, pixels = 0, 0
    for d in descs:
        d.dst_off = off
        off += (d.width * d.height * 3 + 15) // 16 * 16
        pixels += d.width * d.height
    coef_dev = torch.from_numpy(coef).to(dev)
    dst = torch.empty((off,), dtype=torch.uint8, device=dev)
    ws_bytes = lib.ssd_jpeg_ws_bytes(descs, len(datas))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    times = []
    for r in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if lib.ssd_jpeg_decode_batch_dev(coef_dev.data_ptr(), coef.nbytes, descs, len(datas), dst.data_ptr(), off, ws.data_ptr(), ws_bytes, s):
            raise RuntimeError(last_error())
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            times.append(e0.elapsed_time(e1))
    # coefficients read (2 B each), planes written and read (1 B per coefficient each), pixels written (3 B)
    moved = coef.nbytes + 2 * (coef.nbytes // 2) + 3 * pixels
    return statistics.median(times), min(times), moved, coef.nbytes


def huffdec_time(files, batch, dev, reps=20):
    """(median, min ms per batch of the Huffman launches with their descriptor copy, file bytes, coefficient bytes) for one batch"""
    import ctypes as C
    import torch
    from ssd_tensorflow_amd import jpeg
    from ssd_tensorflow_amd._lib import lib, last_error
    datas = [open(f, 'rb').read() for f in files[:batch]]
    n = len(datas)
    plans, descs, keep = (jpeg.Plan * n)(), (jpeg.Desc * n)(), []
    fbytes = cbytes = 0
    for k, data in enumerate(datas):
        st, d, plan = jpeg.scan_plan(data, plans[k])
        assert st == jpeg.OK
        keep.append(plan._segs)
        C.memmove(C.byref(descs[k]), C.byref(d), C.sizeof(jpeg.Desc))
        plans[k].file_off = fbytes
        fbytes += (len(data) + 15) // 16 * 16
        for c in range(3):
            descs[k].coef_off[c] += cbytes // 2
        cbytes += lib.ssd_jpeg_coef_bytes(data, len(data))
    host = np.zeros(fbytes, np.uint8)
    for k, data in enumerate(datas):
        host[plans[k].file_off:plans[k].file_off + len(data)] = np.frombuffer(data, np.uint8)
    files_dev = torch.from_numpy(host).to(dev)
    coef = torch.empty((cbytes // 2,), dtype=torch.int16, device=dev)
    recs = torch.empty((2 * n,), dtype=torch.int32, device=dev)
    ws_bytes = lib.ssd_jpeg_huffdec_ws_bytes(plans, descs, n)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    times = []
    for r in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if lib.ssd_jpeg_huffdec_batch_dev(files_dev.data_ptr(), fbytes, plans, descs, n, coef.data_ptr(), cbytes, recs.data_ptr(), ws.data_ptr(),
                                          ws_bytes, 0, s):
            raise RuntimeError(last_error())
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            times.append(e0.elapsed_time(e1))
    assert recs.cpu().numpy().reshape(n, 2)[:, 0].tolist() == [jpeg.OK] * n
    return statistics.median(times), min(times), fbytes, cbytes


def detect_rate(files, decoder, model, outdir, entropy='host'):
    def run(part, tag):
        t0 = time.perf_counter()
        subprocess.run([sys.executable, '-m', 'ssd_tensorflow_amd.detect', '--model', model, '--output-dir', os.path.join(outdir, decoder + entropy + tag),
                        '--batch-size', '32', '--dtype', 'bf16', '--decoder', decoder, '--decoder-entropy', entropy] + part, cwd=ROOT, check=True,
                       timeout=900, stdout=subprocess.DEVNULL)
        return time.perf_counter() - t0
    small, full = run(files[:32], '_32'), run(files * 4, '_all')      # (each file four times: a window of seconds, not of one)
    return (4 * len(files) - 32) / (full - small), small, full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-detect', action='store_true')
    ap.add_argument('--entropy-gpu', action='store_true', help="also measure decode_batch(entropy='gpu') and detect.py --decoder-entropy gpu")
    args = ap.parse_args()
    import torch
    dev = torch.device('cuda', 0)
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as tmp:
        files = make_files(tmp, args.files)
        n = len(files)
        say('# tools/decode_rate.py: %d files of 500 x 375, quality 90, 4:2:0 (%.1f KB each), batches of %d, %d interleaved rounds, %s'
            % (n, sum(os.path.getsize(f) for f in files) / n / 1e3, args.batch, args.rounds, torch.cuda.get_device_name(0)))
        paths = [('host: load_image_bgr + plan_params + upload', lambda: host_path(files, args.batch, dev))]
        for t in (1, 4, 8, 16):
            paths.append(('gpu:  jpeg.decode_batch threads=%d' % t, lambda t=t: gpu_path(files, args.batch, t)))
        if args.entropy_gpu:
            paths.append(("gpu:  jpeg.decode_batch entropy='gpu'", lambda: gpu_path(files, args.batch, None, 'gpu')))
        for _, fn in paths[:2] + paths[6:]:
            fn()                                                       # warm-up: allocator, pinned pool, code objects
        wall = {name: [] for name, _ in paths}
        cpu = {name: [] for name, _ in paths}
        h2d_host = 0
        for r in range(args.rounds):
            for name, fn in paths:
                c0, t0 = time.process_time(), time.perf_counter()
                moved = fn()
                wall[name].append((time.perf_counter() - t0) / n)
                cpu[name].append((time.process_time() - c0) / n)
                h2d_host = moved or h2d_host
        ms, ms_min, moved, coef_bytes = kernel_time(files, args.batch, dev)
        big = kernel_time(files, 4 * args.batch, dev)
        say('# %-46s %10s %22s %24s' % ('path', 'images/s', 'wall ms/image (min..max)', 'CPU ms/image (min..max)'))
        for name, _ in paths:
            w, c = wall[name], cpu[name]
            say('  %-46s %10.0f %9.3f (%.3f..%.3f) %11.3f (%.3f..%.3f)' % (name, 1 / statistics.median(w), statistics.median(w) * 1e3, min(w) * 1e3,
                                                                       max(w) * 1e3, statistics.median(c) * 1e3, min(c) * 1e3, max(c) * 1e3))
        base = statistics.median(cpu[paths[0][0]])
        one = statistics.median(cpu[paths[1][0]])
        say('# CPU seconds per image, gpu threads=1 / host: %.3f (per round: %s)'
            % (one / base, ' '.join('%.3f' % (a / b) for a, b in zip(cpu[paths[1][0]], cpu[paths[0][0]]))))
        say('# host-to-device bytes per image: host %.0f, gpu %.0f (int16 coefficients of whole MCUs)' % (h2d_host / n, coef_bytes / args.batch))
        say('# decode kernels (jpeg_idct + jpeg_pack, batch of %d): median %.3f ms, min %.3f ms = %.2f us/image; %.1f MB to move -> %.0f GB/s'
            % (args.batch, ms, ms_min, ms / args.batch * 1e3, moved / 1e6, moved / ms / 1e6))
        say('# the same for a batch of %d: median %.3f ms = %.2f us/image; %.1f MB -> %.0f GB/s'
            % (4 * args.batch, big[0], big[0] / (4 * args.batch) * 1e3, big[2] / 1e6, big[2] / big[0] / 1e6))
        if args.entropy_gpu:
            name = paths[-1][0]
            for ref in (paths[1][0], paths[3][0]):
                say("# entropy='gpu' / %s: CPU per image %.3f, wall per image %.3f" % (ref.split('decode_batch ')[1], statistics.median(cpu[name]) /
                    statistics.median(cpu[ref]), statistics.median(wall[name]) / statistics.median(wall[ref])))
            for b in (args.batch, 4 * args.batch):
                med, low, fbytes, cbytes = huffdec_time(files, b, dev)
                say('# Huffman stage on the GPU (9 launches + descriptor copy, batch of %d): median %.3f ms, min %.3f ms = %.2f us/image; %.1f MB of files '
                    'in, %.1f MB of coefficients out' % (b, med, low, med / b * 1e3, fbytes / 1e6, cbytes / 1e6))
            say("# host-to-device bytes per image with entropy='gpu': %.0f (the file, rounded up to 16; plus the plan tables in the workspace)" % (fbytes / b))
        if not args.no_detect and args.entropy_gpu:
            from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
            model = os.path.join(tmp, 'model.npz')
            with Session(0) as sess:
                net = SSDVGG(sess, 'vgg300')
                net.build_from_vgg(None, 20, max_batch=32)
                net.build_optimizer()
                net.save_checkpoint(model)
            for ent in ('host', 'gpu', 'host', 'gpu'):
                rate, small, full = detect_rate(files, 'gpu', model, tmp, ent)
                say('  detect.py --decoder gpu --decoder-entropy %-4s --dtype bf16 --batch-size 32: %6.0f images/s (%d files %.1f s, 32 files %.1f s)'
                    % (ent, rate, 4 * n, full, small))
        elif not args.no_detect:
            from ssd_tensorflow_amd.ssdvgg import SSDVGG, Session
            model = os.path.join(tmp, 'model.npz')
            with Session(0) as sess:
                net = SSDVGG(sess, 'vgg300')
                net.build_from_vgg(None, 20, max_batch=32)
                net.build_optimizer()
                net.save_checkpoint(model)
            for dec in ('pillow', 'gpu', 'pillow', 'gpu'):
                rate, small, full = detect_rate(files, dec, model, tmp)
                say('  detect.py --decoder %-6s --dtype bf16 --batch-size 32: %6.0f images/s (%d files %.1f s, 32 files %.1f s)'
                    % (dec, rate, 4 * n, full, small))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
