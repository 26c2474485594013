#!/usr/bin/env python3
"""Seconds of writing one resident level as a JPEG-tiled TIFF: the GPU encode (tiffwrite.write_pyramid, csrc/jpeg_enc.hip) beside the
only route that existed before it - the same tiles encoded by Pillow on the host and written with the same container code - and its
stages.

  python tools/jpeg_enc_times.py [--size 16384] [--window 1.0] [--repeats 3] [--out profiles/jpeg_enc_bench.json]

The level is the synthetic H&E-like one of tools/jpeg_times.py, size x size pixels, 256 x 256 tiles, quality 70, once at 4:2:0 and
once at 4:2:2.  The versions alternate in one process; each gets a window of at least --window seconds of back-to-back calls after a
warm-up of every version, and the comparison is repeated --repeats times: the figure is the median round, the spread its range over
the median.  End-to-end figures are wall-clock with a device synchronisation at both ends and include the file write (into a
temporary directory); the host route starts from the level in host memory (its device-to-host copy is not charged to it) and runs
Pillow on 4 and on 16 threads.  Stage figures are HIP events around one whole-level batch, wall-clock for the file write.  The
transform kernel is held against the 6.29 TB/s copy rate (README.md) over the bytes it has to move: 3 per pixel in, the int16
coefficients out."""
import argparse
import ctypes as C
import io
import json
import os
import struct
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from jpeg_times import COPY_RATE, events, summary, timed, wall  # noqa: E402
from stain_times import he_level  # noqa: E402
from wsi_segmentation_pipeline_amd import native, tiffwrite as TW  # noqa: E402
from wsi_segmentation_pipeline_amd.tiffslide import TiffSlide  # noqa: E402

TILE, QUALITY = (256, 256), 70


def _pillow_scan(tile, ss):
    """the scan bytes of Pillow's abbreviated stream of one tile"""
    b = io.BytesIO()
    Image.fromarray(tile).save(b, 'JPEG', quality=QUALITY, subsampling=ss, streamtype=2)
    s = b.getbuffer()
    at = bytes(s[:64]).index(b'\xff\xda')
    return bytes(s[at + 2 + struct.unpack('>H', s[at + 2:at + 4])[0]:len(s) - 2])


def pillow_encoder(threads):
    """a stand-in for the device encode (tiffwrite.write_pyramid's `encode`): Pillow on `threads` threads, one batch per tile row"""
    pool = ThreadPoolExecutor(threads)

    def encode(level, tile, qtables, sampling, restart):
        tw, th = tile
        ss = TW.SAMPLINGS.index(tuple(sampling))
        cols = level.shape[1] // tw
        rows = [pool.submit(lambda y=y: [_pillow_scan(np.ascontiguousarray(level[y:y + th, x * tw:(x + 1) * tw]), ss) for x in range(cols)])
                for y in range(0, level.shape[0], th)]
        for k, fut in enumerate(rows):
            scans = fut.result()
            sizes = np.array([len(s) for s in scans], np.uint32)
            offs = np.zeros(cols, np.uint64)
            np.cumsum(sizes[:-1], out=offs[1:])
            yield k * cols, sizes, offs, np.frombuffer(b''.join(scans), np.uint8)
    return encode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs a GPU')
    if args.size % 256:
        raise SystemExit('--size: a multiple of 256 (the host route encodes whole tiles)')
    dev = torch.device('cuda:0')
    lib = native.load()
    size = args.size
    level = he_level(size, dev)
    host_level = level.cpu().numpy()
    npix, n = size * size, (size // 256) ** 2
    tmp = tempfile.mkdtemp(prefix='jpeg_enc_times_')
    gpu_path, host_path = os.path.join(tmp, 'gpu.tif'), os.path.join(tmp, 'host.tif')
    res = {'what': 'one resident level of %d x %d pixels (%d MB of RGB) written as %d JPEG tiles of 256 x 256, quality 70, JPEGTables; windows of '
                   '>= %.1f s per version, the versions alternating, %d rounds' % (size, size, npix * 3 // 10 ** 6, n, args.window, args.repeats),
           'host_cpus_available': len(os.sched_getaffinity(0))}
    pil4, pil16 = pillow_encoder(4), pillow_encoder(16)
    q = TW.quality_tables(QUALITY)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dp = lambda t: C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def host_clock(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3
    for name, samp in (('420', (2, 2)), ('422', (2, 1))):
        r = res[name] = {}
        report = {}

        def gpu():
            report['gpu'] = TW.write_pyramid(gpu_path, [level], tile=TILE, quality=QUALITY, subsampling=samp)

        def gpu_pyramid():
            report['pyr'] = TW.write_pyramid(gpu_path, level, tile=TILE, quality=QUALITY, subsampling=samp, downsample=2)

        def host(enc):
            return lambda: report.__setitem__('host', TW.write_pyramid(host_path, [host_level], tile=TILE, quality=QUALITY, subsampling=samp, encode=enc))
        gpu()
        host(pil16)()
        a, b = TiffSlide(gpu_path), TiffSlide(host_path)
        r['tile_streams_differing_from_pillow'] = sum(bytes(a.tile_bytes(0, i)) != bytes(b.tile_bytes(0, i)) for i in range(n))
        a.close()
        b.close()
        r['file_bytes'] = report['gpu']['bytes']
        host(pil4)()
        gpu_pyramid()
        r['pyramid_levels'] = [(l['width'], l['height']) for l in report['pyr']['levels']]
        rounds = timed({'write_pyramid_gpu_one_level': (gpu, wall), 'write_pyramid_gpu_whole_pyramid': (gpu_pyramid, wall),
                        'host_route_pillow_4_threads': (host(pil4), wall), 'host_route_pillow_16_threads': (host(pil16), wall)}, args.window, args.repeats)
        for k, v in rounds.items():
            r[k] = summary(v, gpixels_per_s=round(npix / float(np.median(v)) / 1e6, 3))
            print(name, k, json.dumps(r[k]), flush=True)
        r['host16_over_gpu'] = round(r['host_route_pillow_16_threads']['ms'] / r['write_pyramid_gpu_one_level']['ms'], 2)
        r['gpu_beats_host16_by_more_than_spread'] = bool(max(rounds['write_pyramid_gpu_one_level']) < min(rounds['host_route_pillow_16_threads']))
        # the stages, the whole level as one batch
        hs, vs = samp
        tile_ws = lib.wsi_jenc_workspace_bytes(256, 256, 3, hs, vs)
        ws = torch.empty(n * tile_ws, dtype=torch.uint8, device=dev)
        sizes_dev = torch.empty(n, dtype=torch.int32, device=dev)
        ranges = torch.empty(12 * n + 8, dtype=torch.uint8, device=dev)
        cols = size // 256

        def transform():
            native.check(lib.wsi_jenc_transform(dp(level), level.stride(0), size, size, cols, cols, 0, n, 256, 256, 3, hs, vs, p(q[0]), p(q[1]), dp(ws), ws.numel(),
                                                st()), 'transform')

        def size_pass():
            native.check(lib.wsi_jenc_entropy_size(dp(ws), ws.numel(), n, 256, 256, 3, hs, vs, 0, dp(sizes_dev), 0, st()), 'size')
        transform()
        size_pass()
        sizes = sizes_dev.cpu().numpy().view(np.uint32)
        offs = np.zeros(n, np.uint64)
        np.cumsum((sizes[:-1].astype(np.uint64) + 15) // 16 * 16, out=offs[1:])
        total = int(offs[-1]) + int(sizes[-1])
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        pinned = torch.empty(total, dtype=torch.uint8).pin_memory()

        def write_pass():
            native.check(lib.wsi_jenc_entropy_write(dp(ws), ws.numel(), n, 256, 256, 3, hs, vs, 0, p(offs), p(sizes), dp(ranges), dp(out), total, 0, st()), 'write')
        head = TW.tile_header(256, 256, 3, samp)
        host_buf = pinned.numpy()

        def file_write():
            with open(gpu_path, 'wb') as f:
                TW.write_tiles(f, head, sizes, offs, host_buf, [], [])
        write_pass()
        stages = {'transform': (transform, events), 'entropy_size_pass': (size_pass, events), 'entropy_write_pass': (write_pass, events),
                  'd2h_copy': (lambda: pinned.copy_(out, non_blocking=True), events), 'file_write_host': (file_write, host_clock),
                  'copy_of_the_level': (lambda: report.setdefault('c', torch.empty_like(level)).copy_(level), events)}
        rounds = timed(stages, args.window, args.repeats)
        for k, v in rounds.items():
            r[k] = summary(v)
        report.clear()
        moved = (3 + tile_ws * n // npix) * npix                # RGB in, int16 coefficients out
        r['transform']['bytes_it_has_to_move'] = moved
        r['transform']['share_of_copy_rate'] = round(moved / (r['transform']['ms'] * 1e-3) / COPY_RATE, 4)
        r['scan_bytes'] = int(sizes.sum())
        r['entropy_write_pass']['compressed_gbytes_per_s'] = round(int(sizes.sum()) / r['entropy_write_pass']['ms'] / 1e6, 3)
        r['d2h_copy']['gbytes_per_s'] = round(total / r['d2h_copy']['ms'] / 1e6, 2)
        r['stages_sum_ms'] = round(sum(r[k]['ms'] for k in ('transform', 'entropy_size_pass', 'entropy_write_pass', 'd2h_copy', 'file_write_host')), 3)
        r['write_pyramid_not_in_a_stage_ms'] = round(r['write_pyramid_gpu_one_level']['ms'] - r['stages_sum_ms'], 3)
        for k in stages:
            print(name, k, json.dumps(r[k]), flush=True)
        del ws, out, pinned, host_buf
    for f in (gpu_path, host_path):
        if os.path.exists(f):
            os.remove(f)
    os.rmdir(tmp)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)
            fh.write('\n')
    print(json.dumps({k: {j: res[k][j] for j in ('host16_over_gpu', 'gpu_beats_host16_by_more_than_spread', 'tile_streams_differing_from_pillow')}
                      for k in ('420', '422')}))


if __name__ == '__main__':
    main()
