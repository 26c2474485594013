#!/usr/bin/env python3
"""Seconds of bringing one JPEG-tiled TIFF level into HBM: the GPU decode (TiffSlide.device_level -> ingest.level_from_tiff,
csrc/jpeg.hip) beside the host route that existed before it (ingest.level_from_slide over TiffSlide.read_region: Pillow decodes the
tiles on ring threads), its stages, and the whole beside infer_slide_cls of that level.

  python tools/jpeg_times.py [--size 16384] [--window 1.0] [--repeats 3] [--out profiles/jpeg_bench.json]

A synthetic H&E-like level of size x size pixels is encoded once on the host as 256 x 256 tiles, 4:2:2, quality 70, with a JPEGTables
tag (tests/tiff_fixture.py writes the file).  The versions alternate in one process; each gets a window of at least --window seconds
of back-to-back calls after a warm-up of every version, and the comparison is repeated --repeats times: the figure is the median round,
the spread its range over the median.  End-to-end figures are wall-clock with a device synchronisation at both ends (the host work - map,
marker walk, staging - is part of them); stage figures are HIP events around the copy and the two entries, and wall-clock for the walk.
The reconstruct stage is held against the 6.29 TB/s copy rate (README.md) over the bytes it has to move: the int16 coefficients in and
the RGB level out."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import tiff_fixture as TF  # noqa: E402
from stain_times import he_level  # noqa: E402
from wsi_segmentation_pipeline_amd import ingest, native, slide as S, synthetic as W  # noqa: E402
from wsi_segmentation_pipeline_amd.engine import TrunkEngine  # noqa: E402
from wsi_segmentation_pipeline_amd.tiffslide import TiffSlide  # noqa: E402

COPY_RATE = 6.29e12


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(versions, window, repeats):
    """{name: (callable, clock)} -> {name: [ms per call of each round]}; the versions alternate"""
    rounds = {k: [] for k in versions}
    for _ in range(repeats):
        for k, (fn, clock) in versions.items():
            spent, calls = 0.0, 0
            while spent < window * 1e3:
                spent += clock(fn)
                calls += 1
            rounds[k].append(spent / calls)
    return rounds


def summary(r, **extra):
    ms = float(np.median(r))
    return dict({'ms': round(ms, 3), 'rounds_ms': [round(v, 3) for v in r], 'spread': round((max(r) - min(r)) / ms, 4)}, **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs a GPU')
    dev = torch.device('cuda:0')
    lib = native.load()
    size = args.size
    host_level = he_level(size, dev).cpu().numpy()
    tmp = tempfile.mkdtemp(prefix='jpeg_times_')
    path = os.path.join(tmp, 'level.tif')
    t0 = time.perf_counter()
    TF.write_tiff(path, [host_level], tile=(256, 256), quality=70, subsampling=1, jpegtables=True)
    encode_s = time.perf_counter() - t0
    del host_level
    slide = TiffSlide(path)
    lv = slide.levels[0]
    npix = size * size
    res = {'what': 'one level of %d x %d pixels (%d MB of RGB) as %d JPEG tiles of 256 x 256, 4:2:2, quality 70, JPEGTables: %d MB compressed '
                   '(encoded on the host in %.1f s, not part of any figure); windows of >= %.1f s per version, the versions alternating, %d rounds'
                   % (size, size, npix * 3 // 10 ** 6, len(lv.offsets), int(lv.counts.sum()) // 10 ** 6, encode_s, args.window, args.repeats),
           'host_cpus_available': len(os.sched_getaffinity(0)), 'host_route_threads': {'ring_default': 4, '16_threads': 16}}
    # (a), (b): end to end
    ring16 = ingest.IngestRing(slots=16, slot_bytes=size * 4 * 256)                     # a band = one tile row, 16 decoder threads
    keep = {}

    def gpu_path():
        keep['gpu'] = ingest.level_from_tiff(slide, 0, dev)

    def host_default():
        keep['host'] = ingest.level_from_slide(slide, 0, dev)

    def host_16():
        keep['host16'] = ingest.level_from_slide(slide, 0, dev, ring=ring16)
    gpu_path()
    host_16()
    res['gpu_bytes_differing_from_host_path'] = int((keep['gpu'] != keep['host16']).sum())
    res['decode_report'] = slide.decode_report[0]
    keep.clear()
    rounds = timed({'device_level_gpu': (gpu_path, wall), 'host_route_ring_default': (host_default, wall), 'host_route_16_threads': (host_16, wall)},
                   args.window, args.repeats)
    for k, r in rounds.items():
        res[k] = summary(r, gpixels_per_s=round(npix / float(np.median(r)) / 1e6, 3))
        print(k, json.dumps(res[k]), flush=True)
    keep.clear()
    g, h = res['device_level_gpu'], res['host_route_16_threads']
    res['host16_over_gpu'] = round(h['ms'] / g['ms'], 2)
    res['gpu_beats_host16_by_more_than_spread'] = bool(max(rounds['device_level_gpu']) < min(rounds['host_route_16_threads']))
    # (c): the stages, the whole level as one batch
    buf = np.frombuffer(slide._map, np.uint8)
    base = ingest.jpeg_parse_tables(lv.tables)[1]
    walk = lambda: ingest.jpeg_walk(buf, lv.offsets, lv.counts, base)
    rec, sets, n_sets = walk()
    n = len(rec)
    geom = (256, 256, 3, 2, 1)
    tile_ws = lib.wsi_jpeg_workspace_bytes(*geom)
    data_at, tot, stage = ingest.jpeg_stage(buf, rec, list(range(n)), np.arange(n, dtype=np.int32))
    pinned = torch.from_numpy(stage).pin_memory()
    staged = torch.empty_like(pinned, device=dev)
    ws = torch.empty(n * tile_ws, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    sets_dev = torch.from_numpy(sets[:n_sets].view(np.uint8).reshape(-1).copy()).to(dev)
    out = torch.empty((size, size, 3), dtype=torch.uint8, device=dev)
    st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    rec_bytes = n * C.sizeof(native.WsiJpegTile)

    def entropy():
        native.check(lib.wsi_jpeg_entropy(p(staged, data_at), tot, p(staged), n, p(sets_dev), n_sets, 0, *geom, p(ws), ws.numel(), p(status), 0, st()), 'entropy')

    def reconstruct():
        native.check(lib.wsi_jpeg_reconstruct(p(ws), ws.numel(), p(status), p(staged, rec_bytes), n, *geom, 1, lv.cols, lv.rows, p(out), size * 3, size, size,
                                              st()), 'reconstruct')

    def host_clock(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3
    staged.copy_(pinned)
    entropy()
    reconstruct()
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    stages = {'marker_walk_host': (walk, host_clock), 'stage_gather_host': (lambda: ingest.jpeg_stage(buf, rec, list(range(n)), np.arange(n, dtype=np.int32), stage), host_clock),
              'h2d_copy': (lambda: staged.copy_(pinned, non_blocking=True), events), 'entropy_decode': (entropy, events), 'reconstruct': (reconstruct, events),
              'copy_of_the_level': (lambda: keep.setdefault('c', torch.empty_like(out)).copy_(out), events)}
    rounds = timed(stages, args.window, args.repeats)
    for k, r in rounds.items():
        res[k] = summary(r)
    moved = 7 * npix                                            # int16 coefficients of Y + Cb + Cr at 4:2:2 (4 bytes / pixel) in, 3 bytes / pixel out
    res['h2d_copy']['gbytes_per_s'] = round((data_at + tot) / res['h2d_copy']['ms'] / 1e6, 2)
    res['reconstruct']['bytes_it_has_to_move'] = moved
    res['reconstruct']['share_of_copy_rate'] = round(moved / (res['reconstruct']['ms'] * 1e-3) / COPY_RATE, 4)
    res['reconstruct']['bytes_it_moves'] = 11 * npix            # + the u8 planes between the IDCT and the store pass, written and read
    res['entropy_decode']['compressed_gbytes_per_s'] = round(tot / res['entropy_decode']['ms'] / 1e6, 3)
    res['entropy_decode']['tiles'] = n
    for k in stages:
        print(k, json.dumps(res[k]), flush=True)
    res['stages_sum_ms'] = round(sum(res[k]['ms'] for k in ('marker_walk_host', 'stage_gather_host', 'h2d_copy', 'entropy_decode', 'reconstruct')), 3)
    res['device_level_not_in_a_stage_ms'] = round(res['device_level_gpu']['ms'] - res['stages_sum_ms'], 3)      # host time no stage holds
    del buf
    # (e): beside the inference of that level
    eng = TrunkEngine(W.make_resnet18_state_dict(11, with_fc=False), dev, head=tuple(W.make_head_state_dict(22, 'classifier')[k] for k in ('fc.0.weight', 'fc.0.bias')))
    tiles = S.tile_grid(size, size, 256, 256, 256, 256)

    def infer():
        S.infer_slide_cls(eng, out, tiles, 256, 256, 1.0 / 16, (size // 16, size // 16), 4, (0., 0., 0., 0.))
    with torch.no_grad():
        infer()
        torch.cuda.synchronize()
        r = timed({'infer_slide_cls': (infer, events)}, args.window, args.repeats)['infer_slide_cls']
    res['infer_slide_cls'] = summary(r, tiles=int(len(tiles)))
    res['device_level_over_infer'] = round(res['device_level_gpu']['ms'] / res['infer_slide_cls']['ms'], 3)
    print('infer_slide_cls', json.dumps(res['infer_slide_cls']), flush=True)
    slide.close()
    os.remove(path)
    os.rmdir(tmp)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)
            fh.write('\n')
    print(json.dumps({k: res[k] for k in ('host16_over_gpu', 'gpu_beats_host16_by_more_than_spread', 'device_level_over_infer')}))


if __name__ == '__main__':
    main()
