#!/usr/bin/env python3
"""Milliseconds of rasterising a slide's annotations into the sampled class map: the GPU kernel (annotations.rasterize, csrc/poly.hip)
beside the only route that exists without it - the reference's procedure (utils/read_xml.py:69-78: fill every polygon on a
full-resolution RGB canvas, then keep every step-th pixel) with Pillow's ImageDraw.polygon standing in for cv2.fillPoly.

  python tools/annotation_times.py [--window 1.0] [--repeats 3] [--host-divisor 4] [--out profiles/annotations_bench.json]

The workload is synthetic and seeded: 200 polygons of about 2 000 vertices each (half star-shaped with a rough outline, half smooth
blobs) on a 131 072 x 98 304 frame, sampled with steps 4, 16 and 64.  The host route cannot hold that frame's canvas (38 GB); it runs
on the frame divided by --host-divisor each way, the polygons scaled with it, and the GPU is timed on that reduced frame as well, at
the same steps, so the two are compared on equal work.  (Pillow rounds edges its own way: the two maps differ in boundary pixels and
are not compared here; the GPU map equals tests/annotations_oracle.py in the tests.)
The versions alternate in one process; each gets a window of at least --window seconds of back-to-back calls after a warm-up, and the
comparison is repeated --repeats times: the figure is the median round, the spread its range over the median.  The kernel figure is
HIP events around the launch alone, with the packed polygons already on the device; `rasterize` is the whole host call (packing in
NumPy, two uploads, the launch), wall-clock with a synchronisation at both ends.  Also recorded: the compiler's resource report of the
kernel, and the rasterisation at a slide's scoring level beside one utils.eval.predict_wsis call on that slide."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch
from PIL import Image, ImageDraw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from jpeg_times import events, summary, timed, wall  # noqa: E402
from wsi_segmentation_pipeline_amd import annotations as A, native  # noqa: E402

FRAME = (131072, 98304)
STEPS = (4, 16, 64)


def synthetic_annotations(frame=FRAME, n=200, vertices=2000, seed=3):
    """n polygons of about `vertices` vertices: even ones star-shaped with a rough outline, odd ones smooth blobs (a few harmonics)"""
    rng = np.random.default_rng(seed)
    w, h = frame
    coords, labels = [], []
    for k in range(n):
        m = int(vertices * rng.uniform(0.8, 1.2))
        r = rng.uniform(0.01, 0.06) * w
        cx, cy = rng.uniform(r, w - r), rng.uniform(r, h - r)
        t = np.linspace(0, 2 * np.pi, m, endpoint=False)
        if k % 2 == 0:
            rad = r * rng.uniform(0.55, 1.0, m)
        else:
            rad = r * (0.75 + sum(rng.uniform(0.02, 0.08) * np.sin(j * t + rng.uniform(0, 6.28)) for j in range(2, 7)))
        coords.append(np.stack((np.rint(cx + rad * np.cos(t)), np.rint(cy + rad * np.sin(t))), 1).astype(np.int64))
        labels.append(1 + k % 3)
    return coords, labels


def scaled(coords, divisor):
    return [c // divisor for c in coords]


def host_route(coords, labels, frame, step):
    """the reference's saveImage with Pillow drawing: an (H, W, 3) canvas, one fill per polygon, every step-th pixel"""
    colors = [(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)]
    img = Image.new('RGB', frame)
    draw = ImageDraw.Draw(img)
    for c, l in zip(coords, labels):
        draw.polygon([tuple(p) for p in c.tolist()], fill=colors[l])
    return np.asarray(img)[::step, ::step]


def resource_report():
    """registers, LDS and scratch of poly_raster_kernel from hipcc -Rpass-analysis=kernel-resource-usage (a compile; nothing runs)"""
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-Rpass-analysis=kernel-resource-usage', '-c',
           os.path.join(native.CSRC, 'poly.hip'), '-o', os.devnull]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = {}
    for key, pat in (('vgprs', r'VGPRs: (\d+)'), ('agprs', r'AGPRs: (\d+)'), ('sgprs', r'SGPRs: (\d+)'), ('scratch_bytes_per_lane', r'ScratchSize \[bytes/lane\]: (\d+)'),
                     ('lds_bytes', r'LDS Size \[bytes/block\]: (\d+)'), ('occupancy_waves_per_simd', r'Occupancy \[waves/SIMD\]: (\d+)')):
        m = re.search(pat, res.stdout)
        out[key] = int(m.group(1)) if m else None
    return out


def kernel_call(lib, dev, coords, labels, size, step):
    """a callable that launches wsi_poly_raster on polygons already on the device, and the map it paints"""
    edges, polys = A.pack_polygons(coords, labels)
    e, p = torch.from_numpy(edges).to(dev), torch.from_numpy(polys).to(dev)
    out = torch.zeros((size[1], size[0]), dtype=torch.uint8, device=dev)

    def call():
        native.check(lib.wsi_poly_raster(C.c_void_p(e.data_ptr()), len(edges), C.c_void_p(p.data_ptr()), len(polys), C.c_void_p(out.data_ptr()),
                                         size[0], size[1], size[0], 0, 0, step, step, C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'wsi_poly_raster')
    return call, out


def predict_wsis_share(dev, window, repeats):
    """one predict_wsis call on a 8192 x 6144 slide (levels / 4 and / 16, 64 x 64 tiles, a one-layer dense model) beside the
    rasterisation of the annotations, scaled to that slide, at the level it scores at"""
    import myargs
    import utils.dataset as ds
    import utils.eval as val
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    a = myargs.args
    a.scan_level, a.scan_resize, a.num_classes, a.class_probs = 0, 1, 4, [0., 0., 0., 0.]
    a.tile_w = a.tile_h = a.tile_stride_w = a.tile_stride_h = 64
    a.wsi_mask_pth = '/nonexistent'
    rng = np.random.default_rng(1)
    l0 = rng.integers(0, 256, (6144, 8192, 3), dtype=np.uint8)
    slide = ArraySlide([l0, l0[::4, ::4], l0[::16, ::16]], [1.0, 4.0, 16.0])
    slide.name = 'bench.svs'
    coords, labels = synthetic_annotations()
    coords = scaled(coords, 16)

    class Dense(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 4, 1)

        def forward(self, x):
            return self.conv(x)

    model = Dense().to(dev)

    def predict():
        dataset = ds.Dataset_wsis({'bench.svs': slide}, {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}, bs=256)
        val.predict_wsis(model, dataset, 0, save=False)

    def raster():
        A.level_map(coords, labels, slide, 2, dev)
    predict()
    raster()
    r = timed({'predict_wsis': (predict, wall), 'level_map': (raster, wall)}, window, repeats)
    out = {k: summary(v) for k, v in r.items()}
    out['level_map_share_of_predict_wsis'] = round(out['level_map']['ms'] / out['predict_wsis']['ms'], 5)
    out['slide'] = '8192 x 6144, scored at level 2 (512 x 384), one-layer dense model, 64 x 64 tiles'
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--host-divisor', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs a GPU')
    dev = torch.device('cuda:0')
    lib = native.load()
    coords, labels = synthetic_annotations()
    report = {'workload': {'frame': list(FRAME), 'polygons': len(coords), 'vertices': int(sum(len(c) for c in coords)), 'steps': list(STEPS)},
              'window_s': args.window, 'repeats': args.repeats, 'kernel_resources': resource_report(), 'full_frame': {}, 'reduced_frame': {}}
    print('resources', report['kernel_resources'], flush=True)
    for step in STEPS:                                           # the full frame: the GPU alone
        size = (FRAME[0] // step, FRAME[1] // step)
        call, out = kernel_call(lib, dev, coords, labels, size, step)
        call()
        r = timed({'kernel': (call, events), 'rasterize': (lambda: A.rasterize(coords, labels, size, step, out=out), wall)}, args.window, args.repeats)
        report['full_frame']['step %d' % step] = dict({k: summary(v) for k, v in r.items()}, map=list(size), covered=int((out > 0).sum().item()))
        print('full frame, step %d' % step, report['full_frame']['step %d' % step], flush=True)
        del out
    d = args.host_divisor
    frame = (FRAME[0] // d, FRAME[1] // d)
    small = scaled(coords, d)
    report['reduced_frame']['frame'] = list(frame)
    report['reduced_frame']['canvas_bytes'] = frame[0] * frame[1] * 3
    for step in STEPS:
        size = (-(-frame[0] // step), -(-frame[1] // step))
        call, out = kernel_call(lib, dev, small, labels, size, step)
        call()
        r = timed({'kernel': (call, events), 'rasterize': (lambda: A.rasterize(small, labels, size, step, out=out), wall),
                   'host_pillow': (lambda: host_route(small, labels, frame, step), lambda fn: _host_clock(fn))}, args.window, args.repeats)
        s = {k: summary(v) for k, v in r.items()}
        s['host_over_rasterize'] = round(s['host_pillow']['ms'] / s['rasterize']['ms'], 1)
        s['faster_by_more_than_the_spreads'] = bool(s['host_pillow']['ms'] * (1 - s['host_pillow']['spread']) > s['rasterize']['ms'] * (1 + s['rasterize']['spread']))
        report['reduced_frame']['step %d' % step] = dict(s, map=list(size))
        print('reduced frame, step %d' % step, report['reduced_frame']['step %d' % step], flush=True)
        del out
    report['beside_predict_wsis'] = predict_wsis_share(dev, args.window, args.repeats)
    print('beside predict_wsis', report['beside_predict_wsis'], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(report, f, indent=1)
            f.write('\n')


def _host_clock(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


if __name__ == '__main__':
    main()
