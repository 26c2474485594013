#!/usr/bin/env python3
"""Two builds of libwsi_hip.so alternating in ONE process on the same device buffers: milliseconds of the contour build and order stages
and of the region count, runs and runs + link stages.  tools/contour_times.py and tools/region_times.py compare two trees in two
processes, whose allocations land at different addresses; stages that bisect or chase pointers (contour build, region link) then differ
by more than a round's spread although their kernels are the same.  Here both libraries see the same map, workspace and stream.

  python tools/map_ab.py --other /path/to/other/libwsi_hip.so [--size 8192x6144] [--rounds 7] [--out profiles/map_kernels_ab.json]

Maps: the seeded three-label blob map of the two tools; for the regions also one region filling the map and a tumour-bed outline.  A
figure is the median of --rounds windows of back-to-back calls between two events; the libraries take turns window by window."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import contour_fixture as F  # noqa: E402
from wsi_segmentation_pipeline_amd import contours as CT, native  # noqa: E402
from wsi_segmentation_pipeline_amd.engine import _ptr  # noqa: E402


def load(path):
    lib = C.CDLL(path)
    for name, (res, args) in native.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def alternate(libs, call, calls, rounds):
    """{name: {median_ms, rounds_ms}}: call(lib) `calls` times per window, the libraries in turn, one warm-up window each"""
    def window(lib):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            if call(lib) != 0:
                raise RuntimeError('an entry refused its arguments')
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls
    for lib in libs.values():
        window(lib)
    ms = {name: [] for name in libs}
    for _ in range(rounds):
        for name, lib in libs.items():
            ms[name].append(round(window(lib), 5))
    return {name: {'median_ms': float(np.median(v)), 'rounds_ms': v} for name, v in ms.items()}


def contour_stages(libs, md, w, h, tp, st, dev, calls, rounds):
    lib = libs['this']
    count_ws = torch.empty(lib.wsi_contour_count_workspace_bytes(w, h), dtype=torch.uint8, device=dev)
    n_t, counts = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    native.check(lib.wsi_contour_count(_ptr(md), w, h, w, tp, _ptr(count_ws), _ptr(n_t), st), 'wsi_contour_count')
    n = int(n_t.item())
    nbytes = lib.wsi_contour_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    build = lambda l: l.wsi_contour_build(_ptr(md), w, h, w, tp, _ptr(count_ws), n, _ptr(ws), nbytes, st)
    out = {'n_edges': n, 'build': alternate(libs, build, calls, rounds)}
    native.check(build(lib), 'wsi_contour_build')             # order reads what build and ranks left and writes other arrays: it repeats
    native.check(lib.wsi_contour_ranks(_ptr(ws), nbytes, n, st), 'wsi_contour_ranks')
    out['order'] = alternate(libs, lambda l: l.wsi_contour_order(_ptr(ws), nbytes, n, w, _ptr(counts), st), calls, rounds)
    return out


def region_stages(libs, md, w, h, tp, st, dev, calls, rounds):
    lib = libs['this']
    count_ws = torch.empty(lib.wsi_region_count_workspace_bytes(w, h), dtype=torch.uint8, device=dev)
    n_t = torch.zeros(1, dtype=torch.int32, device=dev)
    count = lambda l: l.wsi_region_count(_ptr(md), w, h, w, tp, _ptr(count_ws), _ptr(n_t), st)
    native.check(count(lib), 'wsi_region_count')
    n = int(n_t.item())
    nbytes = lib.wsi_region_workspace_bytes(w, h, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    runs = lambda l: l.wsi_region_runs(_ptr(md), w, h, w, tp, _ptr(count_ws), n, _ptr(ws), nbytes, st)
    link = lambda l: runs(l) or l.wsi_region_link(_ptr(ws), nbytes, w, h, n, 8, st)       # the link needs the parents the runs stage leaves
    return {'n_runs': n, 'count': alternate(libs, count, calls, rounds), 'runs': alternate(libs, runs, calls, rounds),
            'runs+link': alternate(libs, link, calls, rounds)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--other', required=True, help='the libwsi_hip.so of the build to compare with')
    ap.add_argument('--size', default='8192x6144')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=60)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs a GPU')
    dev = torch.device('cuda:0')
    libs = {'other': load(args.other), 'this': load(native.LIB_PATH)}
    w, h = (int(v) for v in args.size.split('x'))
    y, x = np.ogrid[0:h, 0:w]
    bed = (((y - 0.5 * h) / (0.33 * h)) ** 2 + ((x - 0.45 * w) / (0.3 * w)) ** 2 <= 1.0)
    pad = np.pad(bed, 1)
    maps = {'blobs': F.blob_map(h, w, 3, 7, radius=8), 'one_region': np.full((h, w), 3, np.uint8),
            'bed_outline': (bed & ~(pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:])).astype(np.uint8)}
    table = np.ascontiguousarray(CT.traced_table(None), np.uint8)
    tp = table.ctypes.data_as(C.c_void_p)
    report = {'map': [w, h], 'rounds': args.rounds, 'calls_per_window': args.calls, 'regions': {}}
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        for kind, m in maps.items():
            md = torch.from_numpy(m).to(dev)
            if kind == 'blobs':
                report['contours'] = contour_stages(libs, md, w, h, tp, st, dev, args.calls, args.rounds)
                print('contours', report['contours'], flush=True)
            report['regions'][kind] = region_stages(libs, md, w, h, tp, st, dev, args.calls, args.rounds)
            print('regions', kind, report['regions'][kind], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(report, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
