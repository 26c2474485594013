#!/usr/bin/env python3
"""Milliseconds of the exact Euclidean distance transform on the device: distance.distance_sq (csrc/edt.hip) end to end and pass by pass,
beside SciPy's distance_transform_edt on the host on the same map in the same run, and surface_distances beside one
utils.eval.predict_wsis call.

  python tools/edt_times.py [--window 1.0] [--repeats 3] [--sizes 2048x1536,8192x6144] [--out profiles/edt_bench.json]

Maps, at each size: a seeded three-label blob map, a tumour-bed outline (the perimeter of a convex bed), the adversarial map of a single
feature pixel (in a corner: the outward scan of the row pass is O(distance) per pixel), and the empty map.  The versions alternate in
one process; each gets a window of at least --window seconds of back-to-back calls after a warm-up, and the comparison is repeated
--repeats times: a figure is the median round, its spread the rounds' range over the median.  `distance_sq` is the whole host call on a
workspace and an output allocated once, wall-clock with a synchronisation at both ends; a pass is HIP events round its entry, averaged
over the window's calls.  The column pass streams: it is set against the bytes it must move (the map read twice, the g plane written
once) at the chip's 6.29 TB/s copy rate.  The one condition the row pass must meet is recorded as `adversarial_not_slower_than_scipy`.
Also recorded: the compiler's resource report of every kernel."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import contour_fixture as CF  # noqa: E402
import edt_oracle as O  # noqa: E402
from jpeg_times import summary, timed, wall  # noqa: E402
from wsi_segmentation_pipeline_amd import distance as D, native  # noqa: E402

COPY_TBS = 6.29


def resource_report():
    """registers, LDS, scratch and waves per SIMD of every kernel of edt.hip from hipcc's resource remarks (a compile; nothing runs)"""
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-Rpass-analysis=kernel-resource-usage', '-c',
           os.path.join(native.CSRC, 'edt.hip'), '-o', os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    out = {}
    for block in text.split('Function Name: ')[1:]:
        name = re.match(r'_ZN(?:\d+_GLOBAL__N_1|7wsi_map)(\d+)', block)
        mangled = block.split()[0]
        short = mangled[name.end():name.end() + int(name.group(1))] if name else mangled
        vals = {}
        for key, pat in (('vgprs', r' VGPRs: (\d+)'), ('sgprs', r'TotalSGPRs: (\d+)'), ('scratch_bytes_per_lane', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('lds_bytes', r'LDS Size \[bytes/block\]: (\d+)'), ('waves_per_simd', r'Occupancy \[waves/SIMD\]: (\d+)')):
            m = re.search(pat, block)
            vals[key] = int(m.group(1)) if m else None
        out[short] = vals
    return out


def make_maps(h, w):
    """{kind: u8 (h, w)}"""
    y, x = np.ogrid[0:h, 0:w]
    bed = (((y - 0.5 * h) / (0.33 * h)) ** 2 + ((x - 0.45 * w) / (0.3 * w)) ** 2 <= 1.0).astype(np.uint8)
    single = np.zeros((h, w), np.uint8)
    single[0, 0] = 1
    return {'blobs': CF.blob_map(h, w, 3, 7, radius=8), 'bed_outline': O.bwperim(bed), 'single_pixel': single, 'empty': np.zeros((h, w), np.uint8)}


def scipy_edt():
    try:
        from scipy import ndimage
    except ImportError:
        return None
    return ndimage.distance_transform_edt


def map_report(kind, m, dev, window, repeats, edt):
    h, w = m.shape
    md = torch.from_numpy(m).to(dev)
    need = int(native.load().wsi_edt_workspace_bytes(w, h))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty((h, w), dtype=torch.int32, device=dev)
    D.distance_sq(md, out=out, workspace=ws)                     # warm-up
    e2e, passes, host_ms, checked = [], {}, [], None
    for _ in range(repeats):                                     # the device and the host route alternate
        spent, calls, acc = 0.0, 0, {}
        while spent < window * 1e3:
            st = {}
            spent += wall(lambda: D.distance_sq(md, out=out, workspace=ws, stages=st))
            calls += 1
            for k, (a, b) in st.items():
                acc[k] = acc.get(k, 0.0) + a.elapsed_time(b)
        e2e.append(spent / calls)
        for k, v in acc.items():
            passes.setdefault(k, []).append(v / calls)
        if edt is not None:
            spent, calls = 0.0, 0
            while spent < window:
                t = time.perf_counter()
                ref = edt(m == 0)
                spent += time.perf_counter() - t
                calls += 1
            host_ms.append(spent / calls * 1e3)
            if checked is None and m.any():                      # faster and different is not faster: the same integers
                checked = bool(np.array_equal(np.rint(ref ** 2).astype(np.int64), out.cpu().numpy().astype(np.int64)))
            del ref
    res = {'kind': kind, 'map': [w, h], 'features': int((m != 0).sum()), 'workspace_bytes': need, 'distance_sq': summary(e2e),
           'passes': {k: summary(r) for k, r in passes.items()}}
    moved = 2 * h * w + 2 * h * w                                # the map twice (summaries, write g), the u16 plane once
    ms = res['passes']['columns']['ms']
    res['passes']['columns'].update(bytes_it_must_move=moved, gbs=round(moved / ms / 1e6, 1), share_of_copy_rate=round(moved / ms / 1e6 / (COPY_TBS * 1e3), 4))
    if edt is not None:
        res['scipy_host'] = summary(host_ms)
        res['scipy_over_distance_sq'] = round(res['scipy_host']['ms'] / res['distance_sq']['ms'], 1)
        res['equals_scipy'] = checked
    else:
        res['scipy_host'] = 'not measured: SciPy is not installed'
    return res


def predict_wsis_share(dev, window, repeats):
    """one predict_wsis call (save=False) on a 8192 x 6144 slide whose 16 x 16 blocks carry a class's grey, with and without
    boundary_scores, and surface_distances alone on the two beds"""
    import myargs
    import utils.dataset as ds
    import utils.eval as val
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    a = myargs.args
    a.scan_level, a.scan_resize, a.num_classes, a.class_probs = 0, 1, 4, [0., 0., 0., 0.]
    a.tile_w = a.tile_h = a.tile_stride_w = a.tile_stride_h = 64
    a.val_save_pth = tempfile.mkdtemp(prefix='edt_times_')
    a.wsi_mask_pth = os.path.join(a.val_save_pth, 'masks')       # an all-foreground mask: every tile is predicted
    os.makedirs(a.wsi_mask_pth)
    from PIL import Image
    Image.fromarray(np.full((384, 512), 255, np.uint8)).save(os.path.join(a.wsi_mask_pth, 'bench.svs.png'))
    greys = np.asarray((225, 165, 105, 45), np.uint8)
    gt = CF.blob_map(384, 512, 3, 7, radius=6)
    gt[120:260, 150:380] = 3
    l2 = np.repeat(greys[gt][..., None], 3, -1)
    slide = ArraySlide([np.repeat(np.repeat(l2, 16, 0), 16, 1), np.repeat(np.repeat(l2, 4, 0), 4, 1), l2], [1.0, 4.0, 16.0])
    slide.name = 'bench.svs'
    centres = torch.tensor([(g / 255.0 - a.dataset_mean[0]) / a.dataset_std[0] for g in greys.tolist()], device=dev)

    class ReadsTheGrey(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return -(x[:, :1] - centres.view(1, 4, 1, 1)).abs()

    model = ReadsTheGrey().to(dev)
    tb_gt = np.zeros((384, 512), np.uint8)
    tb_gt[100:270, 170:400] = 255
    gd, td = torch.from_numpy(gt).to(dev), torch.from_numpy(tb_gt).to(dev)
    last = {}

    def predict(**kw):
        dataset = ds.Dataset_wsis({'bench.svs': slide}, {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}, bs=256)
        dataset.wsis['bench.svs']['gt'], dataset.wsis['bench.svs']['tb_gt'] = gd, td
        last.update(val.predict_wsis(model, dataset, 0, save=False, **kw)['bench.svs'])

    predict(boundary_scores=True)
    bed = (last['tumor_bed'] > 0).to(torch.uint8)
    scores = {k: last['scores'][k] for k in ('hd_tb', 'hd95_tb', 'assd_tb')}
    r = timed({'predict_wsis': (predict, wall), 'predict_wsis_boundary_scores': (lambda: predict(boundary_scores=True), wall),
               'surface_distances_alone': (lambda: D.surface_distances(bed, td), wall)}, window, repeats)
    out = {k: summary(v) for k, v in r.items()}
    extra = out['predict_wsis_boundary_scores']['ms'] - out['predict_wsis']['ms']
    out['boundary_scores_extra_ms'] = round(extra, 3)
    out['boundary_scores_share_of_predict_wsis'] = round(extra / out['predict_wsis']['ms'], 5)
    out['map'] = '512 x 384 at level 2 of a 8192 x 6144 slide'
    out['scores'] = scores
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--sizes', default='2048x1536,8192x6144')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs a GPU')
    dev = torch.device('cuda:0')
    edt = scipy_edt()
    report = {'window_s': args.window, 'repeats': args.repeats, 'copy_rate_tbs': COPY_TBS, 'row_pass': 'outward scan', 'kernel_resources': resource_report(),
              'maps': []}
    print('resources', report['kernel_resources'], flush=True)

    def save():
        if args.out:
            with open(args.out, 'w') as f:
                json.dump(report, f, indent=1)
                f.write('\n')

    for size in args.sizes.split(','):
        w, h = (int(v) for v in size.split('x'))
        for kind, m in make_maps(h, w).items():
            res = map_report(kind, m, dev, args.window, args.repeats, edt)
            report['maps'].append(res)
            print(size, res, flush=True)
            if kind == 'single_pixel' and (w, h) == (8192, 6144) and edt is not None:
                report['adversarial_not_slower_than_scipy'] = bool(res['distance_sq']['ms'] <= res['scipy_host']['ms'])
            save()
    report['beside_predict_wsis'] = predict_wsis_share(dev, args.window, args.repeats)
    print('beside predict_wsis', report['beside_predict_wsis'], flush=True)
    save()


if __name__ == '__main__':
    main()
