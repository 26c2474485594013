#!/usr/bin/env python3
"""Milliseconds of the region tables on the device: regions.label (csrc/regions.hip) end to end and stage by stage, beside the two ways
there were before on the same map in the same run - SciPy on the host (ndimage.label plus ndimage.sum / find_objects per class, on the
map copied to the host) and proposals.connected_components once per class, the only device route that existed (labels and a count, no
measurements; 8-connected only) - and region_table=True beside one utils.eval.predict_wsis call.

  python tools/region_times.py [--window 1.0] [--repeats 3] [--sizes 2048x1536,8192x6144] [--out profiles/regions_bench.json]

Maps, at each size: a seeded three-label blob map (the generator of tools/contour_times.py), a tumour-bed outline, one region filling the
map (all H runs go onto one record: what the contention on one record costs, next to the blob map of the same size) and, at the first
size only, the checkerboard at connectivity 4, where runs equal pixels and every pixel is a region: the adversarial case (at 8192 x
6144 its 25 million regions make SciPy's find_objects build 25 million Python tuples).  The versions alternate in one process; each gets
a window of at least --window seconds of back-to-back calls after a warm-up, and the comparison is repeated --repeats times: a figure is
the median round, its spread the rounds' range over the median.  `label` is the whole host call (its two synchronisations and its
allocations included), wall-clock with a synchronisation at both ends; a stage is HIP events round its entry, averaged over the window's
calls.  The streaming stages are set against the bytes they must move at the chip's 6.29 TB/s copy rate: count and runs each read the
map once, paint writes four bytes per pixel.  Also recorded: the compiler's resource report of every kernel, and the conditions
`blobs_faster_than_both_baselines` (by more than the two spreads together) and `checkerboard_faster_than_scipy`."""
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
from jpeg_times import summary, timed, wall  # noqa: E402
from wsi_segmentation_pipeline_amd import native, proposals as PR, regions as R  # noqa: E402

COPY_TBS = 6.29


def resource_report():
    """registers, LDS, scratch and waves per SIMD of every kernel of regions.hip from hipcc's resource remarks (a compile; nothing runs)"""
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-Rpass-analysis=kernel-resource-usage', '-c',
           os.path.join(native.CSRC, 'regions.hip'), '-o', os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    out = {}
    for block in text.split('Function Name: ')[1:]:
        name = re.match(r'_ZN(?:\d+_GLOBAL__N_1|7wsi_map)(\d+)', block)
        mangled = block.split()[0]
        short = mangled[name.end():name.end() + int(name.group(1))] if name else mangled
        if 'ILb1E' in mangled:
            short += '<runs>'
        elif 'ILb0E' in mangled:
            short += '<count>'
        vals = {}
        for key, pat in (('vgprs', r' VGPRs: (\d+)'), ('sgprs', r'TotalSGPRs: (\d+)'), ('scratch_bytes_per_lane', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('lds_bytes', r'LDS Size \[bytes/block\]: (\d+)'), ('waves_per_simd', r'Occupancy \[waves/SIMD\]: (\d+)')):
            m = re.search(pat, block)
            vals[key] = int(m.group(1)) if m else None
        out[short] = vals
    return out


def make_maps(h, w, first):
    """{kind: (u8 (h, w), connectivity)}"""
    y, x = np.ogrid[0:h, 0:w]
    bed = (((y - 0.5 * h) / (0.33 * h)) ** 2 + ((x - 0.45 * w) / (0.3 * w)) ** 2 <= 1.0)
    pad = np.pad(bed, 1)
    outline = (bed & ~(pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:])).astype(np.uint8)
    maps = {'blobs': (CF.blob_map(h, w, 3, 7, radius=8), 8), 'bed_outline': (outline, 8), 'one_region': (np.full((h, w), 3, np.uint8), 8)}
    if first:
        maps['checkerboard'] = (CF.checkerboard(h, w, 1, 2), 4)
    return maps


def scipy_route():
    try:
        from scipy import ndimage
    except ImportError:
        return None

    def route(m, connectivity):
        structure = np.ones((3, 3), int) if connectivity == 8 else None
        regions = 0
        for c in np.unique(m).tolist():
            if c == 0:
                continue
            lab, n = ndimage.label(m == c, structure)
            idx = np.arange(1, n + 1)
            ndimage.sum(np.ones(lab.shape, np.uint8), lab, idx)
            ndimage.find_objects(lab)
            regions += n
        return regions
    return route


def map_report(kind, m, connectivity, dev, window, repeats, scipy):
    h, w = m.shape
    md = torch.from_numpy(m).to(dev)
    classes = [c for c in np.unique(m).tolist() if c]
    r = R.label(md, None, connectivity)                           # warm-up
    n, n_runs = r.n, r.n_runs
    del r

    def cc_route():
        return [PR.connected_components(md == c)[1] for c in classes]

    e2e, stages, host_ms, cc_ms, same = [], {}, [], [], None
    for _ in range(repeats):                                     # the three routes alternate
        spent, calls, acc = 0.0, 0, {}
        while spent < window * 1e3:
            st = {}
            spent += wall(lambda: R.label(md, None, connectivity, stages=st))
            calls += 1
            for k, (a, b) in st.items():
                acc[k] = acc.get(k, 0.0) + a.elapsed_time(b)
        e2e.append(spent / calls)
        for k, v in acc.items():
            stages.setdefault(k, []).append(v / calls)
        spent, calls = 0.0, 0
        while spent < window * 1e3:
            spent += wall(cc_route)
            calls += 1
        cc_ms.append(spent / calls)
        if scipy is not None:
            spent, calls = 0.0, 0
            while spent < window:
                t = time.perf_counter()
                found = scipy(md.cpu().numpy(), connectivity)     # the copy to the host is part of that route
                spent += time.perf_counter() - t
                calls += 1
            host_ms.append(spent / calls * 1e3)
            same = bool(found == n) if same is None else same and found == n      # faster and different is not faster
    res = {'kind': kind, 'map': [w, h], 'connectivity': connectivity, 'runs': n_runs, 'regions': n,
           'workspace_bytes': int(native.load().wsi_region_workspace_bytes(w, h, max(n_runs, 1))), 'label': summary(e2e),
           'stages': {k: summary(v) for k, v in stages.items()},
           'connected_components_per_class': summary(cc_ms, note='8-connected only; labels and a count, no measurements')}
    for name, moved in (('count', h * w), ('runs', h * w + 16 * n_runs), ('paint', 4 * h * w + 20 * n_runs)):
        ms = res['stages'][name]['ms']
        res['stages'][name].update(bytes_it_must_move=moved, gbs=round(moved / max(ms, 1e-6) / 1e6, 1),
                                   share_of_copy_rate=round(moved / max(ms, 1e-6) / 1e6 / (COPY_TBS * 1e3), 4))
    res['cc_over_label'] = round(res['connected_components_per_class']['ms'] / res['label']['ms'], 2)
    if scipy is not None:
        res['scipy_host'] = summary(host_ms)
        res['scipy_over_label'] = round(res['scipy_host']['ms'] / res['label']['ms'], 1)
        res['same_region_count_as_scipy'] = same
    else:
        res['scipy_host'] = 'not measured: SciPy is not installed'
    return res


def faster_by_more_than_the_spreads(ours, other):
    return bool(other['ms'] - ours['ms'] > ours['spread'] * ours['ms'] + other['spread'] * other['ms'])


def predict_wsis_share(dev, window, repeats):
    """one predict_wsis call (save=False) on the 8192 x 6144 slide of tools/edt_times.py, with and without region_table"""
    import myargs
    import utils.dataset as ds
    import utils.eval as val
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    a = myargs.args
    a.scan_level, a.scan_resize, a.num_classes, a.class_probs = 0, 1, 4, [0., 0., 0., 0.]
    a.tile_w = a.tile_h = a.tile_stride_w = a.tile_stride_h = 64
    a.val_save_pth = tempfile.mkdtemp(prefix='region_times_')
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
    truth = gt.copy()
    truth[0:90, 300:512] = 0
    gd = torch.from_numpy(truth).to(dev)
    last = {}

    def predict(**kw):
        dataset = ds.Dataset_wsis({'bench.svs': slide}, {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}, bs=256)
        dataset.wsis['bench.svs']['gt'] = gd
        last.update(val.predict_wsis(model, dataset, 0, save=False, **kw)['bench.svs'])

    predict(region_table=True)
    scores = {k: last['scores'][k] for k in ('lesions_pred', 'lesions_gt', 'lesion_precision', 'lesion_recall', 'lesion_f1')}
    regions = last['regions'].n
    r = timed({'predict_wsis': (predict, wall), 'predict_wsis_region_table': (lambda: predict(region_table=True), wall)}, window, repeats)
    out = {k: summary(v) for k, v in r.items()}
    extra = out['predict_wsis_region_table']['ms'] - out['predict_wsis']['ms']
    out['region_table_extra_ms'] = round(extra, 3)
    out['region_table_share_of_predict_wsis'] = round(extra / out['predict_wsis']['ms'], 5)
    out['map'] = '512 x 384 at level 2 of a 8192 x 6144 slide'
    out['regions'] = regions
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
    scipy = scipy_route()
    report = {'window_s': args.window, 'repeats': args.repeats, 'copy_rate_tbs': COPY_TBS, 'kernel_resources': resource_report(), 'maps': []}
    print('resources', report['kernel_resources'], flush=True)

    def save():
        if args.out:
            with open(args.out, 'w') as f:
                json.dump(report, f, indent=1)
                f.write('\n')

    blobs_ok = []
    for k, size in enumerate(args.sizes.split(',')):
        w, h = (int(v) for v in size.split('x'))
        for kind, (m, connectivity) in make_maps(h, w, k == 0).items():
            res = map_report(kind, m, connectivity, dev, args.window, args.repeats, scipy)
            report['maps'].append(res)
            print(size, res, flush=True)
            if kind == 'blobs':
                ok = faster_by_more_than_the_spreads(res['label'], res['connected_components_per_class'])
                blobs_ok.append(ok and (scipy is None or faster_by_more_than_the_spreads(res['label'], res['scipy_host'])))
            if kind == 'checkerboard' and scipy is not None:
                report['checkerboard_faster_than_scipy'] = bool(res['label']['ms'] < res['scipy_host']['ms'])
            save()
    report['blobs_faster_than_both_baselines'] = bool(all(blobs_ok))
    report['beside_predict_wsis'] = predict_wsis_share(dev, args.window, args.repeats)
    print('beside predict_wsis', report['beside_predict_wsis'], flush=True)
    save()


if __name__ == '__main__':
    main()
