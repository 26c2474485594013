#!/usr/bin/env python3
"""Milliseconds of the region hulls on the device: what hulls=True adds to regions.label (csrc/region_hulls.hip), stage by stage, beside
the ways there were before on the same map in the same run - on blob maps the host route (runs and ids copied to the host,
scipy.spatial.ConvexHull plus a NumPy Feret per region), on one-region maps the device route that existed (wsi_convex_hull_image +
wsi_hull_polygon: one hull per map from every pixel, no measurements) - and bed_size=True beside one utils.eval.predict_wsis call.

  python tools/region_hull_times.py [--window 1.0] [--repeats 3] [--out profiles/region_hulls_bench.json]

The versions alternate in one process; each gets a window of at least --window seconds of back-to-back calls after a warm-up, and the
comparison is repeated --repeats times: a figure is the median round, its spread the rounds' range over the median.  `label` and
`label_hulls` are the whole host calls (synchronisations and allocations included), wall-clock with a synchronisation at both ends;
`hull_stages` is the four hull entries alone on a labelled map (their workspace, their one synchronisation and their outputs included),
wall-clock likewise; a stage is HIP events round its entry, averaged over the window's calls.  Also recorded: the compiler's resource
report of every kernel, and the conditions `blobs_ahead_of_host_route` and `one_region_not_slower_than_device_route` (each by the two
spreads together)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import contour_fixture as CF  # noqa: E402
from jpeg_times import summary, timed, wall  # noqa: E402
from wsi_segmentation_pipeline_amd import native, regions as R  # noqa: E402
from wsi_segmentation_pipeline_amd.engine import _ptr  # noqa: E402


def resource_report():
    """registers, LDS, scratch and waves per SIMD of every kernel of region_hulls.hip from hipcc's resource remarks (a compile; nothing runs)"""
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-Rpass-analysis=kernel-resource-usage', '-c',
           os.path.join(native.CSRC, 'region_hulls.hip'), '-o', os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    out = {}
    for block in text.split('Function Name: ')[1:]:
        mangled = block.split()[0]
        name = re.search(r'(hull_\w+?_kernel|scan_\w+?_kernel)', mangled)
        vals = {}
        for key, pat in (('vgprs', r' VGPRs: (\d+)'), ('sgprs', r'TotalSGPRs: (\d+)'), ('scratch_bytes_per_lane', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('lds_bytes', r'LDS Size \[bytes/block\]: (\d+)'), ('waves_per_simd', r'Occupancy \[waves/SIMD\]: (\d+)')):
            m = re.search(pat, block)
            vals[key] = int(m.group(1)) if m else None
        out[name.group(1) if name else mangled] = vals
    return out


def host_route():
    """scipy's ConvexHull, or None where SciPy is not installed"""
    try:
        from scipy.spatial import ConvexHull
    except ImportError:
        return None
    return ConvexHull


def host_hulls(ConvexHull, runs, ids, n):
    order = np.argsort(ids, kind='stable')
    runs, ids = runs[order], ids[order]
    cuts = np.searchsorted(ids, np.arange(1, n + 2))
    feret = np.zeros(n)
    for k in range(n):
        rr = runs[cuts[k]:cuts[k + 1]]
        y, x0, x1 = rr[:, 0], rr[:, 1], rr[:, 2]
        pts = np.concatenate([np.stack([x0, y], 1), np.stack([x0, y + 1], 1), np.stack([x1, y], 1), np.stack([x1, y + 1], 1)]).astype(np.float64)
        v = pts[ConvexHull(pts).vertices]
        d = v[:, None, :] - v[None, :, :]
        feret[k] = np.sqrt((d * d).sum(-1).max())
    return feret


def label_with_workspace(md, connectivity):
    lib = native.load()
    h, w = md.shape
    probe = R.label(md, None, connectivity, labels=False)
    ws = torch.empty(lib.wsi_region_workspace_bytes(w, h, probe.n_runs), dtype=torch.uint8, device=md.device)
    return R.label(md, None, connectivity, labels=False, workspace=ws), ws


def device_route(md):
    """the hull route that existed: the hull image of the whole mask and its polygon, the vertex count read by the host"""
    lib = native.load()
    h, w = md.shape
    ws = torch.empty(lib.wsi_tumor_bed_workspace_bytes(h, w), dtype=torch.uint8, device=md.device)
    dst = torch.empty_like(md)
    cap = 4 * h + 8
    out = torch.empty((cap, 2), dtype=torch.float64, device=md.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=md.device)
    st = torch.cuda.current_stream(md.device).cuda_stream

    def run():
        native.check(lib.wsi_convex_hull_image(_ptr(md), _ptr(dst), h, w, _ptr(ws), st), 'wsi_convex_hull_image')
        native.check(lib.wsi_hull_polygon(_ptr(ws), h, w, _ptr(out), cap, _ptr(cnt), st), 'wsi_hull_polygon')
        return int(cnt.item())
    return run


def map_report(kind, m, connectivity, dev, window, repeats, against):
    h, w = m.shape
    md = torch.from_numpy(m).to(dev)
    lib = native.load()
    r, rws = label_with_workspace(md, connectivity)
    n, n_runs = r.n, r.n_runs
    st = torch.cuda.current_stream(dev).cuda_stream
    hulls_alone = lambda: R._hulls(lib, rws, int(rws.numel()), r.table, w, h, n_runs, n, dev, st, lambda name: None)
    first = hulls_alone()
    stages_acc, calls = {}, [0]

    def label_hulls():
        s = {}
        R.label(md, None, connectivity, labels=False, hulls=True, stages=s)
        torch.cuda.synchronize()
        calls[0] += 1
        for k, (a, b) in s.items():
            stages_acc[k] = stages_acc.get(k, 0.0) + a.elapsed_time(b)
    versions = {'label': (lambda: R.label(md, None, connectivity, labels=False), wall), 'label_hulls': (label_hulls, wall), 'hull_stages': (hulls_alone, wall)}
    same = None
    if against == 'device':
        route = device_route(md)
        route()
        versions['convex_hull_image_and_polygon'] = (route, wall)
    elif against == 'host' and host_route() is not None:
        ConvexHull = host_route()
        lay_runs = 0                                             # runs lie first in the region workspace; id: the eighth array
        r256 = lambda b: (b + 255) // 256 * 256
        id_at = r256(16 * n_runs) + r256(4 * (h + 1)) + 3 * r256(4 * n_runs) + 2 * r256(4 * (n_runs + 1))

        def host():
            runs = rws[lay_runs:lay_runs + 16 * n_runs].view(torch.int32).reshape(-1, 4).cpu().numpy()
            ids = rws[id_at:id_at + 4 * n_runs].view(torch.int32).cpu().numpy()
            return host_hulls(ConvexHull, runs, ids, n)
        same = bool(np.array_equal(host(), first.feret_max()))
        versions['scipy_host'] = (host, wall)
    rounds = timed(versions, window, repeats)
    res = {'kind': kind, 'map': [w, h], 'connectivity': connectivity, 'runs': n_runs, 'regions': n, 'vertices': int(first.vertices.shape[0]),
           'largest_hull': int(first.hull_n.max()), 'workspace_bytes': int(lib.wsi_regionhull_workspace_bytes(w, h, n_runs, n))}
    res.update({k: summary(v) for k, v in rounds.items()})
    res['hulls_extra_ms'] = round(res['label_hulls']['ms'] - res['label']['ms'], 3)
    res['stages'] = {k: round(v / max(calls[0], 1), 4) for k, v in stages_acc.items()}
    if same is not None:
        res['same_feret_as_host_route'] = same
    return res


def ahead_by_more_than_the_spreads(ours, other):
    return bool(other['ms'] - ours['ms'] > ours['spread'] * ours['ms'] + other['spread'] * other['ms'])


def not_slower_by_more_than_the_spreads(ours, other):
    return bool(ours['ms'] - other['ms'] <= ours['spread'] * ours['ms'] + other['spread'] * other['ms'])


def predict_wsis_share(dev, window, repeats):
    """one predict_wsis call (save=False, region_table=True) on the 8192 x 6144 slide of tools/edt_times.py, with and without bed_size"""
    import myargs
    import utils.dataset as ds
    import utils.eval as val
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    a = myargs.args
    a.scan_level, a.scan_resize, a.num_classes, a.class_probs = 0, 1, 4, [0., 0., 0., 0.]
    a.tile_w = a.tile_h = a.tile_stride_w = a.tile_stride_h = 64
    a.val_save_pth = tempfile.mkdtemp(prefix='region_hull_times_')
    a.wsi_mask_pth = os.path.join(a.val_save_pth, 'masks')
    os.makedirs(a.wsi_mask_pth)
    from PIL import Image
    Image.fromarray(np.full((384, 512), 255, np.uint8)).save(os.path.join(a.wsi_mask_pth, 'bench.svs.png'))
    greys = np.asarray((225, 165, 105, 45), np.uint8)
    gt = CF.blob_map(384, 512, 3, 7, radius=6)
    gt[120:260, 150:380] = 3
    l2 = np.repeat(greys[gt][..., None], 3, -1)
    slide = ArraySlide([np.repeat(np.repeat(l2, 16, 0), 16, 1), np.repeat(np.repeat(l2, 4, 0), 4, 1), l2], [1.0, 4.0, 16.0])
    slide.name = 'bench.svs'
    slide.mpp = 0.25
    centres = torch.tensor([(g / 255.0 - a.dataset_mean[0]) / a.dataset_std[0] for g in greys.tolist()], device=dev)

    class ReadsTheGrey(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return -(x[:, :1] - centres.view(1, 4, 1, 1)).abs()

    model = ReadsTheGrey().to(dev)
    gd = torch.from_numpy(gt).to(dev)
    bed_gt = torch.from_numpy(np.where(gt == 3, 255, 0).astype(np.uint8)).to(dev)
    last = {}

    def predict(**kw):
        dataset = ds.Dataset_wsis({'bench.svs': slide}, {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}, bs=256)
        dataset.wsis['bench.svs']['gt'] = gd
        dataset.wsis['bench.svs']['tb_gt'] = bed_gt
        last.update(val.predict_wsis(model, dataset, 0, save=False, region_table=True, **kw)['bench.svs'])

    predict(bed_size=True)
    bed = last['bed_size']
    r = timed({'predict_wsis': (predict, wall), 'predict_wsis_bed_size': (lambda: predict(bed_size=True), wall)}, window, repeats)
    out = {k: summary(v) for k, v in r.items()}
    extra = out['predict_wsis_bed_size']['ms'] - out['predict_wsis']['ms']
    out['bed_size_extra_ms'] = round(extra, 3)
    out['bed_size_share_of_predict_wsis'] = round(extra / out['predict_wsis']['ms'], 5)
    out['predict_wsis_spread'] = out['predict_wsis']['spread']
    out['map'] = '512 x 384 at level 2 of a 8192 x 6144 slide, region_table=True in both'
    out['bed_size'] = bed
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs a GPU')
    dev = torch.device('cuda:0')
    report = {'window_s': args.window, 'repeats': args.repeats, 'kernel_resources': resource_report(), 'maps': []}
    print('resources', report['kernel_resources'], flush=True)

    def save():
        if args.out:
            with open(args.out, 'w') as f:
                json.dump(report, f, indent=1)
                f.write('\n')

    y, x = np.ogrid[0:6144, 0:8192]
    bed = ((((y - 0.5 * 6144) * 0.9 + (x - 0.45 * 8192) * 0.3) / (0.33 * 6144)) ** 2 + (((x - 0.45 * 8192) * 0.9 - (y - 0.5 * 6144) * 0.3) / (0.3 * 8192)) ** 2 <= 1.0)
    cases = [('blobs', CF.blob_map(1536, 2048, 3, 7, radius=8), 8, 'host'), ('blobs', CF.blob_map(6144, 8192, 3, 7, radius=8), 8, None),
             ('one_region_full_map', np.full((6144, 8192), 3, np.uint8), 8, 'device'), ('tumour_bed_mask', bed.astype(np.uint8), 8, 'device'),
             ('one_column', np.ones((32768, 1), np.uint8), 8, None), ('checkerboard', CF.checkerboard(1536, 2048, 1, 2), 4, None)]
    for kind, m, connectivity, against in cases:
        res = map_report(kind, m, connectivity, dev, args.window, args.repeats, against)
        report['maps'].append(res)
        print(kind, res, flush=True)
        if against == 'host' and 'scipy_host' in res:
            report['blobs_ahead_of_host_route'] = ahead_by_more_than_the_spreads(res['hull_stages'], res['scipy_host'])
        if against == 'device':
            report.setdefault('one_region_not_slower_than_device_route', {})[kind] = not_slower_by_more_than_the_spreads(
                res['hull_stages'], res['convex_hull_image_and_polygon'])
        save()
    report['beside_predict_wsis'] = predict_wsis_share(dev, args.window, args.repeats)
    print('beside predict_wsis', report['beside_predict_wsis'], flush=True)
    save()


if __name__ == '__main__':
    main()
