#!/usr/bin/env python3
"""Milliseconds of tracing a class map into annotation polygons: contours.trace (csrc/contour.hip) end to end and stage by stage, beside
the only host route this project has - the map copied to the host and traced by the NumPy / Python spec (tests/contours_oracle.py;
it is NOT cv2.findContours, which is absent here and follows another rule) - and the save_xml hook beside one utils.eval.predict_wsis call.

  python tools/contour_times.py [--window 1.0] [--repeats 3] [--out profiles/contours_bench.json]

Maps: seeded three-label blob maps of 2 048 x 1 536 (a level-2 map) and 8 192 x 6 144.  The versions alternate in one process; each gets
a window of at least --window seconds of back-to-back calls after a warm-up, and the comparison is repeated --repeats times: a figure is
the median round, its spread the rounds' range over the median.  `trace` is the whole host call (five entries, two read-backs of counts,
the workspace allocations), wall-clock with a synchronisation at both ends; a stage is HIP events round its entry, averaged over the
window's calls.  The streaming stages (count, build, emit) are set against the bytes they must move at the chip's 6.29 TB/s copy rate.
Also recorded: the compiler's resource report of every kernel."""
import argparse
import json
import math
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
import contour_fixture as F  # noqa: E402
import contours_oracle as O  # noqa: E402
from jpeg_times import summary, timed, wall  # noqa: E402
from wsi_segmentation_pipeline_amd import contours as CT, native  # noqa: E402

COPY_TBS = 6.29


def resource_report():
    """registers, LDS, scratch and waves per SIMD of every kernel of contour.hip from hipcc's resource remarks (a compile; nothing runs)"""
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-Rpass-analysis=kernel-resource-usage', '-c',
           os.path.join(native.CSRC, 'contour.hip'), '-o', os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    out = {}
    for block in text.split('Function Name: ')[1:]:
        name = re.match(r'_ZN(?:\d+_GLOBAL__N_1|7wsi_map)(\d+)', block)
        mangled = block.split()[0]
        short = mangled[name.end():name.end() + int(name.group(1))] if name else mangled
        if 'ILb0E' in mangled or 'ILb1E' in mangled:
            short += '<build>' if 'ILb1E' in mangled else '<count>'
        elif re.search(r'kernelI[jm]E', mangled):
            short += '<u64>' if 'kernelImE' in mangled else '<u32>'
        vals = {}
        for key, pat in (('vgprs', r' VGPRs: (\d+)'), ('sgprs', r'TotalSGPRs: (\d+)'), ('scratch_bytes_per_lane', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('lds_bytes', r'LDS Size \[bytes/block\]: (\d+)'), ('waves_per_simd', r'Occupancy \[waves/SIMD\]: (\d+)')):
            m = re.search(pat, block)
            vals[key] = int(m.group(1)) if m else None
        out[short] = vals
    return out


def trace_rounds(md, table, step, window, repeats, host=None):
    """[end-to-end ms per round], {stage: [ms per round]}, [host ms per round]: the device and the host route alternate"""
    e2e, stages, host_ms = [], {}, []
    for _ in range(repeats):
        spent, calls, acc = 0.0, 0, {}
        while spent < window * 1e3:
            st = {}
            spent += wall(lambda: CT.trace_raw(md, table, step, stages=st))
            calls += 1
            for k, (a, b) in st.items():
                acc[k] = acc.get(k, 0.0) + a.elapsed_time(b)
        e2e.append(spent / calls)
        for k, v in acc.items():
            stages.setdefault(k, []).append(v / calls)
        if host is not None:
            spent, calls = 0.0, 0
            while spent < window:
                t = time.perf_counter()
                host()
                spent += time.perf_counter() - t
                calls += 1
            host_ms.append(spent / calls * 1e3)
    return e2e, stages, host_ms


def map_report(h, w, dev, window, repeats, with_host):
    m = F.blob_map(h, w, 3, 7, radius=8)
    md = torch.from_numpy(m).to(dev)
    table = CT.traced_table(None)
    v, rec, a2, n_edges = CT.trace_raw(md, table, 16)           # warm-up, and the sizes
    nv, nl = len(v), len(rec)
    del v, rec, a2
    host = (lambda: O.trace(md.cpu().numpy(), None, 16)) if with_host else None
    e2e, stages, host_ms = trace_rounds(md, table, 16, window, repeats, host)
    out = {'map': [w, h], 'n_edges': n_edges, 'n_loops': nl, 'n_vertices': nv, 'doubling_rounds': max(0, math.ceil(math.log2(n_edges))),
           'workspace_bytes': int(native.load().wsi_contour_workspace_bytes(n_edges)), 'trace': summary(e2e),
           'stages': {k: summary(r) for k, r in stages.items()}}
    must_move = {'count': h * w, 'build': h * w + n_edges * (4 + 1 + 4 + 8 + 4), 'emit': n_edges * 12 + nv * 8 + nl * 40}
    for k, nbytes in must_move.items():
        ms = out['stages'][k]['ms']
        out['stages'][k].update(bytes_it_must_move=nbytes, gbs=round(nbytes / ms / 1e6, 1), share_of_copy_rate=round(nbytes / ms / 1e6 / (COPY_TBS * 1e3), 4))
    out['stages_sum_ms'] = round(sum(s['ms'] for s in out['stages'].values()), 3)
    if with_host:
        out['host_numpy_spec'] = summary(host_ms)
        out['host_over_trace'] = round(out['host_numpy_spec']['ms'] / out['trace']['ms'], 1)
    return out


def predict_wsis_share(dev, window, repeats):
    """one predict_wsis call (save=True) on a 8192 x 6144 slide whose 16 x 16 blocks carry a class's grey, with and without save_xml, and the
    hook's two halves alone on the map it traces: the device trace and the XML text"""
    import myargs
    import utils.dataset as ds
    import utils.eval as val
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    a = myargs.args
    a.scan_level, a.scan_resize, a.num_classes, a.class_probs = 0, 1, 4, [0., 0., 0., 0.]
    a.tile_w = a.tile_h = a.tile_stride_w = a.tile_stride_h = 64
    a.val_save_pth = tempfile.mkdtemp(prefix='contour_times_')
    a.wsi_mask_pth = os.path.join(a.val_save_pth, 'masks')       # an all-foreground mask: every tile is predicted
    os.makedirs(a.wsi_mask_pth)
    from PIL import Image
    Image.fromarray(np.full((384, 512), 255, np.uint8)).save(os.path.join(a.wsi_mask_pth, 'bench.svs.png'))
    greys = np.asarray((225, 165, 105, 45), np.uint8)
    gt = F.blob_map(384, 512, 3, 7, radius=6)
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

    def predict(**kw):
        val.predict_wsis(model, ds.Dataset_wsis({'bench.svs': slide}, {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}, bs=256), 0, **kw)

    gd = torch.from_numpy(gt).to(dev)
    traced = CT.trace(gd, (1, 2, 3), 16, bounds=(8192, 6144))
    xml = os.path.join(a.val_save_pth, 'alone.xml')
    predict(save_xml=True)
    r = timed({'predict_wsis': (predict, wall), 'predict_wsis_save_xml': (lambda: predict(save_xml=True), wall),
               'trace_alone': (lambda: CT.trace(gd, (1, 2, 3), 16, bounds=(8192, 6144)), wall),
               'write_imagescope_alone': (lambda: CT.write_imagescope(xml, traced), wall)}, window, repeats)
    out = {k: summary(v) for k, v in r.items()}
    extra = out['predict_wsis_save_xml']['ms'] - out['predict_wsis']['ms']
    out['save_xml_extra_ms'] = round(extra, 3)
    out['save_xml_share_of_predict_wsis'] = round(extra / out['predict_wsis']['ms'], 5)
    out['map'] = '512 x 384 at level 2 of a 8192 x 6144 slide: %d loops, %d vertices, %d bytes of XML' % (len(traced), len(traced.vertices), os.path.getsize(xml))
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
    report = {'window_s': args.window, 'repeats': args.repeats, 'copy_rate_tbs': COPY_TBS, 'kernel_resources': resource_report()}
    print('resources', report['kernel_resources'], flush=True)
    report['level2_map'] = map_report(1536, 2048, dev, args.window, args.repeats, True)
    print('2048 x 1536', report['level2_map'], flush=True)
    report['large_map'] = map_report(6144, 8192, dev, args.window, args.repeats, True)
    print('8192 x 6144', report['large_map'], flush=True)
    report['beside_predict_wsis'] = predict_wsis_share(dev, args.window, args.repeats)
    print('beside predict_wsis', report['beside_predict_wsis'], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(report, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
