#!/usr/bin/env python3
"""Patches per second of cellularity scoring (four test-time views + Regressor head), fused path against the reference-style loop.

  python tools/cellularity_times.py [--arch resnet18] [--precision parity] [--patch 512] [--steps 5] [--out profiles/cellularity_bench.json]

Patches are --patch x --patch (512: the reference's tile_h / tile_w), as many as fill the engine's batch with four views each.
Three versions alternate in one process, each timed with HIP events per call (median of --steps calls after one warm-up, with the
spread):
  (a) fused u8   utils.eval.SlideClassifierModel.regress_views(slide_u8=...): wsi_tile_views_u8 -> trunk on the atlas -> wsi_mlp_views
  (b) fused fp32 regress_views(x=...): wsi_views_f32 -> trunk -> wsi_mlp_views
  (c) module loop utils.eval.module_loop_views: per view torch ops, model.encoder, model.regressor (fp32 NCHW map, pf_pack, wsi_avgpool_fc,
      two wsi_linear), torch add / divide - the loop a caller could write before forward_views existed, in batches of --loop-batch
Per launch (HIP events, median of --reps after two warm-ups): the view producers, with their bytes per second (read + write once each)
against the device copy rate the project uses (tools/hbm_calib.py, 6.29 TB/s); wsi_mlp_views against two wsi_linear + torch add,
divide and clamp on the same features.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import resnets_shift  # noqa: E402
from models import models as M  # noqa: E402
from utils import eval as val  # noqa: E402
from wsi_segmentation_pipeline_amd import engine as E, synthetic as W  # noqa: E402

COPY_CEILING = 6.29e12            # bytes/s, measured device copy rate of an MI355X
VIEWS = E.VIEWS_REFERENCE


def timed(fn, reps, warm):
    ms = []
    for i in range(reps + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return {'ms_median': round(float(np.median(ms)), 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='resnet18', choices=['resnet18', 'resnet34', 'resnet50'])
    ap.add_argument('--precision', default='parity')
    ap.add_argument('--patch', type=int, default=512)
    ap.add_argument('--patches', type=int, default=0, help='0 = what fills the engine batch with four views each')
    ap.add_argument('--loop-batch', type=int, default=0, help='module-loop batch; 0 = the same patches per call as the fused path')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    T = args.patch
    net = getattr(resnets_shift, args.arch)(False, precision=args.precision)
    feat = 2048 if net.bottleneck else 512
    if net.bottleneck:
        net.load_state_dict(W.make_bottleneck_state_dict(21, list(W.RESNET50_LAYERS), with_fc=False), strict=False)
    else:
        net.load_state_dict(W.make_resnet_state_dict(31, net.layers, with_fc=False), strict=False)
    reg, cls = M.Regressor(feat, 1), M.Classifier(feat, 4)
    reg.load_state_dict(W.make_head_state_dict(32, 'regressor', feat, 1))
    cls.load_state_dict(W.make_head_state_dict(33, 'classifier', feat, 4))
    model = val.SlideClassifierModel(net, cls, reg).to(dev).eval()
    eng = net.hip_engine(dev)
    base = getattr(eng, '_par', eng)
    n = args.patches or base._views_chunk(T, T, len(VIEWS))
    g = torch.Generator(device=dev).manual_seed(3)
    stack = torch.randint(0, 256, (n * T, T, 3), dtype=torch.uint8, device=dev, generator=g)
    xy = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    xy[:, 1] = torch.arange(n, dtype=torch.int32, device=dev) * T
    x = E.tile_gather(stack, xy, T, T, base.lut)
    lb = args.loop_batch or n
    res = {'what': '%s, precision %s, %d patches of %d x %d, views %s, Regressor(%d, 1); engine batch %d images; module loop in batches of %d'
                   % (args.arch, args.precision, n, T, T, list(VIEWS), feat, n * len(VIEWS), lb),
           'patches': n, 'copy_ceiling_Bps': COPY_CEILING}

    def loop():
        return torch.cat([val.module_loop_views(model, model.regressor, x[i:i + lb], VIEWS) for i in range(0, n, lb)])
    versions = {'a_fused_u8': lambda: model.regress_views(slide_u8=stack, tile_xy=xy, ph=T, pw=T, views=VIEWS),
                'b_fused_f32': lambda: model.regress_views(x=x, views=VIEWS),
                'c_module_loop': loop}
    with torch.no_grad():
        outs = {k: fn() for k, fn in versions.items()}                    # warm-up of every version (workspaces, the 'auto' decision)
        torch.cuda.synchronize()
        res['max_abs_difference_to_module_loop'] = {k: float((outs[k].view(-1) - outs['c_module_loop'].view(-1)).abs().max()) for k in ('a_fused_u8', 'b_fused_f32')}
        times = {k: [] for k in versions}
        for _ in range(args.steps):                                       # the versions alternate
            for k, fn in versions.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b))
        for k, t in times.items():
            med = float(np.median(t))
            res[k] = {'ms_median': round(med, 2), 'ms_min': round(min(t), 2), 'ms_max': round(max(t), 2), 'ms_steps': [round(v, 2) for v in t],
                      'patches_per_s': round(n / med * 1e3, 1)}
            print(k, json.dumps(res[k]), flush=True)
        res['a_not_slower_than_c_beyond_spread'] = bool(res['a_fused_u8']['ms_min'] <= res['c_module_loop']['ms_max'])
        if hasattr(eng, 'report'):
            res['precision_report'] = eng.report

        # per launch
        ids = list(VIEWS)
        r = timed(lambda: E.tile_views(stack, xy, T, T, ids), args.reps, 2)
        nbytes = n * T * T * 3 * (len(ids) + len(ids))                    # every view reads its source tile and writes its own
        r.update(bytes=nbytes, GBps=round(nbytes / r['ms_median'] / 1e6, 1), of_copy_ceiling=round(nbytes / (r['ms_median'] * 1e-3) / COPY_CEILING, 3))
        res['launch_tile_views_u8'] = r
        r = timed(lambda: E.views_f32(x, ids), args.reps, 2)
        nbytes = n * T * T * 3 * 4 * (len(ids) + len(ids))
        r.update(bytes=nbytes, GBps=round(nbytes / r['ms_median'] / 1e6, 1), of_copy_ceiling=round(nbytes / (r['ms_median'] * 1e-3) / COPY_CEILING, 3))
        res['launch_views_f32'] = r
        f = torch.randn((len(ids) * n, feat), device=dev, generator=g).abs_()
        mlp = model._views_mlp('regressor')
        res['launch_mlp_views'] = timed(lambda: E.mlp_views(f, n, len(ids), mlp, clamp=(0.0, 1.0)), args.reps, 2)

        def two_linear():
            h = base.linear(f, mlp[0], mlp[1], relu=True)
            y = base.linear(h, mlp[2], mlp[3]).view(len(ids), n, -1)
            acc = y[0].clone()
            for k in range(1, len(ids)):
                acc += y[k]
            return (acc / len(ids)).clamp_(0.0, 1.0)
        res['launch_two_linear_plus_torch'] = timed(two_linear, args.reps, 2)
        res['mlp_views_vs_two_linear_max_abs_difference'] = float((E.mlp_views(f, n, len(ids), mlp, clamp=(0.0, 1.0))[0] - two_linear()).abs().max())
        share = (res['launch_tile_views_u8']['ms_median'] + res['launch_mlp_views']['ms_median']) / res['a_fused_u8']['ms_median']
        res['view_and_head_kernels_share_of_fused_u8_call'] = round(share, 4)
    print(json.dumps({k: v for k, v in res.items() if k.startswith('launch_') or k.endswith('share_of_fused_u8_call')}, indent=1))
    if args.out:                                                          # one entry per (arch, precision): a second run adds its own
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                doc = json.load(fh)
        doc['%s_%s' % (args.arch, args.precision)] = res
        with open(args.out, 'w') as fh:
            json.dump(doc, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
