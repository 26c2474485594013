#!/usr/bin/env python3
"""Patches per second of the FPN 'seg' model (parity mode, 256 x 256 tiles) on the HIP path, beside the same module's torch-op forward and
the HIP U-Net and Linknet on the same tiles, and what its three memory-bound kernel kinds reach of the copy rate.

  python tools/fpn_times.py [--encoder resnet18|resnet34|resnet50] [--tiles 512] [--patch 256] [--window 1.0] [--repeats 3] [--out profiles/fpn_bench.json]

The versions alternate in one process; each gets a window of at least --window seconds of back-to-back calls (HIP events per call) after
a warm-up of every version, and the whole comparison is repeated --repeats times: the figure is the median round, the spread its range.
  (a) hip_u8        FPNEngine.forward_tiles: tiles read from a device-resident u8 slide (the product path of utils.eval)
  (b) hip_f32       model(x) in eval mode: the same launches on normalised fp32 tiles
  (c) torch_ops     the same module's torch-op forward (training-mode code path, BatchNorm and Dropout in eval mode) on the same GPU
  (d) unet_hip_u8   the HIP U-Net (same encoder, same tiles)
  (e) linknet_hip_u8  the HIP Linknet (BasicBlock encoders only)
Then one profiled forward of (a) (wsi_prof_begin / wsi_prof_end, a run of its own): milliseconds per record kind, and for the three kinds
of csrc/fpn.hip the bytes they have to move - computed here from the shapes - over their time, as a share of the 6.29 TB/s copy rate
(README.md).  Events between launches slow the stream down: the per-kind table is not an end-to-end figure.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wsi_segmentation_pipeline_amd import engine as E, native, synthetic as W, unet  # noqa: E402

COPY_RATE = 6.29e12                      # bytes / s of a device-to-device copy on this card (README.md)
KINDS = {1: '3x3 stride 1 (encoder)', 2: '3x3 stride 2 (encoder)', 3: '1x1 stride-2 downsample', 4: 'stem + max pool', 5: '3x3 stride 1 (layer 1)',
         6: 'seg unit 3x3 conv', 7: 'nearest x2 upsample of the pyramid', 9: 'refused fused launch', 11: '1x1 stride 1 (encoder)',
         12: 'lateral 1x1 conv', 15: 'GroupNorm statistics', 16: 'GroupNorm apply (+ upsample)', 17: 'merge + head + x4'}
UNIT_LEVEL = (0, 1, 2, 1, 2, 2, 3)       # the pyramid level (/ 32 ... / 4) each of the seven seg units reads (csrc/fpn.hip FPN_UNIT_LEVEL)


def new_kind_bytes(n, patch, classes, bytes_per_channel=4):
    """Bytes each record of kinds 15 / 16 / 17 has to move for n tiles of patch x patch, in record order: the statistics read their
    128-channel map once; the apply reads it once more and writes the (upsampled) result; the merge + head reads four quarter-resolution
    maps, writes and re-reads the fp32 quarter logits and writes the fp32 logits."""
    px = 128 * bytes_per_channel
    stats, apply = [], []
    for L in UNIT_LEVEL:
        side = (patch // 32) << L
        stats.append(n * side * side * px)
        apply.append(n * side * side * px * (5 if L < 3 else 2))
    q = patch // 4
    head = n * (4 * q * q * px + 2 * classes * q * q * 4 + classes * patch * patch * 4)
    return {15: stats, 16: apply, 17: [head]}


def _profile(lib, run, n, patch, classes):
    cap = 4096
    native.check(lib.wsi_prof_begin(cap), 'wsi_prof_begin')
    try:
        run()
    finally:
        ms, kind, fl = np.zeros(cap, np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        cnt = lib.wsi_prof_end(*[a.ctypes.data_as(C.c_void_p) for a in (ms, kind, fl)], cap)
    ms, kind = ms[:cnt], kind[:cnt]
    total, calls = float(ms.sum()), max(1, int((kind == 17).sum()))
    out = {'records': int(cnt), 'engine_calls': calls, 'ms_total': round(total, 3), 'by_kind': {}}
    need = new_kind_bytes(n // calls, patch, classes)
    for k in sorted(set(int(v) for v in kind)):
        t = ms[kind == k]
        row = {'launches': int(t.size), 'ms': round(float(t.sum()), 3), 'share': round(float(t.sum()) / total, 4)}
        if k in need:
            b = float(sum(need[k])) * calls
            row['bytes'] = int(b)
            row['share_of_copy_rate'] = round(b / (float(t.sum()) * 1e-3) / COPY_RATE, 4)
            row['ms_per_launch'] = [round(float(v), 4) for v in t[:len(need[k])]]
            row['share_of_copy_rate_per_launch'] = [round(bb / (float(v) * 1e-3) / COPY_RATE, 4) for bb, v in zip(need[k], t)]
        out['by_kind']['%d %s' % (k, KINDS.get(k, '?'))] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--encoder', default='resnet18', choices=['resnet18', 'resnet34', 'resnet50'])
    ap.add_argument('--tiles', type=int, default=512)
    ap.add_argument('--patch', type=int, default=256)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs a GPU')
    dev = torch.device('cuda:0')
    n, T, classes = args.tiles, args.patch, 4
    arch, layers = unet.ENCODERS[args.encoder]
    basic = arch == 'basic'
    sd = W.make_fpn_state_dict(31, layers, classes) if basic else W.make_fpn_bottleneck_state_dict(31, layers, classes)
    model = unet.FPN(args.encoder, encoder_weights=None, classes=classes, activation=None)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    eng = model.hip_engine(dev)
    ueng = unet.UNetEngine(W.make_unet_resnet_state_dict(21, layers, classes) if basic else W.make_unet_bottleneck_state_dict(21, layers, classes),
                           dev, planes=E.PARITY)
    leng = unet.LinknetEngine(W.make_linknet_state_dict(21, layers, classes), dev, planes=E.PARITY) if basic else None
    g = torch.Generator(device=dev).manual_seed(3)
    stack = torch.randint(0, 256, (n * T, T, 3), dtype=torch.uint8, device=dev, generator=g)
    xy = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    xy[:, 1] = torch.arange(n, dtype=torch.int32, device=dev) * T
    x = E.tile_gather(stack, xy, T, T, eng.trunk.lut)

    def torch_ops():
        model.train()
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.Dropout2d)):
                m.eval()
        try:
            return model(x)
        finally:
            model.eval()

    versions = {'a_hip_u8': lambda: eng.forward_tiles(stack, xy, T, T), 'b_hip_f32': lambda: model(x), 'c_torch_ops': torch_ops,
                'd_unet_hip_u8': lambda: ueng.forward_tiles(stack, xy, T, T)}
    if leng is not None:
        versions['e_linknet_hip_u8'] = lambda: leng.forward_tiles(stack, xy, T, T)
    res = {'what': 'FPN on %s, parity mode, %d tiles of %d x %d, classes %d; HIP events per call, windows of >= %.1f s per version, the versions '
                   'alternating, %d rounds' % (args.encoder, n, T, T, classes, args.window, args.repeats),
           'tiles': n, 'engine_batch': eng._batch(T, T), 'workspace_bytes_per_tile': int(eng._ws_bytes(C.byref(eng.dw), 16, T, T, eng.planes) // 16)}
    with torch.no_grad():
        outs = {k: fn() for k, fn in versions.items() if k[0] in 'abc'}           # warm-up of every version and shape
        for k, fn in versions.items():
            if k not in outs:
                fn()
        torch.cuda.synchronize()
        res['max_abs_difference_to_torch_ops'] = {k: float((outs[k] - outs['c_torch_ops']).abs().max()) for k in ('a_hip_u8', 'b_hip_f32')}
        res['max_abs_logit'] = float(outs['c_torch_ops'].abs().max())
        del outs
        rounds = {k: [] for k in versions}
        for _ in range(args.repeats):
            for k, fn in versions.items():                                        # the versions alternate
                spent, calls = 0.0, 0
                while spent < args.window * 1e3:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    spent += a.elapsed_time(b)
                    calls += 1
                rounds[k].append(n * calls / spent * 1e3)
        for k, r in rounds.items():
            res[k] = {'patches_per_s': round(float(np.median(r)), 1), 'rounds': [round(v, 1) for v in r],
                      'spread': round((max(r) - min(r)) / float(np.median(r)), 4)}
            print(k, json.dumps(res[k]), flush=True)
        res['hip_u8_over_torch_ops'] = round(res['a_hip_u8']['patches_per_s'] / res['c_torch_ops']['patches_per_s'], 3)
        res['hip_u8_over_torch_ops_worst_rounds'] = round(min(rounds['a_hip_u8']) / max(rounds['c_torch_ops']), 3)
        res['hip_u8_over_unet_hip_u8'] = round(res['a_hip_u8']['patches_per_s'] / res['d_unet_hip_u8']['patches_per_s'], 3)
        res['prof'] = _profile(eng.lib, versions['a_hip_u8'], n, T, classes)
    print(json.dumps(res['prof']['by_kind'], indent=1))
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                doc = json.load(fh)
        doc['%s_parity_%d' % (args.encoder, n)] = res
        with open(args.out, 'w') as fh:
            json.dump(doc, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
