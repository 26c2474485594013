#!/usr/bin/env python3
"""Patches per second of the Linknet 'seg' model (parity mode, 256 x 256 tiles) on the HIP path, beside the same module's torch-op forward
and the HIP U-Net on the same tiles, and which route of its last block + head is faster.

  python tools/linknet_times.py [--encoder resnet18] [--tiles 512] [--patch 256] [--steps 7] [--out profiles/linknet_bench.json]

Six versions alternate in one process, each call timed with HIP events (median of --steps calls after a warm-up of every version, with
the spread):
  (a) hip_f32          model(x) in eval mode: wsi_linknet_forward on normalised fp32 tiles (fused last block + head)
  (b) hip_u8           LinknetEngine.forward_tiles: the same launches fed from a device-resident u8 slide (the product path of utils.eval)
  (c) hip_u8_no_tail   (b) under ConvMode.LINKNET_NO_TAIL: the last block as three launches + the head kernel
  (d) torch_ops        the same module's torch-op forward (training-mode code path with BatchNorm in eval mode) on the same GPU
  (e) unet_hip_u8      the HIP U-Net (same encoder, same tiles) through UNetEngine.forward_tiles
  (f) trunk_hip_u8     the bare trunk (TrunkEngine.forward_tiles, pooled features) in the same precision mode: the decoder-free floor
Then one profiled forward of (b) and one of (c) (wsi_prof_begin / wsi_prof_end, runs of their own): the time share of every record kind.
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

KINDS = {1: '3x3 stride 1 (encoder)', 2: '3x3 stride 2 (encoder)', 3: '1x1 stride-2 downsample', 4: 'stem + max pool', 5: '3x3 stride 1 (layer 1)',
         7: 'x0 stem conv', 8: '1x1 head', 9: 'refused fused launch', 12: 'decoder 1x1 conv', 13: 'decoder transposed conv',
         14: 'fused last block + head'}


def _profile(lib, run):
    cap = 4096
    native.check(lib.wsi_prof_begin(cap), 'wsi_prof_begin')
    try:
        run()
    finally:
        ms, kind, fl = np.zeros(cap, np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        cnt = lib.wsi_prof_end(*[a.ctypes.data_as(C.c_void_p) for a in (ms, kind, fl)], cap)
    total = float(ms[:cnt].sum())
    return {'records': int(cnt), 'ms_total': round(total, 3),
            'share_by_kind': {'%d %s' % (k, KINDS.get(k, '?')): {'launches': int((kind[:cnt] == k).sum()), 'ms': round(float(ms[:cnt][kind[:cnt] == k].sum()), 3),
                                                                'share': round(float(ms[:cnt][kind[:cnt] == k].sum()) / total, 4)}
                              for k in sorted(set(int(v) for v in kind[:cnt]))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--encoder', default='resnet18', choices=sorted(unet.ENCODER_LAYERS))
    ap.add_argument('--tiles', type=int, default=512)
    ap.add_argument('--patch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs a GPU')
    dev = torch.device('cuda:0')
    n, T = args.tiles, args.patch
    layers = unet.ENCODER_LAYERS[args.encoder]
    sd = W.make_linknet_state_dict(21, layers, 4)
    model = unet.Linknet(args.encoder, encoder_weights=None, classes=4, activation=None)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    eng = model.hip_engine(dev)
    ueng = unet.UNetEngine(W.make_unet_resnet_state_dict(21, layers, 4), dev, planes=E.PARITY)
    trunk = E.TrunkEngine({k[8:]: v for k, v in sd.items() if k.startswith('encoder.')}, dev, planes=E.PARITY, streams=1)     # (one stream: the events of this script see all of its work)
    g = torch.Generator(device=dev).manual_seed(3)
    stack = torch.randint(0, 256, (n * T, T, 3), dtype=torch.uint8, device=dev, generator=g)
    xy = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    xy[:, 1] = torch.arange(n, dtype=torch.int32, device=dev) * T
    x = E.tile_gather(stack, xy, T, T, eng.trunk.lut)

    def torch_ops():
        model.train()
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eval()
        try:
            return model(x)
        finally:
            model.eval()

    def no_tail():
        with native.conv_mode(native.ConvMode.LINKNET_NO_TAIL):
            return eng.forward_tiles(stack, xy, T, T)
    versions = {'a_hip_f32': lambda: model(x), 'b_hip_u8': lambda: eng.forward_tiles(stack, xy, T, T), 'c_hip_u8_no_tail': no_tail,
                'd_torch_ops': torch_ops, 'e_unet_hip_u8': lambda: ueng.forward_tiles(stack, xy, T, T),
                'f_trunk_hip_u8': lambda: trunk.forward_tiles(stack, xy, T, T, feat=True, logits=False)}
    res = {'what': 'Linknet on %s, parity mode, %d tiles of %d x %d, classes 4; HIP events per call, median of %d alternating steps after a warm-up'
                   % (args.encoder, n, T, T, args.steps),
           'tiles': n, 'engine_batch': eng._batch(T, T), 'workspace_bytes_per_tile': int(eng._ws_bytes(C.byref(eng.dw), 16, T, T, eng.planes) // 16),
           'unet_workspace_bytes_per_tile': int(ueng._ws_bytes(C.byref(ueng.dw), 16, T, T, ueng.planes) // 16)}
    with torch.no_grad():
        outs = {k: fn() for k, fn in versions.items()}                            # warm-up of every version and shape
        torch.cuda.synchronize()
        res['max_abs_difference_to_torch_ops'] = {k: float((outs[k] - outs['d_torch_ops']).abs().max()) for k in ('a_hip_f32', 'b_hip_u8', 'c_hip_u8_no_tail')}
        res['max_abs_logit'] = float(outs['d_torch_ops'].abs().max())
        del outs
        times = {k: [] for k in versions}
        for _ in range(args.steps):                                               # the versions alternate
            for k, fn in versions.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b))
        for k, t in times.items():
            med = float(np.median(t))
            res[k] = {'ms_median': round(med, 2), 'ms_min': round(min(t), 2), 'ms_max': round(max(t), 2), 'patches_per_s': round(n / med * 1e3, 1)}
            print(k, json.dumps(res[k]), flush=True)
        res['hip_u8_over_torch_ops'] = round(res['d_torch_ops']['ms_median'] / res['b_hip_u8']['ms_median'], 3)
        res['hip_u8_over_unet_hip_u8'] = round(res['e_unet_hip_u8']['ms_median'] / res['b_hip_u8']['ms_median'], 3)
        res['fused_tail_over_three_launches'] = round(res['c_hip_u8_no_tail']['ms_median'] / res['b_hip_u8']['ms_median'], 3)
        # per-kind shares of one profiled forward of each route (events between the launches: not an end-to-end figure)
        res['prof_fused_tail'] = _profile(eng.lib, versions['b_hip_u8'])
        res['prof_three_launches'] = _profile(eng.lib, no_tail)
    print(json.dumps({k: res[k]['share_by_kind'] for k in ('prof_fused_tail', 'prof_three_launches')}, indent=1))
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
