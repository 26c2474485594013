#!/usr/bin/env python3
"""Patches per second of the U-Net on a ResNet-50 encoder (parity mode, 256 x 256 tiles): the HIP path against the two ways a caller
could run this model without it.

  python tools/unet_bottleneck_times.py [--encoder resnet50] [--tiles 128] [--patch 256] [--steps 7] [--out profiles/unet_resnet50_bench.json]

Four versions alternate in one process, each call timed with HIP events (median of --steps calls after a warm-up of every version, with
the spread):
  (a) hip_f32      model(x) in eval mode: wsi_unet_bneck_forward on normalised fp32 tiles
  (b) hip_u8       UNetEngine.forward_tiles: the same launches fed from a device-resident u8 slide (the product path of utils.eval)
  (c) torch_ops    the same module's torch-op forward (training-mode code path with BatchNorm in eval mode) on the same GPU
  (d) taps_torch   what there was before the U-Net entries took Bottleneck encoders: the HIP Bottleneck trunk for the encoder maps (one
                   wsi_bneck_forward_tap call per map - a tap call runs the net up to that block - and x0 with torch ops), then the
                   module's torch-op decoder
Then one profiled forward of (a) (wsi_prof_begin / wsi_prof_end, a run of its own): the time share of every record kind
(4 stem + pool, 11 pointwise 1x1, 1 / 2 3x3 stride 1 / 2, 3 strided 1x1 downsample, 7 x0 stem conv, 6 decoder 3x3, 10 fused tail).
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

KINDS = {1: '3x3 stride 1 (encoder)', 2: '3x3 stride 2 (encoder)', 3: '1x1 stride-2 downsample', 4: 'stem + max pool', 6: 'decoder 3x3 conv',
         7: 'x0 stem conv / concat glue', 8: '1x1 head', 9: 'refused fused launch', 10: 'fused tail (block 5 + head)', 11: 'pointwise 1x1 (encoder)'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--encoder', default='resnet50', choices=sorted(unet.BOTTLENECK_ENCODER_LAYERS))
    ap.add_argument('--tiles', type=int, default=128)
    ap.add_argument('--patch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs a GPU')
    dev = torch.device('cuda:0')
    n, T = args.tiles, args.patch
    layers = unet.BOTTLENECK_ENCODER_LAYERS[args.encoder]
    sd = W.make_unet_bottleneck_state_dict(21, layers, 4)
    for key in ('decoder.final_conv.weight', 'decoder.final_conv.bias'):          # logits of the size trained heads give (bench.py --workload seg)
        sd[key] = sd[key] * (8.0 / 216.0)
    model = unet.Unet(args.encoder, encoder_weights=None, classes=4, activation=None)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    eng = model.hip_engine(dev)
    trunk = E.BottleneckEngine({k[8:]: v for k, v in sd.items() if k.startswith('encoder.')}, dev, planes=E.PARITY)
    taps = [sum(layers[:s + 1]) for s in (3, 2, 1, 0)]                           # the last block of layer4..1, network order
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

    def taps_torch():
        enc = [trunk.forward_f32(x, tap=t) for t in taps]
        model.train()
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eval()
        try:
            e = model.encoder
            return model.decoder(enc + [e.relu(e.bn1(e.conv1(x)))])
        finally:
            model.eval()
    versions = {'a_hip_f32': lambda: model(x), 'b_hip_u8': lambda: eng.forward_tiles(stack, xy, T, T), 'c_torch_ops': torch_ops, 'd_taps_torch': taps_torch}
    res = {'what': 'U-Net on %s, parity mode, %d tiles of %d x %d, classes 4; HIP events per call, median of %d alternating steps after a warm-up'
                   % (args.encoder, n, T, T, args.steps),
           'tiles': n, 'engine_batch': eng._batch(T, T), 'workspace_bytes_per_tile': int(eng._ws_bytes(C.byref(eng.dw), 16, T, T, eng.planes) // 16)}
    with torch.no_grad():
        outs = {k: fn() for k, fn in versions.items()}                            # warm-up of every version and shape
        torch.cuda.synchronize()
        res['max_abs_difference_to_torch_ops'] = {k: float((outs[k] - outs['c_torch_ops']).abs().max()) for k in versions if k != 'c_torch_ops'}
        res['max_abs_logit'] = float(outs['c_torch_ops'].abs().max())
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
        res['hip_f32_over_torch_ops'] = round(res['c_torch_ops']['ms_median'] / res['a_hip_f32']['ms_median'], 3)
        res['hip_f32_over_taps_torch'] = round(res['d_taps_torch']['ms_median'] / res['a_hip_f32']['ms_median'], 3)
        # per-kind shares of one profiled forward (events between the launches: not an end-to-end figure)
        cap = 4096
        native.check(eng.lib.wsi_prof_begin(cap), 'wsi_prof_begin')
        try:
            model(x)
        finally:
            ms, kind, fl = np.zeros(cap, np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
            cnt = eng.lib.wsi_prof_end(*[a.ctypes.data_as(C.c_void_p) for a in (ms, kind, fl)], cap)
        total = float(ms[:cnt].sum())
        res['prof_records'] = int(cnt)
        res['prof_ms_total'] = round(total, 3)
        res['prof_share_by_kind'] = {'%d %s' % (k, KINDS.get(k, '?')): {'launches': int((kind[:cnt] == k).sum()), 'ms': round(float(ms[:cnt][kind[:cnt] == k].sum()), 3),
                                                                       'share': round(float(ms[:cnt][kind[:cnt] == k].sum()) / total, 4)}
                                     for k in sorted(set(int(v) for v in kind[:cnt]))}
    print(json.dumps(res['prof_share_by_kind'], indent=1))
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
