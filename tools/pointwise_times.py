#!/usr/bin/env python3
"""Times of the pointwise-conv kernel (csrc/conv_pw.hip) against the gather kernel it replaces, and of a whole ResNet-50 pass.

  python tools/pointwise_times.py [--planes 2] [--reps 7] [--out profiles/resnet50_pointwise.json]
  python tools/pointwise_times.py --whole-net [--out profiles/resnet50_bench.json]

Shapes: the twelve stride-1 1x1 convs of ResNet-50 at 256 x 256 patches (conv1 / conv3 of every stage, layer 1's downsample, and conv1
of the strided blocks, which runs at the previous stage's map size).  N is chosen per shape so that input + output exceed 1.25 x the
256 MiB Infinity Cache, and three sets of buffers rotate, so no launch re-reads what an earlier one left in a cache.  Each launch is
timed with HIP events; the figure is the median of --reps launches after two warm-up launches, with the spread (min, max).  Both routes
run in the same process: the default dispatch and ConvMode.PW_GATHER (the gather kernel, the route before this kernel).  The
default dispatch sends 64-channel outputs to the gather kernel too (csrc/conv_pw.hip): those rows say dispatch = gather and both
columns time the same kernel (the figures that decided it are kept in profiles/resnet50_pointwise.json under "cout64_study").
Bytes are algorithmic: input + output (+ residual) once each, over real pixels; the ceiling is the 6.29 TB/s copy rate measured on
this chip.

--whole-net: patches/s of ResNet-50 in parity mode on u8 slide input, 256 x 256 tiles, through an engine as callers get it (its own
batch cap and its two streams), and the profiler's per-kind totals of ONE batch on ONE stream (an engine with streams=1 and the
same batch size as one of the first engine's batches), so that the per-kind times add up (kind 11 = stride-1 1x1 convs).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wsi_segmentation_pipeline_amd import engine as E, native, synthetic as W  # noqa: E402

COPY_CEILING = 6.29e12            # bytes/s, measured device copy rate of an MI355X
CACHE = 256 << 20
# (name, cin, cout, map side at 256 x 256 patches, residual)
SHAPES = [
    ('layer1.0.conv1', 64, 64, 64, False), ('layer1.0.conv3 / downsample', 64, 256, 64, True), ('layer1.1.conv1', 256, 64, 64, False),
    ('layer2.0.conv1', 256, 128, 64, False), ('layer2.1.conv1', 512, 128, 32, False), ('layer2.x.conv3', 128, 512, 32, True),
    ('layer3.0.conv1', 512, 256, 32, False), ('layer3.1.conv1', 1024, 256, 16, False), ('layer3.x.conv3', 256, 1024, 16, True),
    ('layer4.0.conv1', 1024, 512, 16, False), ('layer4.1.conv1', 2048, 512, 8, False), ('layer4.x.conv3', 512, 2048, 8, True),
]


def time_shape(dev, planes, cin, cout, side, resid, reps, sets=3):
    bpc = 2 if planes == 1 else 4
    per_patch = side * side * (cin + cout) * bpc
    n = max(16, -(-int(1.25 * CACHE) // per_patch))
    g = torch.Generator(device=dev).manual_seed(cin + cout)
    wt = torch.randn(cout, cin, 1, 1) * (2.0 / cin) ** 0.5
    wpk, bias = E.prepack_conv(wt, None, planes, dev)
    bufs = []
    for _ in range(sets):
        x = E.pf_pack(torch.randn(n, cin, side, side, device=dev, generator=g).abs_(), planes)
        r = E.pf_pack(torch.randn(n, cout, side, side, device=dev, generator=g), planes) if resid else None
        bufs.append((x, r, E.pf_zeros(n, cout, side, side, planes, dev)))
    out = {}
    for route, mode in (('pointwise', 0), ('gather', native.ConvMode.PW_GATHER)):
        ms = []
        with native.conv_mode(mode):
            for i in range(reps + 2):
                x, r, o = bufs[i % sets]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                E.conv1x1_bn_act(x, n, side, side, cin, cout, wpk, bias, 1, r, True, planes, out=o)
                b.record()
                b.synchronize()
                if i >= 2:
                    ms.append(a.elapsed_time(b))
        out[route] = ms
        if route == 'pointwise':
            keep = [o.clone() for _, _, o in bufs]
        else:                                                # the two kernels add the K lines in the same order: equal to the bit
            out['equal'] = all(torch.equal(k, o) for k, (_, _, o) in zip(keep, bufs))
    nbytes = n * side * side * (cin + cout * (2 if resid else 1)) * bpc
    return n, nbytes, out


def shapes_main(args, dev):
    rows = []
    for name, cin, cout, side, resid in SHAPES:
        n, nbytes, t = time_shape(dev, args.planes, cin, cout, side, resid, args.reps)
        row = {'conv': name, 'cin': cin, 'cout': cout, 'map': side, 'residual': resid, 'n': n, 'algorithmic_bytes': nbytes}
        for route in ('pointwise', 'gather'):
            med = float(np.median(t[route]))
            row[route] = {'ms_median': round(med, 4), 'ms_min': round(min(t[route]), 4), 'ms_max': round(max(t[route]), 4),
                          'GBps': round(nbytes / med / 1e6, 1), 'of_copy_ceiling': round(nbytes / (med * 1e-3) / COPY_CEILING, 3)}
        row['speedup'] = round(row['gather']['ms_median'] / row['pointwise']['ms_median'], 2)
        # at least as fast beyond the spread of the repetitions: the slowest pointwise launch against the fastest gather launch
        row['faster_beyond_spread'] = bool(row['pointwise']['ms_max'] <= row['gather']['ms_min'])
        row['dispatch'] = 'pointwise' if cout % 128 == 0 else 'gather (by shape: 64-channel outputs, see csrc/conv_pw.hip)'
        row['bit_identical_to_gather'] = bool(t['equal'])
        rows.append(row)
        print('%-30s %4d -> %4d  %2dx%-2d n %4d  pointwise %7.3f ms (%6.1f GB/s, %4.1f %% of copy)  gather %7.3f ms  x%.2f %s'
              % (name, cin, cout, side, side, n, row['pointwise']['ms_median'], row['pointwise']['GBps'], 100 * row['pointwise']['of_copy_ceiling'],
                 row['gather']['ms_median'], row['speedup'], ('' if row['faster_beyond_spread'] else '(inside the spread)') + ('' if t['equal'] else ' DIFFERS FROM GATHER')), flush=True)
    return {'what': 'stride-1 1x1 convs of ResNet-50 at 256 x 256 patches, planes %d: pointwise kernel vs gather kernel (ConvMode.PW_GATHER), HIP-event '
                    'median of %d launches, rotating buffers, input + output > 1.25 x 256 MiB' % (args.planes, args.reps),
            'copy_ceiling_Bps': COPY_CEILING, 'planes': args.planes, 'shapes': rows}


def whole_net_main(args, dev):
    lib = native.load()
    sd = W.make_bottleneck_state_dict(21, list(W.RESNET50_LAYERS), with_fc=False)
    eng = E.BottleneckEngine(sd, dev, planes=args.planes, head=(sd['fc0.weight'], sd['fc0.bias']))
    T = 256
    n = cap = eng._auto_cap(T, T)
    g = torch.Generator(device=dev).manual_seed(3)
    side = int(np.ceil(np.sqrt(n)))
    slide = torch.randint(0, 256, (-(-n // side) * T, side * T, 3), dtype=torch.uint8, device=dev, generator=g)
    xy = torch.tensor([[T * (i % side), T * (i // side)] for i in range(n)], dtype=torch.int32, device=dev)
    sizes = E.batch_sizes(n, eng._auto_cap(T, T), T, T)         # what forward_tiles will do with the slide resident
    res = {'what': 'ResNet-50 ([3, 4, 6, 3] Bottleneck), planes %d, u8 slide input, 256 x 256 tiles, head Linear(2048 -> 4): %d tiles per call, which the '
                   'engine runs as batches of %s (BottleneckEngine._auto_cap) over its two streams; kernel_ms_by_kind: one batch of %d on one stream'
                   % (args.planes, n, sizes, max(sizes)), 'tiles': n, 'batches': sizes,
           'workspace_bytes_per_patch': int(lib.wsi_bneck_workspace_bytes(64, T, T, args.planes) // 64)}
    nb = max(sizes)
    one = E.BottleneckEngine(sd, dev, planes=args.planes, head=(sd['fc0.weight'], sd['fc0.bias']), streams=1, max_batch=nb)
    for route, mode in (('pointwise', 0), ('gather', native.ConvMode.PW_GATHER)):
        with native.conv_mode(mode):
            eng.forward_tiles(slide, xy, T, T, logits=True)
            torch.cuda.synchronize()
            times = []
            for _ in range(args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                eng.forward_tiles(slide, xy, T, T, logits=True)
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
            eng.release_workspaces()
            one.forward_tiles(slide, xy[:nb], T, T, logits=True)
            torch.cuda.synchronize()
            recs = 128
            native.check(lib.wsi_prof_begin(recs), 'wsi_prof_begin')
            one.forward_tiles(slide, xy[:nb], T, T, logits=True)
            torch.cuda.synchronize()
            ms, kind, fl = np.zeros(recs, np.float32), np.zeros(recs, np.int32), np.zeros(recs, np.float64)
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            k = lib.wsi_prof_end(p(ms), p(kind), p(fl), recs)
            one.release_workspaces()
        med = float(np.median(times))
        kinds = {}
        for i in range(k):
            e = kinds.setdefault(int(kind[i]), {'launches': 0, 'ms': 0.0, 'flops': 0.0})
            e['launches'] += 1; e['ms'] += float(ms[i]); e['flops'] += float(fl[i])
        res[route] = {'ms_per_call_median': round(med, 2), 'ms_steps': [round(t, 2) for t in times], 'patches_per_s': round(n / med * 1e3, 1),
                      'kernel_ms_by_kind': {str(kk): {'launches': v['launches'], 'ms': round(v['ms'], 3), 'TFLOPs': round(v['flops'] / max(v['ms'], 1e-9) / 1e9, 1)}
                                            for kk, v in sorted(kinds.items())},
                      'kernel_ms_batch': nb, 'kernel_ms_sum': round(float(ms[:k].sum()), 3)}
        print(route, json.dumps(res[route]), flush=True)
    res['kinds'] = {'1': '3x3 stride 1', '2': '3x3 stride 2', '3': '1x1 stride-2 downsample (gather kernel)', '4': 'stem + maxpool', '11': 'stride-1 1x1 (pointwise kernel)'}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--planes', type=int, default=2)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--whole-net', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = whole_net_main(args, dev) if args.whole_net else shapes_main(args, dev)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
