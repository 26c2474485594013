#!/usr/bin/env python
"""What the host layer of the trunks (csrc/trunk.hip, engine.py) makes the kernels compute, as text: seeded synthetic weights,
BasicBlock nets [1,1,1,1], [2,2,2,2], [3,4,6,3] and Bottleneck nets [1,1,1,1], [3,4,6,3], every planes value the architecture
takes, the f32 route and the u8 slide route.  Per case the SHA-256 of features, logits, feature map and every tap, and the ordered
(kind, FLOPs) records wsi_prof_begin / wsi_prof_end return for the full run: 3 images of 64 x 64, then 2 images on the same engine
(the smaller batch in the larger workspace); the mx BasicBlock nets also on 2 images of 256 x 256 (96-byte lines and the row-stacked
layer 1 are reachable only there), full run, taps, full run again (the workspace changes its line layout twice).  Last the U-Net on
[2,2,2,2] in parity mode.  Two builds that print the same text launch the same kernels on the same bytes in the same order:

    python tools/trunk_bytes.py > a.txt        # on one build
    python tools/trunk_bytes.py > b.txt        # on the other;  cmp a.txt b.txt

(profiles/trunk_host_refactor_bytes_*.txt).  Every case runs once; the first failure ends the process."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wsi_segmentation_pipeline_amd import native, engine as E, synthetic as W      # noqa: E402
from wsi_segmentation_pipeline_amd.unet import UNetEngine                           # noqa: E402

NETS = [('basic', [1, 1, 1, 1]), ('basic', [2, 2, 2, 2]), ('basic', [3, 4, 6, 3]), ('bottleneck', [1, 1, 1, 1]), ('bottleneck', [3, 4, 6, 3])]
PLANES = {'basic': (1, 2, 3), 'bottleneck': (1, 2)}
RECS = 256


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def profiled(lib, run):
    """(what run() returns, its profiler records as text)"""
    native.check(lib.wsi_prof_begin(RECS), 'wsi_prof_begin')
    try:
        out = run()
    finally:
        ms, kind, fl = np.zeros(RECS, np.float32), np.zeros(RECS, np.int32), np.zeros(RECS, np.float64)
        n = lib.wsi_prof_end(*[a.ctypes.data_as(C.c_void_p) for a in (ms, kind, fl)], RECS)
    if not 0 <= n < RECS:
        raise RuntimeError('wsi_prof_end returned %d' % n)
    return out, '%d records: %s' % (n, ' '.join('%d:%d' % (kind[i], int(fl[i])) for i in range(n)))


def sources(dev, n, tile):
    """the two input routes of n tiles: ('f32', forward_f32 arguments), ('u8', forward_tiles arguments)"""
    g = torch.Generator().manual_seed(100 * tile + n)
    x = torch.randn(n, 3, tile, tile, generator=g).to(dev)
    slide = torch.randint(0, 256, (tile + 40, 2 * tile + 24, 3), dtype=torch.uint8, generator=g).to(dev)
    xy = torch.stack([torch.randint(0, tile + 24, (n,), generator=g), torch.randint(0, 40, (n,), generator=g)], 1).to(torch.int32).to(dev)
    return [('f32', lambda eng, **kw: eng.forward_f32(x, **kw)), ('u8 ', lambda eng, **kw: eng.forward_tiles(slide, xy, tile, tile, **kw))]


def full(lib, eng, fwd, what):
    (feat, logits, fmap), recs = profiled(lib, lambda: fwd(eng, feat=True, logits=True, fmap=True))
    print('%s  feat %s  logits %s  fmap %s' % (what, sha(feat), sha(logits), sha(fmap)), flush=True)
    print('%s  %s' % (what, recs), flush=True)
    return sha(feat), sha(logits), sha(fmap)


def taps(eng, fwd, what):
    for tap in range(sum(eng.layers) + 1):
        t = fwd(eng, tap=tap)
        print('%s  tap %2d %-18s %s' % (what, tap, tuple(t.shape), sha(t)), flush=True)


def main():
    lib = native.load()
    dev = torch.device('cuda:0')
    for arch, layers in NETS:
        make, cls = (W.make_resnet_state_dict, E.TrunkEngine) if arch == 'basic' else (W.make_bottleneck_state_dict, E.BottleneckEngine)
        sd = make(11, layers, with_fc=False)
        for planes in PLANES[arch]:
            eng = cls(sd, dev, planes=planes, head=(sd['fc0.weight'], sd['fc0.bias']))
            name = '%-10s %-12s planes %d' % (arch, layers, planes)
            for n in (3, 2):
                for route, fwd in sources(dev, n, 64):
                    what = '%s  %s n %d  64' % (name, route, n)
                    full(lib, eng, fwd, what)
                    taps(eng, fwd, what)
            if arch == 'basic' and planes == 3:
                for route, fwd in sources(dev, 2, 256):
                    what = '%s  %s n 2 256' % (name, route)
                    first = full(lib, eng, fwd, what)
                    taps(eng, fwd, what)
                    if full(lib, eng, fwd, what + ' again') != first:
                        raise RuntimeError('%s: the run after the taps differs from the run before them' % what)
            eng.release_workspaces()
    unet = UNetEngine(W.make_unet_state_dict(7, 4), dev, planes=E.PARITY)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 3, 64, 64, generator=g).to(dev)
    (logits, enc), recs = profiled(lib, lambda: unet.forward_f32(x, enc=True))
    print('unet [2, 2, 2, 2] planes 2  f32 n 3  64  logits %s  enc %s' % (sha(logits), ' '.join(sha(t) for t in enc)), flush=True)
    print('unet [2, 2, 2, 2] planes 2  f32 n 3  64  %s' % recs, flush=True)
    slide = torch.randint(0, 256, (104, 152, 3), dtype=torch.uint8, generator=g).to(dev)
    xy = torch.tensor([[0, 0], [88, 40], [31, 17]], dtype=torch.int32, device=dev)
    logits, recs = profiled(lib, lambda: unet.forward_tiles(slide, xy[:2], 64, 64))
    print('unet [2, 2, 2, 2] planes 2  u8  n 2  64  logits %s' % sha(logits), flush=True)
    print('unet [2, 2, 2, 2] planes 2  u8  n 2  64  %s' % recs, flush=True)


if __name__ == '__main__':
    main()
