#!/usr/bin/env python
"""What the host layer of the segmentation models (unet.py over csrc/seg_host.h and the decoder files) makes the kernels compute, as text, in the style of
tools/trunk_bytes.py: seeded synthetic weights; the U-Net on ResNet-18 at planes 1, 2, 3, the U-Net on a Bottleneck [1, 1, 1, 1]
encoder at planes 1, 2, the Linknet on ResNet-18 at planes 1, 2, and the FPN and the PSPNet on ResNet-18 and on a Bottleneck
[1, 1, 1, 1] encoder at planes 1, 2, each with 4 classes and again with 5 (no fused tail: the plain last block + head).  Per case, on
one engine: forward_f32 with the encoder maps on 3 tiles of 64 x 64 (the smallest shape with all five
decoder levels and both fused tails), 2 tiles on the same engine (the smaller batch in the larger workspace), forward_tiles on 2 tiles
of a seeded u8 slide, and decode() on the encoder maps of the first call.  Last the parity U-Net on 2 tiles of 64 x 96, whose fourth
decoder level is 48 wide, so the fused tail does not apply with 4 classes either, the parity FPN and PSPNet on ResNet-18 on the same
tiles, and one PSPNet forward_f32 without the encoder maps (the encoder stops after layer 2).  Per run the SHA-256 of every output and
the ordered (kind, FLOPs) records of wsi_prof_begin / wsi_prof_end.  Two builds that print the same text launch the same kernels on the same bytes
in the same order:

    python tools/seg_bytes.py > a.txt        # on one build
    python tools/seg_bytes.py > b.txt        # on the other;  cmp a.txt b.txt

(profiles/seg_host_refactor_bytes_*.txt, profiles/seg_models_refactor_bytes_*.txt).  The file names nothing that the tree before
native.profiled lacks, so one copy of it runs on both sides of that change.  Every case runs once; the first failure ends the process."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wsi_segmentation_pipeline_amd import native, synthetic as W                    # noqa: E402
from wsi_segmentation_pipeline_amd.unet import FPNEngine, LinknetEngine, PSPNetEngine, UNetEngine            # noqa: E402

CASES = [('unet resnet18', UNetEngine, lambda c: W.make_unet_state_dict(7, c), (1, 2, 3)),
         ('unet bottleneck [1, 1, 1, 1]', UNetEngine, lambda c: W.make_unet_bottleneck_state_dict(7, [1, 1, 1, 1], c), (1, 2)),
         ('linknet resnet18', LinknetEngine, lambda c: W.make_linknet_state_dict(7, classes=c), (1, 2)),
         ('fpn resnet18', FPNEngine, lambda c: W.make_fpn_state_dict(7, classes=c), (1, 2)),
         ('fpn bottleneck [1, 1, 1, 1]', FPNEngine, lambda c: W.make_fpn_bottleneck_state_dict(7, [1, 1, 1, 1], c), (1, 2)),
         ('pspnet resnet18', PSPNetEngine, lambda c: W.make_pspnet_state_dict(7, classes=c), (1, 2)),
         ('pspnet bottleneck [1, 1, 1, 1]', PSPNetEngine, lambda c: W.make_pspnet_bottleneck_state_dict(7, [1, 1, 1, 1], c), (1, 2))]
WIDE = [('unet resnet18', UNetEngine, W.make_unet_state_dict), ('fpn resnet18', FPNEngine, lambda s, c: W.make_fpn_state_dict(s, classes=c)),
        ('pspnet resnet18', PSPNetEngine, lambda s, c: W.make_pspnet_state_dict(s, classes=c))]      # the 64 x 96 cases
RECS = 256


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def profiled(lib, run):
    """(what run() returns, its profiler records as text)"""
    if hasattr(native, 'profiled'):
        out, recs = native.profiled(run, RECS)
    else:                                                  # a tree from before native.profiled: the same calls, spelled out
        import ctypes as C
        native.check(lib.wsi_prof_begin(RECS), 'wsi_prof_begin')
        try:
            out = run()
        finally:
            ms, kind, fl = np.zeros(RECS, np.float32), np.zeros(RECS, np.int32), np.zeros(RECS, np.float64)
            n = lib.wsi_prof_end(*[a.ctypes.data_as(C.c_void_p) for a in (ms, kind, fl)], RECS)
        if not 0 <= n < RECS:
            raise RuntimeError('wsi_prof_end returned %d' % n)
        recs = [(int(kind[i]), float(fl[i])) for i in range(n)]
    return out, '%d records: %s' % (len(recs), ' '.join('%d:%d' % (k, int(f)) for k, f in recs))


def inputs(dev, n, h, w):
    """n normalised fp32 tiles of h x w; a u8 slide and n tile corners in it"""
    g = torch.Generator().manual_seed(1000 * h + 10 * w + n)
    x = torch.randn(n, 3, h, w, generator=g).to(dev)
    slide = torch.randint(0, 256, (h + 40, 2 * w + 24, 3), dtype=torch.uint8, generator=g).to(dev)
    xy = torch.stack([torch.randint(0, w + 24, (n,), generator=g), torch.randint(0, 40, (n,), generator=g)], 1).to(torch.int32).to(dev)
    return x, slide, xy


def report(lib, what, run):
    out, recs = profiled(lib, run)
    logits, enc = out if isinstance(out, tuple) else (out, None)
    print('%s  logits %-18s %s%s' % (what, tuple(logits.shape), sha(logits), '' if enc is None else '  enc ' + ' '.join(sha(t) for t in enc)),
          flush=True)
    print('%s  %s' % (what, recs), flush=True)
    return enc


def main():
    lib = native.load()
    dev = torch.device('cuda:0')
    for name, cls, make, planes_of in CASES:
        for classes in (4, 5):
            sd = make(classes)
            for planes in planes_of:
                eng = cls(sd, dev, planes=planes, classes=classes)
                what = '%-28s planes %d classes %d' % (name, planes, classes)
                n = len(eng.dw.cin)
                print('%s  cin %s cout %s head_cin %d classes %d tail %s' % (what, eng.dw.cin[:n], eng.dw.cout[:n], getattr(eng.dw, 'head_cin', 0),
                                                                            eng.dw.classes, bool(getattr(eng.dw, 'tail_w', None))), flush=True)
                x3, _, _ = inputs(dev, 3, 64, 64)
                x2, slide, xy = inputs(dev, 2, 64, 64)
                enc = report(lib, what + '  f32 n 3', lambda: eng.forward_f32(x3, enc=True))
                report(lib, what + '  f32 n 2', lambda: eng.forward_f32(x2, enc=True))
                report(lib, what + '  u8  n 2', lambda: eng.forward_tiles(slide, xy, 64, 64))
                report(lib, what + '  decode ', lambda: eng.decode(enc))
                eng.release_workspaces()
    for name, cls, make in WIDE:
        eng = cls(make(7, 4), dev, planes=2, classes=4)
        x, slide, xy = inputs(dev, 2, 64, 96)
        what = '%-28s planes 2 classes 4  64 x 96' % name
        report(lib, what + '  f32 n 2', lambda: eng.forward_f32(x, enc=True))
        report(lib, what + '  u8  n 2', lambda: eng.forward_tiles(slide, xy, 64, 96))
        eng.release_workspaces()
    eng = PSPNetEngine(W.make_pspnet_state_dict(7, classes=4), dev, planes=2, classes=4)
    x3, _, _ = inputs(dev, 3, 64, 64)
    report(lib, '%-28s planes 2 classes 4  no enc   f32 n 3' % 'pspnet resnet18', lambda: eng.forward_f32(x3)[0])
    eng.release_workspaces()


if __name__ == '__main__':
    main()
