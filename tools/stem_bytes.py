#!/usr/bin/env python
"""One SHA-256 per stem route: a seeded 300 x 300 u8 slide (and seeded f32 tiles), seeded weights, every route
wsi_stem_pool_dispatch / wsi_stem_dispatch can take - the five StemMode values x planes 1 / 2 / 3 (+ 96-byte lines) x u8 and f32
input x tiles of 64, 192, 256, 288, 512 x 64 and 7 pooled rows per workgroup - each hashed over the WHOLE output buffer (pads and
fill included), then the U-Net's x0 route (logits, x1 and x0 of wsi_unet_forward on u8 tiles: x0 stored by the fused stem kernel, and by
the unfused conv kernel's line epilogue).  Two builds that print the same text write the same stem bytes:

    python tools/stem_bytes.py > a.txt        # on one build
    python tools/stem_bytes.py > b.txt        # on the other;  cmp a.txt b.txt

(profiles/stem_refactor_bytes_*.txt)."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wsi_segmentation_pipeline_amd import native, synthetic as W          # noqa: E402
from wsi_segmentation_pipeline_amd.engine import TrunkEngine              # noqa: E402
from wsi_segmentation_pipeline_amd.unet import UNetEngine                 # noqa: E402

TILES = (64, 192, 256, 288, 512)
ROWS = (64, 7)
ORIGINS = [(0, 0), (-5, -7), (120, 90)]          # inside; black on the left and top; past the right and bottom edge of the slide


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def stem_case(lib, eng, src, n, tile, planes, lines96, mode, rows):
    dev = eng.device
    pixels = lib.wsi_pf_bytes(n, tile // 4, tile // 4, 64, 3) // 256
    plane96 = pixels * 96
    nbytes = 2 * plane96 if lines96 else lib.wsi_pf_bytes(n, tile // 4, tile // 4, 64, planes)
    out = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)
    scratch = torch.zeros(n * (tile // 2) * (tile // 2) * 64, dtype=torch.float32, device=dev)
    wt = eng.wt
    args = src + [wt.stem_w, wt.stem_b, wt.stem_w_u8, wt.stem_b_u8, C.cast(wt.norm, C.c_void_p), n, tile, tile, scratch.data_ptr(), out.data_ptr()]
    st = torch.cuda.current_stream().cuda_stream
    with native.stem_mode(mode, rows):
        if lines96:
            rc = lib.wsi_stem_conv7x7_bn_relu_maxpool_lines96(*args, plane96, st)
        else:
            rc = lib.wsi_stem_conv7x7_bn_relu_maxpool(*args, planes, st)
    return sha(out) if rc == 0 else 'rc %d' % rc


def main():
    lib = native.load()
    dev = torch.device('cuda:0')
    slide = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (300, 300, 3), dtype=np.uint8)).to(dev)
    xy = torch.tensor(ORIGINS, dtype=torch.int32, device=dev)
    n = len(ORIGINS)
    sd = W.make_resnet18_state_dict(11, with_fc=False)
    engines = {p: TrunkEngine(sd, dev, planes=p) for p in (1, 2, 3)}
    for tile in TILES:
        x = torch.from_numpy(np.random.default_rng(tile).standard_normal((n, 3, tile, tile)).astype(np.float32)).to(dev)
        for kind in ('u8', 'f32'):
            for planes, lines96 in ((1, False), (2, False), (3, False), (3, True)):
                eng = engines[planes]
                if kind == 'u8':
                    src = [None, slide.data_ptr(), slide.stride(0), slide.shape[0], slide.shape[1], xy.data_ptr(), eng.lut.data_ptr()]
                else:
                    src = [x.data_ptr(), None, 0, 0, 0, None, None]
                for mode in native.StemMode:
                    for rows in ROWS:
                        print('%-3s tile %3d planes %d lines96 %d %-15s rows %2d  %s' % (
                            kind, tile, planes, lines96, mode.name, rows, stem_case(lib, eng, src, n, tile, planes, lines96, mode, rows)), flush=True)
    # the U-Net's half-resolution skip x0 (planes 2, u8 tiles): stored by the fused stem kernel, or by the unfused conv kernel as PF lines
    ueng = UNetEngine(W.make_unet_state_dict(9, 3), dev, planes=2)
    for tile in TILES:
        for mode in native.StemMode:
            for rows in ROWS:
                for unfused_x0 in (False, True):
                    try:
                        with native.stem_mode(mode, rows), native.conv_mode(native.ConvMode.UNET_X0_UNFUSED if unfused_x0 else 0):
                            logits, enc = ueng._run(n, tile, tile, None, slide, xy, True, True)
                        res = 'logits %s x1 %s x0 %s' % (sha(logits), sha(enc[3]), sha(enc[4]))
                    except RuntimeError as e:                    # a shape the U-Net entry declines: its return code is the result
                        res = str(e).split(' (')[0]
                    print('x0  tile %3d %-15s rows %2d x0_unfused %d  %s' % (tile, mode.name, rows, unfused_x0, res), flush=True)


if __name__ == '__main__':
    main()
