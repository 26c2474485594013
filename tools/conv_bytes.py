#!/usr/bin/env python
"""One SHA-256 per conv route: seeded inputs and weights, every tile configuration the product build dispatches through
wsi_conv3x3_bn_act_cfg (x planes; residual on / off x ReLU on / off on the shapes of tests/test_gpu_conv_routes.py), the default
dispatch, the phase-split writer, the stride-2 block entries under their ConvMode bases, the 1x1 conv and the fused upsample +
concat conv - each case hashed over the WHOLE output buffer (pads and guards included, pre-filled with 0xAB; a return code counts
as a result), a route's line being the SHA-256 over its cases' results in run order - then the logits and features of a 2-image mx
trunk at 64- and 256-pixel patches under the default mode and each route switch taken singly (the 96-byte-line paths are reachable
only there).  Two builds that print the same text write the same conv bytes:

    python tools/conv_bytes.py > a.txt        # on one build
    python tools/conv_bytes.py > b.txt        # on the other;  cmp a.txt b.txt

(profiles/conv_refactor_bytes_*.txt).  --cases prints every case's own line as well (1600 lines: to find the case behind a route
that differs).  Every case runs once; the first failure ends the process."""
import ctypes as C
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wsi_segmentation_pipeline_amd import native, engine as E, synthetic as W      # noqa: E402
from wsi_segmentation_pipeline_amd.native import ConvMode as M                      # noqa: E402

CFG_PLANES = {30: (1, 2, 3), 31: (1, 2, 3), 38: (3,), 39: (1, 2, 3), 40: (3,), 41: (3,), 60: (1, 2, 3), 70: (1, 2, 3), 71: (1, 2, 3),
              72: (1, 3), 73: (1, 3), 74: (1, 3), 77: (1, 3), 78: (1, 3), 83: (2,), 90: (2, 3), 91: (2, 3)}
SHAPES = [(3, 64, 64, 5, 7), (3, 128, 128, 5, 7), (5, 128, 128, 8, 8), (9, 128, 256, 4, 4), (1, 64, 64, 8, 64), (3, 64, 128, 4, 64),
          (1, 64, 64, 6, 64), (1, 64, 64, 3, 130), (2, 32, 32, 5, 40), (2, 256, 256, 16, 16)]          # n, cin, cout, h, w
S2_SHAPES = [(3, 64, 128, 16, 16), (2, 64, 128, 64, 64), (5, 256, 512, 4, 4), (1, 64, 128, 80, 80), (1, 64, 128, 2, 2)]
UP_SHAPES = [(2, 64, 64, 64, 8, 16), (2, 64, 0, 128, 8, 16), (3, 64, 32, 32, 6, 10), (1, 64, 64, 64, 4, 136)]   # n, c_up, c_skip, cout, h, w
TRUNK_MODES = (0, M.XCD_ORDER, M.XCD_RANGES_OFF, M.XCD_RANGES_L1, M.L1_SLAB3, M.L1_LINES128, M.L1_PERSISTENT, M.NO_SLAB_PAIR,
               M.WIDE_NO_D8, M.WIDE_NEVER, M.NO_DS_FOLD, M.NO_S2_SPLIT)
dev = None
CASES = '--cases' in sys.argv
routes = {}            # route name -> (running SHA-256 over its cases' results, cases, cases that returned a code); printed in first-use order


def case(route, what, res):
    """One case's result (hashes or 'rc N') joins its route's line."""
    h = routes.setdefault(route, [hashlib.sha256(), 0, 0])
    h[0].update(('%s %s\n' % (what, res)).encode())
    h[1] += 1
    h[2] += res.startswith('rc ')
    if CASES:
        print('  %-28s %-44s %s' % (route, what, res), flush=True)


def report():
    for route, (h, n, nrc) in routes.items():
        print('%-28s %3d cases (%3d return codes)  %s' % (route, n, nrc, h.hexdigest()), flush=True)
    routes.clear()


def sha(*ts):
    torch.cuda.synchronize()
    return ' '.join(hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in ts)


def rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def fill(nbytes):
    return torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)


def weights(seed, cout, cin, k, planes):
    g = torch.Generator().manual_seed(seed)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    bn = (torch.rand(cout, generator=g) * 0.5 + 0.75, torch.randn(cout, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1,
          torch.rand(cout, generator=g) * 0.5 + 0.75)
    return E.prepack_conv(wt, bn, planes, dev)


def result(rc, *outs):
    return sha(*outs) if rc == 0 else 'rc %d' % rc


def main():
    global dev
    lib = native.load()
    dev = torch.device('cuda:0')
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: t.data_ptr() if t is not None else None
    for shape in SHAPES:
        n, cin, cout, h, w = shape
        for planes in (1, 2, 3):
            if lib.wsi_prepack_conv_bytes(cout, cin, 3, planes) == 0:
                continue
            wpk, bias = weights(sum(shape), cout, cin, 3, planes)
            xpf = E.pf_pack(rand(1, n, cin, h, w).abs_().to(dev), planes)
            rpf = E.pf_pack(rand(2, n, cout, h, w).to(dev), planes)
            nbytes = lib.wsi_pf_bytes(n, h, w, cout, planes)
            for cfg in [-1] + [c for c, acc in CFG_PLANES.items() if planes in acc]:          # -1: wsi_conv3x3_bn_act, the default dispatch
                for resid in (None, rpf):
                    for relu in (0, 1):
                        out = fill(nbytes)
                        if cfg < 0:
                            rc = lib.wsi_conv3x3_bn_act(P(xpf), P(out), P(resid), P(wpk), P(bias), n, h, w, cin, cout, 1, relu, planes, st)
                        else:
                            rc = lib.wsi_conv3x3_bn_act_cfg(P(xpf), P(out), P(resid), P(wpk), P(bias), n, h, w, cin, cout, 1, relu, planes, cfg, st)
                        case('s1 cfg %2d planes %d' % (cfg, planes) if cfg >= 0 else 's1 default planes %d' % planes,
                             '%s resid %d relu %d' % (shape, resid is not None, relu), result(rc, out))
            if planes >= 2 and h % 2 == 0 and w % 2 == 0 and cin == cout:                          # the phase-split writer (residual = the input)
                out = fill(lib.wsi_pf_split_bytes(n, h, w, cout, planes))
                rc = lib.wsi_conv3x3_bn_act_split(P(xpf), P(out), P(xpf), P(wpk), P(bias), n, h, w, cin, cout, 1, planes, st)
                case('split writer planes %d' % planes, str(shape), result(rc, out))
    report()
    for shape in S2_SHAPES:
        n, cin, cout, h, w = shape
        for planes in (1, 2, 3):
            wp3, b3 = weights(3, cout, cin, 3, planes)
            wp1, b1 = weights(4, cout, cin, 1, planes)
            wp0, b0 = weights(5, cin, cin, 3, planes)
            xpf = E.pf_pack(rand(6, n, cin, h, w).abs_().to(dev), planes)
            nbytes = lib.wsi_pf_bytes(n, h // 2, w // 2, cout, planes)
            for base in (M.S2_GATHER, M.S2_SLAB, M.S2_SLAB_128):
                o3, o1 = fill(nbytes), fill(nbytes)
                with native.conv_mode(0, base):
                    rc = lib.wsi_conv3x3s2_ds_fused(P(xpf), P(o3), P(o1), P(wp3), P(b3), P(wp1), P(b1), n, h, w, cin, cout, planes, st)
                case('s2 %s planes %d' % (base.name, planes), str(shape), result(rc, o3, o1))
            o1 = fill(nbytes)
            rc = lib.wsi_conv1x1_bn(P(xpf), P(o1), P(wp1), P(b1), n, h, w, cin, cout, 2, planes, st)
            case('1x1 planes %d' % planes, str(shape), result(rc, o1))
            if planes == 1:                                  # (speed mode has no phase-split path)
                continue
            split = torch.zeros(lib.wsi_pf_split_bytes(n, h, w, cin, planes), dtype=torch.uint8, device=dev)
            rc = lib.wsi_conv3x3_bn_act_split(P(xpf), P(split), P(xpf), P(wp0), P(b0), n, h, w, cin, cin, 1, planes, st)
            for nt2 in (0, M.S2_NT2):
                o3, o1 = fill(nbytes), fill(nbytes)
                with native.conv_mode(nt2):
                    rc2 = lib.wsi_conv3x3s2_ds_fused_split(P(split), P(o3), P(o1), P(wp3), P(b3), P(wp1), P(b1), n, h, w, cin, cout, planes, st)
                case('s2 split nt2 %d planes %d' % (bool(nt2), planes), str(shape), result(rc or rc2, split, o3, o1))
    for shape in UP_SHAPES:
        n, cu, cs, cout, h, w = shape
        for planes in (2, 3):
            wpk, bias = weights(7, cout, cu + cs, 3, planes)
            up = E.pf_pack(rand(8, n, cu, h // 2, w // 2).abs_().to(dev), planes)
            skip = E.pf_pack(rand(9, n, cs, h, w).abs_().to(dev), planes) if cs else None
            out = fill(lib.wsi_pf_bytes(n, h, w, cout, planes))
            rc = lib.wsi_conv3x3_up_concat_bn_act(P(up), P(skip), P(out), P(wpk), P(bias), n, h, w, cu, cs, cout, 1, planes, st)
            case('up + concat planes %d' % planes, str(shape), result(rc, out))
    report()
    # the trunk (mode 3): 96-byte lines, the folded downsample, the phase-split blocks
    cls = W.make_head_state_dict(22, 'classifier')
    eng = E.TrunkEngine(W.make_resnet18_state_dict(11, with_fc=False), dev, planes=3, head=(cls['fc.0.weight'], cls['fc.0.bias']))
    for tile in (64, 256):
        x = rand(tile, 2, 3, tile, tile).to(dev)
        for mode in TRUNK_MODES:
            try:
                with native.conv_mode(mode):
                    feat, logits, _ = eng.forward_f32(x, feat=True, logits=True)
                res = 'logits %s feat %s' % (sha(logits), sha(feat))
            except RuntimeError as e:                        # a mode the trunk declines: its return code is the result
                res = str(e).split(' (')[0]
            print('trunk tile %3d %-15s  %s' % (tile, M(mode).name if mode else 'default', res), flush=True)


if __name__ == '__main__':
    main()
