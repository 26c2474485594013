#!/usr/bin/env python
"""What the segmentation decoders upload for a state dict and a precision, as JSON: per case the SHA-256 of every array in upload order
(per conv the packed weights and the bias, then the head's weight and bias, then the fused tail's blob if one is made), the stored
`cin` / `cout` tables, `head_cin`, `classes` and whether a tail blob was made.  Host work only: no GPU is needed.

    python tools/seg_pack_digests.py > digests.json

tests/test_seg_pack_cpu.py holds the output of the commit before the decoder description (unet.unet_decoder / linknet_decoder /
pack_decoder) existed, and compares what pack_decoder returns against it.  On such an older tree - copy this file into it - the same
numbers come from the engines' own `_pack_decoder(self, f32, dev)`, called unbound on a stand-in for the engine with a `dev` that
hashes what it is given instead of uploading it; on a tree that has `pack_decoder`, from that function.

The FPN and PSPNet cases pin the whole upload of their engines, which is more than `pack_decoder`'s arrays (the GroupNorm pairs; the
transposed matrices of `pspnet_fold`): `engine_uploads` runs the engine class's own ``_pack_decoder(state_dict)`` on an engine that was
never constructed - device 'cpu', so "uploading" keeps a host tensor - and hashes what it kept, in order.  Those entries of the golden
file are the output of the commit before the engines shared one packer."""
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wsi_segmentation_pipeline_amd import native, synthetic as W, unet      # noqa: E402

CLASSES = 4
CASES = [('unet resnet18', lambda: W.make_unet_state_dict(7, CLASSES), (1, 2, 3)),
         ('unet bottleneck [1, 1, 1, 1]', lambda: W.make_unet_bottleneck_state_dict(7, [1, 1, 1, 1], CLASSES), (1, 2)),
         ('linknet resnet18', lambda: W.make_linknet_state_dict(7), (1, 2))]
ENGINE_CASES = [('fpn resnet18', 'FPNEngine', lambda: W.make_fpn_state_dict(7, classes=CLASSES)),
                ('fpn bottleneck [1, 1, 1, 1]', 'FPNEngine', lambda: W.make_fpn_bottleneck_state_dict(7, [1, 1, 1, 1], CLASSES)),
                ('pspnet resnet18', 'PSPNetEngine', lambda: W.make_pspnet_state_dict(7, classes=CLASSES)),
                ('pspnet bottleneck [1, 1, 1, 1]', 'PSPNetEngine', lambda: W.make_pspnet_bottleneck_state_dict(7, [1, 1, 1, 1], CLASSES))]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(uploads, cin, cout, head_cin, classes, tail):
    return {'uploads': uploads, 'cin': [int(c) for c in cin], 'cout': [int(c) for c in cout], 'head_cin': int(head_cin),
            'classes': int(classes), 'tail': bool(tail)}


def described(lib, name, sd, planes):
    """through unet.pack_decoder (trees that have the decoder description)"""
    arch = 'bottleneck' if 'bottleneck' in name else 'basic'
    dec = unet.linknet_decoder() if name.startswith('linknet') else unet.unet_decoder(unet.ENC_CH[arch], planes)
    pk = unet.pack_decoder(lib, sd, dec, planes, CLASSES)
    arrays = [a for pair in pk.convs for a in pair] + [pk.head_w, pk.head_b] + ([pk.tail] if pk.tail is not None else [])
    return record([sha(a) for a in arrays], pk.cin, pk.cout, dec.head_cin, CLASSES, pk.tail is not None)


def unbound(lib, name, sd, planes):
    """through the engine's own _pack_decoder(self, f32, dev) (trees before the decoder description)"""
    arch = 'bottleneck' if 'bottleneck' in name else 'basic'
    eng = types.SimpleNamespace(lib=lib, planes=planes, enc_ch=unet.ENC_CH[arch], classes=CLASSES)
    uploads = []

    def f32(key):
        return np.ascontiguousarray(sd[key].detach().to('cpu', torch.float32).numpy())

    def dev(a):
        uploads.append(sha(a))
        return types.SimpleNamespace(data_ptr=lambda: 4096)

    (unet.LinknetEngine if name.startswith('linknet') else unet.UNetEngine)._pack_decoder(eng, f32, dev)
    n = len(eng.dw.cin)
    return record(uploads, eng.dw.cin[:n], eng.dw.cout[:n], eng.dw.head_cin, eng.dw.classes, eng.dw.tail_w)


def engine_uploads(lib, cls, name, sd, planes):
    """through the engine class's own _pack_decoder(state_dict), on the CPU: every array it keeps, in upload order"""
    eng = object.__new__(cls)
    eng.lib, eng.device, eng.planes, eng.classes = lib, torch.device('cpu'), planes, CLASSES
    eng.enc_ch = unet.ENC_CH['bottleneck' if 'bottleneck' in name else 'basic']
    eng._keep = []
    eng._pack_decoder(sd)
    n = len(eng.dw.cin)
    return {'uploads': [sha(t.numpy()) for t in eng._keep], 'cin': list(eng.dw.cin[:n]), 'cout': list(eng.dw.cout[:n]),
            'classes': int(eng.dw.classes)}


def digests():
    lib = native.load()
    one = described if hasattr(unet, 'pack_decoder') else unbound
    out = {}
    for name, make, planes_of in CASES:
        sd = make()
        for planes in planes_of:
            out['%s planes %d' % (name, planes)] = one(lib, name, sd, planes)
    for name, cls, make in ENGINE_CASES:
        sd = make()
        for planes in (1, 2):
            out['%s planes %d' % (name, planes)] = engine_uploads(lib, getattr(unet, cls), name, sd, planes)
    return out


if __name__ == '__main__':
    print('{\n%s\n}' % ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(digests().items())))    # a case per line
