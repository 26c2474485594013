#!/usr/bin/env python
"""What the segmentation decoders upload for a state dict and a precision, as JSON: per case the SHA-256 of every array in upload order
(per conv the packed weights and the bias, then the head's weight and bias, then the fused tail's blob if one is made), the stored
`cin` / `cout` tables, `head_cin`, `classes` and whether a tail blob was made.  Host work only: no GPU is needed.

    python tools/seg_pack_digests.py > digests.json

tests/test_seg_pack_cpu.py holds the output of the commit before the decoder description (unet.unet_decoder / linknet_decoder /
pack_decoder) existed, and compares what pack_decoder returns against it.  On such an older tree - copy this file into it - the same
numbers come from the engines' own `_pack_decoder(self, f32, dev)`, called unbound on a stand-in for the engine with a `dev` that
hashes what it is given instead of uploading it; on a tree that has `pack_decoder`, from that function."""
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


def digests():
    lib = native.load()
    one = described if hasattr(unet, 'pack_decoder') else unbound
    out = {}
    for name, make, planes_of in CASES:
        sd = make()
        for planes in planes_of:
            out['%s planes %d' % (name, planes)] = one(lib, name, sd, planes)
    return out


if __name__ == '__main__':
    print('{\n%s\n}' % ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(digests().items())))    # a case per line
