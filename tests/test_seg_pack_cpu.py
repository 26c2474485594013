"""CPU-side pin of what the segmentation decoders upload (unet.pack_decoder on the descriptions unet.unet_decoder / linknet_decoder):
byte for byte what the engines' own ``_pack_decoder`` methods produced on the commit before the decoder description existed, following
tests/test_capi_symbols.py::test_packed_weights_byte_identical.  tests/golden/seg_pack_digests.json is the output of
tools/seg_pack_digests.py on that commit: per case the SHA-256 of every uploaded array in upload order, the stored cin / cout tables,
head_cin, classes and whether a fused-tail blob was made.  The FPN and PSPNet entries pin the whole upload of their engines - the convs,
then the seven GroupNorm weight / bias pairs and the head (FPN), or the transposed stage_w, stage_b and proj_w of the four stages
(PSPNet) - as the commit before the engines shared one packer uploaded it.  No GPU is needed: packing is host work."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from wsi_segmentation_pipeline_amd import native
from wsi_segmentation_pipeline_amd import synthetic as W
from wsi_segmentation_pipeline_amd import unet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = 4
CASES = [('unet resnet18', p) for p in (1, 2, 3)] + [('unet bottleneck [1, 1, 1, 1]', p) for p in (1, 2)] + [('linknet resnet18', p) for p in (1, 2)]
ENGINE_CASES = [(m, p) for m in ('fpn resnet18', 'fpn bottleneck [1, 1, 1, 1]', 'pspnet resnet18', 'pspnet bottleneck [1, 1, 1, 1]') for p in (1, 2)]


@functools.lru_cache(maxsize=None)
def _state_dict(model):
    return {'unet resnet18': lambda: W.make_unet_state_dict(7, CLASSES),
            'unet bottleneck [1, 1, 1, 1]': lambda: W.make_unet_bottleneck_state_dict(7, [1, 1, 1, 1], CLASSES),
            'linknet resnet18': lambda: W.make_linknet_state_dict(7),
            'fpn resnet18': lambda: W.make_fpn_state_dict(7, classes=CLASSES),
            'fpn bottleneck [1, 1, 1, 1]': lambda: W.make_fpn_bottleneck_state_dict(7, [1, 1, 1, 1], CLASSES),
            'pspnet resnet18': lambda: W.make_pspnet_state_dict(7, classes=CLASSES),
            'pspnet bottleneck [1, 1, 1, 1]': lambda: W.make_pspnet_bottleneck_state_dict(7, [1, 1, 1, 1], CLASSES)}[model]()


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(os.path.join(ROOT, 'tests', 'golden', 'seg_pack_digests.json')) as f:
        return json.load(f)


def _lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


@pytest.mark.parametrize('model,planes', CASES)
def test_decoder_pack_byte_identical(model, planes):
    """Order, padding, channel placement and every packed byte: 22 arrays per U-Net case and 32 per Linknet case, one more in parity
    mode (the fused tail's blob)."""
    want = _recorded()['%s planes %d' % (model, planes)]
    if model.startswith('linknet'):
        dec = unet.linknet_decoder()
    else:
        dec = unet.unet_decoder(unet.ENC_CH['bottleneck' if 'bottleneck' in model else 'basic'], planes)
    pk = unet.pack_decoder(_lib(), _state_dict(model), dec, planes, CLASSES)
    arrays = [a for pair in pk.convs for a in pair] + [pk.head_w, pk.head_b] + ([pk.tail] if pk.tail is not None else [])
    assert len(want['uploads']) == 2 * len(dec.rows) + 2 + (planes == 2) and len(dec.rows) == (15 if model.startswith('linknet') else 10)
    assert all(isinstance(a, np.ndarray) and a.flags['C_CONTIGUOUS'] for a in arrays)
    got = {'uploads': [hashlib.sha256(a.tobytes()).hexdigest() for a in arrays], 'cin': [int(c) for c in pk.cin],
           'cout': [int(c) for c in pk.cout], 'head_cin': int(dec.head_cin), 'classes': CLASSES, 'tail': pk.tail is not None}
    assert got == want


@pytest.mark.parametrize('model,planes', ENGINE_CASES)
def test_engine_upload_byte_identical(model, planes):
    """Everything an FPN or PSPNet engine uploads, in order: its own ``_pack_decoder`` on an engine that was never constructed, with
    device 'cpu', so that what it keeps alive is what it would have uploaded.  38 arrays per FPN case (11 convs, 7 GroupNorm pairs, the
    head), 16 per PSPNet case (2 convs, 4 x (stage_w.T, stage_b, proj_w.T))."""
    want = _recorded()['%s planes %d' % (model, planes)]
    eng = object.__new__(unet.FPNEngine if model.startswith('fpn') else unet.PSPNetEngine)
    eng.lib, eng.device, eng.planes, eng.classes = _lib(), torch.device('cpu'), planes, CLASSES
    eng.enc_ch = unet.ENC_CH['bottleneck' if 'bottleneck' in model else 'basic']
    eng._keep = []
    eng._pack_decoder(_state_dict(model))
    n = len(eng.dw.cin)
    assert len(want['uploads']) == (38 if model.startswith('fpn') else 16) and n == (11 if model.startswith('fpn') else 2)
    assert all(t.is_contiguous() for t in eng._keep)
    got = {'uploads': [hashlib.sha256(t.numpy().tobytes()).hexdigest() for t in eng._keep], 'cin': list(eng.dw.cin[:n]),
           'cout': list(eng.dw.cout[:n]), 'classes': int(eng.dw.classes)}
    assert got == want


def test_recorded_cases_are_the_fifteen():
    assert sorted(_recorded()) == sorted('%s planes %d' % c for c in CASES + ENGINE_CASES) and len(CASES + ENGINE_CASES) == 15
