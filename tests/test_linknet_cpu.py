"""CPU-side checks of the Linknet 'seg' model (``unet.Linknet``, smp's transposed-conv decoder on BasicBlock encoders): key list and shapes
against an independently built module of the spec (tests/linknet_oracle.py), the factory's refusals, the torch-op forward against the
oracle, the polyphase form of the transposed conv as wsi_prepack_tconv packs it, and the argument validation of the C entries (-22
before any device work: no GPU needed, no pointer is ever followed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import linknet_oracle as LO
from oracle import resnet_oracle as R
from wsi_segmentation_pipeline_amd import native
from wsi_segmentation_pipeline_amd import synthetic as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R18, R34 = [2, 2, 2, 2], [3, 4, 6, 3]
ENTRIES = ['wsi_linknet_workspace_bytes', 'wsi_linknet_workspace_init', 'wsi_linknet_forward', 'wsi_linknet_decoder']
# stored (cin, cout) of the 15 decoder convs: every tensor at least 64 channels wide (include/wsi_hip.h)
DEC_TABLE = ((512, 128), (128, 128), (128, 256), (256, 64), (64, 64), (64, 128), (128, 64), (64, 64), (64, 64),
             (64, 64), (64, 64), (64, 64), (64, 64), (64, 64), (64, 64))


def _lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


@pytest.mark.parametrize('name,layers', [('resnet18', R18), ('resnet34', R34)])
def test_keys_shapes_and_strict_load(name, layers):
    from wsi_segmentation_pipeline_amd import unet
    model = unet.Linknet(name, encoder_weights=None, classes=4, activation=None)     # the call shape of the reference's eval_tumorbed.py
    assert type(model) is unet.LinknetSeg and isinstance(model, unet.UNetSeg)        # (utils.eval's fused tile path asks for a UNetSeg)
    spec = LO.SpecDecoder(4).state_dict()
    want = [('decoder.' + k, tuple(v.shape)) for k, v in spec.items()]
    assert len(want) == 92
    assert sum(int(np.prod(s)) for k, s in want if k.endswith('.0.weight') or k == 'decoder.final_conv.weight') == 484992
    got = model.state_dict()
    dec = [(k, tuple(v.shape)) for k, v in got.items() if k.startswith('decoder.')]
    assert dec == want
    assert [(k, tuple(s)) for k, s, _ in unet.linknet_decoder_key_shapes(4)] == want
    assert want[6] == ('decoder.layer1.block.1.block.0.weight', (128, 128, 4, 4))
    sd = W.make_linknet_state_dict(21, layers, 4)
    assert list(sd.keys()) == list(got.keys()) and all(tuple(sd[k].shape) == tuple(got[k].shape) for k in sd)
    model.load_state_dict(sd, strict=True)
    back = model.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    assert model.encoder.out_shapes == (512, 256, 128, 64, 64)
    enc = W.make_resnet_state_dict(21, layers, with_fc=False)
    assert all(torch.equal(sd['encoder.' + k], v) for k, v in enc.items() if not k.startswith('fc'))
    # the transposed-conv weights are drawn as N(0, 2 / (4 cout))
    w = sd['decoder.layer1.block.1.block.0.weight']
    assert abs(float(w.std()) / (2.0 / (4 * 128)) ** 0.5 - 1.0) < 0.02


def test_factory_refusals_and_model_name_switch():
    from wsi_segmentation_pipeline_amd import unet as smp
    m = smp.Linknet()                                                                # smp's defaults: resnet34, one class
    assert type(m) is smp.LinknetSeg and m.encoder_name == 'resnet34' and m.classes == 1
    for model_name, cls in (('Unet', smp.UNetSeg), ('Linknet', smp.LinknetSeg)):     # the reference's eval('smp.' + args.model_name)(...)
        assert type(getattr(smp, model_name)('resnet18', encoder_weights=None, classes=4, activation=None)) is cls
    with pytest.raises(ValueError, match='resnet18.*resnet34'):
        smp.Linknet('resnet50')
    with pytest.raises(ValueError, match='resnet18.*resnet34'):
        smp.Linknet('resnet101')
    with pytest.raises(ValueError, match='encoder_weights'):
        smp.Linknet('resnet18', encoder_weights='imagenet')
    with pytest.raises(ValueError, match='activation'):
        smp.Linknet('resnet18', activation='softmax')
    with pytest.raises(ValueError, match='parity.*speed'):
        smp.Linknet('resnet18', classes=4, precision='mx')
    assert smp.Linknet('resnet18', precision='speed').precision == 'speed'


def test_training_mode_forward_matches_the_spec():
    """torch-op forward (BatchNorm in eval mode) at (2, 3, 64, 64) against the float64 oracle: fp32 rounding (1e-5 relative, the bound of
    the other torch-op forwards here; the oracle's own fp32 evaluation is compared too)."""
    from wsi_segmentation_pipeline_amd import unet
    sd = W.make_linknet_state_dict(21, R18, 4)
    model = unet.Linknet('resnet18', classes=4)
    model.load_state_dict(sd, strict=True)
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    x = R.normalize_u8(W.make_u8_patches(41, (2, 3, 64, 64)))
    with torch.no_grad():
        ref, ref_enc = LO.forward(sd, x)
        ref32 = LO.decoder(sd, ref_enc, torch.float32)
        got_enc = model.encoder(x)
        got = model.decoder(got_enc)
        whole = model(x)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (2, 4, 64, 64)
    assert [tuple(t.shape) for t in got_enc] == [(2, 512, 2, 2), (2, 256, 4, 4), (2, 128, 8, 8), (2, 64, 16, 16), (2, 64, 32, 32)]
    scale = float(ref.abs().max())
    assert float((ref32.double() - ref).abs().max()) <= 1e-5 * scale
    assert float((got.double() - ref).abs().max()) <= 1e-5 * scale
    assert float((whole.double() - ref).abs().max()) <= 1e-5 * scale
    for a, b in zip(got_enc, ref_enc):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    model.eval()
    with pytest.raises(RuntimeError, match='GPU'):
        model(x)                                                                     # eval mode: HIP kernels only, no CPU fallback


def _unpack_tconv(pk, bias, c, planes):
    """wsi_prepack_tconv's pack -> the folded weights as w[co][ci][ky][kx] (hi + lo, channel scale undone): the layout of
    tests/test_capi_symbols.py::test_prepack_conv_roundtrip with 16 taps."""
    nl = c * planes // 64
    nblocks = (c // 32) * nl * 16 * 4096
    body = pk[:nblocks].view(np.uint16)
    if planes == 2:
        frag = body.view(np.float16).astype(np.float64).reshape(c // 32, nl, 16, 4, 64, 8)
        inv = pk[nblocks:].view(np.float32).astype(np.float64)
        assert inv.shape == (c,) and np.all(np.log2(inv) == np.round(np.log2(inv)))
    else:
        frag = (body.astype(np.uint32) << 16).view(np.float32).astype(np.float64).reshape(c // 32, nl, 16, 4, 64, 8)
        inv = np.ones(c)
    rec = np.zeros((c, c, 4, 4))
    for nt in range(c // 32):
        for l in range(nl):
            for f in range(4):
                cbase = 32 * l + 16 * (f & 1) if planes == 2 else 64 * l + 16 * f
                for lane in range(64):
                    co, ci = nt * 32 + (lane & 31), cbase + 8 * (lane >> 5)
                    rec[co, ci:ci + 8] += frag[nt, l, :, f, lane, :].T.reshape(8, 4, 4)
    return rec * inv[:, None, None, None]


@pytest.mark.parametrize('planes', [2, 1])
def test_prepack_tconv_polyphase_form_equals_conv_transpose(planes):
    """The form csrc/linknet.hip computes, on the host in float64 from the PACKED weights: output pixel (2i + a, 2j + b) = sum over
    dy in {a - 1, a}, dx in {b - 1, b} of x[i + dy, j + dx] (zero outside the map) times tap (ky, kx) = (a + 1 - 2 dy, b + 1 - 2 dx), i.e.
    rows {(i - 1, ky 3), (i, ky 1)} for a = 0 and {(i, ky 2), (i + 1, ky 0)} for a = 1 - against F.conv_transpose2d + BN with the
    caller's [cin][cout][4][4] weights.  With exact weights the identity holds to 4e-15; here to the pack's rounding."""
    lib = _lib()
    c, n, h, w = 64, 2, 5, 7
    rng = np.random.default_rng(5)
    wt = rng.standard_normal((c, c, 4, 4)).astype(np.float32) * np.float32((2.0 / (4 * c)) ** 0.5)
    wt *= np.exp(rng.uniform(np.log(0.1), np.log(30.0), (1, c, 1, 1))).astype(np.float32)     # per-OUTPUT-channel magnitudes: the planes-2 scales
    bn = [rng.uniform(0.5, 1.5, c).astype(np.float32), rng.standard_normal(c).astype(np.float32), rng.standard_normal(c).astype(np.float32),
          rng.uniform(0.5, 1.5, c).astype(np.float32)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nbytes = lib.wsi_prepack_tconv_bytes(c, planes)
    assert nbytes == (c // 32) * (c * planes // 64) * 16 * 4096 + (c * 4 if planes == 2 else 0)
    pk, bias = np.zeros(nbytes, np.uint8), np.zeros(c, np.float32)
    assert lib.wsi_prepack_tconv(p(wt), *[p(a) for a in bn], 1e-5, c, planes, p(pk), p(bias)) == 0
    wf = _unpack_tconv(pk, bias, c, planes)                                          # [co][ci][ky][kx], BN scale folded in
    x = rng.standard_normal((n, c, h, w))
    xp = np.zeros((n, c, h + 2, w + 2))
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((n, c, 2 * h, 2 * w))
    for a in range(2):
        for b in range(2):
            for dy in (a - 1, a):
                for dx in (b - 1, b):
                    ky, kx = a + 1 - 2 * dy, b + 1 - 2 * dx
                    out[:, :, a::2, b::2] += np.einsum('oc,nchw->nohw', wf[:, :, ky, kx], xp[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
    out += bias.astype(np.float64)[None, :, None, None]
    ref = F.conv_transpose2d(torch.from_numpy(x), torch.from_numpy(wt).double(), None, 2, 1)
    g, be, m, v = (torch.from_numpy(t).double() for t in bn)
    ref = F.batch_norm(ref, m, v, g, be, False, 0.0, 1e-5).numpy()
    tol = 2.0 ** -20 if planes == 2 else 2.0 ** -7                                   # fp16 pair: 22 significand bits; bf16: 8
    assert np.abs(out - ref).max() <= tol * np.abs(ref).max()
    # the exact identity, with the caller's own weights
    exact = np.zeros_like(out)
    wd = wt.astype(np.float64)
    for a in range(2):
        for b in range(2):
            for dy in (a - 1, a):
                for dx in (b - 1, b):
                    exact[:, :, a::2, b::2] += np.einsum('co,nchw->nohw', wd[:, :, a + 1 - 2 * dy, b + 1 - 2 * dx], xp[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
    plain = F.conv_transpose2d(torch.from_numpy(x), torch.from_numpy(wd), None, 2, 1).numpy()
    assert np.abs(exact - plain).max() <= 1e-13 * np.abs(plain).max()
    # refusals
    assert lib.wsi_prepack_tconv_bytes(32, 2) == 0 and lib.wsi_prepack_tconv_bytes(96, 2) == 0 and lib.wsi_prepack_tconv_bytes(64, 3) == 0
    assert lib.wsi_prepack_tconv(None, None, None, None, None, 1e-5, 64, 2, p(pk), p(bias)) == -22
    assert lib.wsi_prepack_tconv(p(wt), None, None, None, None, 1e-5, 48, 2, p(pk), p(bias)) == -22
    assert lib.wsi_prepack_tconv(p(wt), None, None, None, None, 1e-5, 64, 3, p(pk), p(bias)) == -22


def test_single_op_entries_refuse_bad_arguments():
    lib = _lib()
    fake = C.c_void_p(4096)
    other = C.c_void_p(8192)
    t = lib.wsi_tconv4x4s2_bn_relu
    assert t(None, other, fake, fake, 1, 4, 4, 64, 2, None) == -22
    assert t(fake, None, fake, fake, 1, 4, 4, 64, 2, None) == -22
    assert t(fake, other, None, fake, 1, 4, 4, 64, 2, None) == -22
    assert t(fake, other, fake, None, 1, 4, 4, 64, 2, None) == -22
    assert t(fake, fake, fake, fake, 1, 4, 4, 64, 2, None) == -22                     # in == out
    assert t(fake, other, fake, fake, 1, 4, 4, 32, 2, None) == -22                    # no multiple of 64
    assert t(fake, other, fake, fake, 1, 4, 4, 64, 3, None) == -22                    # no mx form
    assert t(fake, other, fake, fake, 0, 4, 4, 64, 2, None) == -22
    assert t(fake, other, fake, fake, 1, 0, 4, 64, 2, None) == -22
    assert t(fake, other, fake, fake, 1 << 14, 512, 512, 64, 2, None) == -22          # positions past 2^31
    a = lib.wsi_conv1x1_bn_relu_add
    assert a(fake, other, None, fake, fake, 1, 4, 4, 64, 64, 2, None) == -22          # the skip is the point of the entry
    assert a(fake, other, other, fake, fake, 1, 4, 4, 64, 64, 2, None) == -22         # skip == out
    assert a(fake, other, fake, fake, fake, 1, 4, 4, 64, 64, 3, None) == -22
    assert a(fake, other, fake, fake, fake, 1, 4, 4, 64, 48, 2, None) == -22
    assert a(None, other, fake, fake, fake, 1, 4, 4, 64, 128, 2, None) == -22


def test_header_declares_the_linknet_entries():
    lib = _lib()
    assert lib.wsi_hip_abi_version() == native.ABI_VERSION == 9                       # additive entries: no bump
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(wsi_\w+)\s*\(', hdr))
    new = set(ENTRIES) | {'wsi_prepack_tconv_bytes', 'wsi_prepack_tconv', 'wsi_tconv4x4s2_bn_relu', 'wsi_conv1x1_bn_relu_add',
                          'wsi_linknet_tail_prepack_bytes', 'wsi_linknet_tail_prepack'}
    assert 'WSI_CONV_MODE_LINKNET_NO_TAIL' in hdr and int(native.ConvMode.LINKNET_NO_TAIL) == 16777216
    assert new <= declared and declared == set(native.SIGNATURES)
    for name in new:
        assert hasattr(lib, name), name
    for name in ENTRIES:                                                             # the four mirror wsi_unet_* argument for argument
        res, args = native.SIGNATURES[name]
        res0, args0 = native.SIGNATURES[name.replace('_linknet', '_unet')]
        assert res is res0 and len(args) == len(args0)
        assert [a for a in args if a is not C.POINTER(native.WsiLinknetDecoderWeights)] == [a for a in args0 if a is not C.POINTER(native.WsiUnetDecoderWeights)]


def test_entries_refuse_bad_arguments_before_any_device_work():
    """As tests/test_unet_bottleneck_cpu.py: every pointer is the fake address 4096 and every call carries exactly one defect, so a call
    that got past validation would fault on the first memset."""
    lib = _lib()
    fake = C.c_void_p(4096)
    wt = native.WsiTrunkWeights()
    wt.planes = 2
    wt.stem_w = wt.stem_b = 4096
    for i in range(2 * native.TRUNK_MAX_BLOCKS):
        wt.conv_w[i] = wt.conv_b[i] = 4096
    for i in range(3):
        wt.down_w[i] = wt.down_b[i] = 4096
    for i in range(4):
        wt.blocks[i] = R34[i]
    dw = native.WsiLinknetDecoderWeights()
    for i, (cin, cout) in enumerate(DEC_TABLE):
        dw.conv_w[i] = dw.conv_b[i] = 4096
        dw.cin[i], dw.cout[i] = cin, cout
    dw.head_w = dw.head_b = 4096
    dw.head_cin, dw.classes = 32, 4
    encs = (C.c_void_p * 5)(*[4096] * 5)

    def sizes(h=64, w=64, planes=2, n=1):
        return lib.wsi_linknet_workspace_bytes(C.byref(dw), n, h, w, planes)

    def calls(h=64, w=64, src=fake, planes=2, n=1, cap=1):
        """(init, forward, decoder) return codes"""
        wt.planes = planes
        try:
            return (lib.wsi_linknet_workspace_init(C.byref(dw), fake, n, h, w, planes, None),
                    lib.wsi_linknet_forward(C.byref(wt), C.byref(dw), src, None, 0, 0, 0, None, None, n, h, w, fake, cap, fake, None, None),
                    lib.wsi_linknet_decoder(C.byref(dw), C.byref(encs), n, h, w, planes, fake, cap, fake, None))
        finally:
            wt.planes = 2

    assert sizes() > lib.wsi_trunk_workspace_bytes(1, 64, 64, 2) > 0
    assert 0 < sizes(planes=1) < sizes()                                             # the same 64-channel widths at 2 bytes per channel
    assert sizes(n=2) > sizes() and sizes(64, 96) > sizes()
    # planes 3 (no mx), planes 0, h % 32, w % 32, n = 0, workspace_n < n
    assert sizes(planes=3) == 0 and calls(planes=3) == (-22, -22, -22)
    assert sizes(planes=0) == 0 and calls(planes=0) == (-22, -22, -22)
    assert sizes(h=48) == 0 and calls(h=48) == (-22, -22, -22)
    assert sizes(w=72) == 0 and calls(w=72) == (-22, -22, -22)
    assert sizes(n=0) == 0 and calls(n=0, cap=0) == (-22, -22, -22)
    assert calls(n=2, cap=1)[1:] == (-22, -22)
    # a width table that disagrees with the spec: one entry at a time, the head's width, a reserved tail pointer
    for i in (0, 4, 14):
        dw.cin[i] += 64
        assert sizes() == 0 and calls() == (-22, -22, -22)
        dw.cin[i] -= 64
        dw.cout[i] = 32
        assert sizes() == 0 and calls() == (-22, -22, -22)
        dw.cout[i] = DEC_TABLE[i][1]
    dw.head_cin = 16
    assert sizes() == 0 and calls() == (-22, -22, -22)
    dw.head_cin = 32
    dw.classes = 0
    assert sizes() == 0 and calls() == (-22, -22, -22)
    dw.classes = 4
    assert sizes() > 0

    def without(table, i):
        keep, table[i] = table[i], None
        try:
            return calls()
        finally:
            table[i] = keep
    assert without(wt.conv_w, 2 * 16 - 1)[1] == -22
    assert without(wt.conv_b, 0)[1] == -22
    assert without(wt.down_b, 2)[1] == -22
    assert without(dw.conv_w, 0)[1:] == (-22, -22)
    assert without(dw.conv_w, 7)[1:] == (-22, -22)                                   # a transposed conv
    assert without(dw.conv_b, 14)[1:] == (-22, -22)
    dw.tail_w = 4096                                                                 # a fused-tail blob stands in for block 5 and the head only
    assert without(dw.conv_w, 11)[1:] == (-22, -22) and without(dw.conv_b, 0)[1:] == (-22, -22)
    dw.tail_w = None
    dw.head_b = None
    assert calls()[1:] == (-22, -22)
    dw.head_b = 4096
    wt.stem_b = None
    assert calls()[1] == -22
    wt.stem_b = 4096
    assert calls(src=None)[1] == -22                                                 # neither in_f32 nor slide
    mx = native.TRUNK_MAX_BLOCKS
    for blocks in ((0, 4, 6, 3), (3, 4, 6, 0), (3, -1, 6, 3), (mx + 1, 1, 1, 1), (3, 8, 36, 3), (2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30)):
        for i in range(4):
            wt.blocks[i] = blocks[i]
        assert calls()[1] == -22, blocks
    for i in range(4):
        wt.blocks[i] = R34[i]
    # NULL workspace / outputs / maps
    assert lib.wsi_linknet_workspace_init(C.byref(dw), None, 1, 64, 64, 2, None) == -22
    assert lib.wsi_linknet_workspace_init(None, fake, 1, 64, 64, 2, None) == -22
    assert lib.wsi_linknet_forward(C.byref(wt), C.byref(dw), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, None, None, None) == -22
    assert lib.wsi_linknet_forward(C.byref(wt), C.byref(dw), fake, None, 0, 0, 0, None, None, 1, 64, 64, None, 1, fake, None, None) == -22
    assert lib.wsi_linknet_forward(None, C.byref(dw), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, fake, None, None) == -22
    assert lib.wsi_linknet_forward(C.byref(wt), None, fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, fake, None, None) == -22
    assert lib.wsi_linknet_decoder(C.byref(dw), None, 1, 64, 64, 2, fake, 1, fake, None) == -22
    assert lib.wsi_linknet_decoder(C.byref(dw), C.byref(encs), 1, 64, 64, 2, fake, 1, None, None) == -22
    encs[3] = None
    assert lib.wsi_linknet_decoder(C.byref(dw), C.byref(encs), 1, 64, 64, 2, fake, 1, fake, None) == -22


def test_tail_prepack_blob_and_refusals():
    """wsi_linknet_tail_prepack: the blob holds the BN-folded fp32 weights of decoder.layer5 and final_conv in the kernel's order (csrc/
    linknet.hip LT_*), zeros where a class or channel is absent; what it refuses."""
    lib = _lib()
    sd = W.make_linknet_state_dict(21, R18, 3)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f = lambda k: np.ascontiguousarray(sd[k].numpy())
    args, keep = [], []
    for j in range(3):
        pre = 'decoder.layer5.block.%d.block' % j
        keep += [f(pre + '.0.weight')] + [f('%s.1.%s' % (pre, s)) for s in ('weight', 'bias', 'running_mean', 'running_var')]
    hw, hb = f('decoder.final_conv.weight').reshape(3, 32), f('decoder.final_conv.bias')
    nbytes = lib.wsi_linknet_tail_prepack_bytes()
    assert nbytes == 5828 * 4
    blob = np.full(nbytes // 4, np.nan, np.float32)
    call = lambda cin=64, cmid=16, cout=32, classes=3, out=blob, a=None: lib.wsi_linknet_tail_prepack(
        *[p(t) for t in (a or keep)], 1e-5, p(hw), p(hb), cin, cmid, cout, classes, p(out) if out is not None else None)
    assert call() == 0 and np.isfinite(blob).all()

    def fold(w, bn):
        sc = bn[0].astype(np.float64) / np.sqrt(bn[3].astype(np.float64) + 1e-5)
        return sc, (bn[1].astype(np.float64) - bn[2].astype(np.float64) * sc).astype(np.float32)
    sc0, b0 = fold(keep[0], keep[1:5])
    sct, bt = fold(keep[5], keep[6:10])
    sc2, b2 = fold(keep[10], keep[11:15])
    w0 = (keep[0].reshape(16, 64).astype(np.float64) * sc0[:, None]).astype(np.float32)                  # [co][ci]
    wt = (keep[5].astype(np.float64) * sct[None, :, None, None]).astype(np.float32)                      # [ci][co][ky][kx]
    w2 = (keep[10].reshape(32, 16).astype(np.float64) * sc2[:, None]).astype(np.float32)                 # [c2][co]
    assert np.array_equal(blob[0:1024].reshape(64, 16), w0.T) and np.array_equal(blob[1024:1040], b0)
    assert np.array_equal(blob[1040:5136].reshape(4, 4, 16, 16), wt.transpose(2, 3, 0, 1)) and np.array_equal(blob[5136:5152], bt)
    assert np.array_equal(blob[5152:5664].reshape(16, 32), w2.T) and np.array_equal(blob[5664:5696], b2)
    wh = blob[5696:5824].reshape(32, 4)
    assert np.array_equal(wh[:, :3], hw.T) and not wh[:, 3].any()
    assert np.array_equal(blob[5824:5827], hb) and blob[5827] == 0.0
    assert call(cin=32) == -22 and call(cmid=17) == -22 and call(cmid=0) == -22 and call(cout=33) == -22
    assert call(classes=5) == -22 and call(classes=0) == -22 and call(out=None) == -22
    assert lib.wsi_linknet_tail_prepack(None, *[p(t) for t in keep[1:]], 1e-5, p(hw), p(hb), 64, 16, 32, 3, p(blob)) == -22
    assert lib.wsi_linknet_tail_prepack(*[p(t) for t in keep], 1e-5, None, p(hb), 64, 16, 32, 3, p(blob)) == -22
