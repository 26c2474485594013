"""CPU-side checks of the FPN 'seg' model (``unet.FPN``, smp's feature-pyramid decoder with GroupNorm and bilinear upsampling on all four
encoders): key list and shapes against an independently built module of the spec (tests/fpn_oracle.py), the factory's refusals, the torch-op
forward against the oracle, the header and the argument validation of the C entries (-22 before any device work: no GPU needed, no pointer
is ever followed), and the choice of the GPU test's variance case."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import fpn_oracle as FO
from oracle import pf_lines_oracle as P
from oracle import resnet_oracle as R
from wsi_segmentation_pipeline_amd import native
from wsi_segmentation_pipeline_amd import synthetic as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R18, R34, R50 = [2, 2, 2, 2], [3, 4, 6, 3], [3, 4, 6, 3]
TOL_PARITY = 2e-5         # tests/test_gpu_kernels.py: one op, relative to the tensor's maximum, fp16 hi + lo pair
ENTRIES = ['wsi_fpn_workspace_bytes', 'wsi_fpn_workspace_init', 'wsi_fpn_forward', 'wsi_fpn_decoder']
SINGLE = ['wsi_groupnorm_scratch_bytes', 'wsi_groupnorm_relu_up2', 'wsi_fpn_merge_head_up4', 'wsi_upsample2_nearest']
SEG_CIN = (256, 128, 128, 256, 128, 256, 256)          # stored cin of the seven 3x3 convs (include/wsi_hip.h)


def _lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


@pytest.mark.parametrize('name,arch,make', [('resnet18', 'basic', lambda: W.make_fpn_state_dict(31, R18, 4)),
                                            ('resnet50', 'bottleneck', lambda: W.make_fpn_bottleneck_state_dict(31, [1, 1, 1, 1], 4))])
def test_keys_shapes_and_strict_load(name, arch, make):
    from wsi_segmentation_pipeline_amd import unet
    spec = FO.SpecDecoder(4, arch).state_dict()
    want = [('decoder.' + k, tuple(v.shape)) for k, v in spec.items()]
    assert len(want) == 31
    assert [(k, tuple(s)) for k, s, _ in unet.fpn_decoder_key_shapes(4, unet.ENC_CH[arch])] == want
    assert want[0] == ('decoder.conv1.weight', (256, unet.ENC_CH[arch][0], 1, 1)) and want[8] == ('decoder.s5.block.0.block.0.weight', (128, 256, 3, 3))
    dec = unet.FPNDecoder(4, enc_ch=unet.ENC_CH[arch])
    assert [(k, tuple(v.shape)) for k, v in dec.state_dict().items()] == [(k[len('decoder.'):], s) for k, s in want]
    assert isinstance(dec.dropout, torch.nn.Dropout2d) and dec.dropout.p == 0.2
    sd = make()
    assert [(k, tuple(v.shape)) for k, v in sd.items() if k.startswith('decoder.')] == want
    if arch == 'basic':
        model = unet.FPN(name, encoder_weights=None, classes=4, activation=None)
        assert list(sd.keys()) == list(model.state_dict().keys())
        model.load_state_dict(sd, strict=True)
        assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
        enc = W.make_resnet_state_dict(31, R18, with_fc=False)
        assert all(torch.equal(sd['encoder.' + k], v) for k, v in enc.items() if not k.startswith('fc'))
    else:
        dec.load_state_dict({k[len('decoder.'):]: v for k, v in sd.items() if k.startswith('decoder.')}, strict=True)
    # the draw: conv weights kaiming (fan_out), GroupNorm weight 0.75 ... 1.25, biases small
    w = sd['decoder.s5.block.0.block.0.weight']
    assert abs(float(w.std()) / (2.0 / (128 * 9)) ** 0.5 - 1.0) < 0.02
    g = sd['decoder.s5.block.0.block.1.weight']
    assert 0.75 <= float(g.min()) and float(g.max()) <= 1.25 and float(sd['decoder.conv1.bias'].abs().max()) <= 0.05


def test_factory_refusals_and_model_name_switch():
    from wsi_segmentation_pipeline_amd import unet as smp
    m = smp.FPN()                                                                    # smp's defaults: resnet34, one class
    assert type(m) is smp.FPNSeg and m.encoder_name == 'resnet34' and m.classes == 1
    m = getattr(smp, 'FPN')('resnet18', encoder_weights=None, classes=4, activation=None)     # the reference's eval('smp.' + args.model_name)(...)
    assert type(m) is smp.FPNSeg and isinstance(m, smp.UNetSeg) and m.classes == 4
    for name in ('resnet50', 'resnet101'):
        b = smp.FPN(name, classes=2)
        assert type(b) is smp.FPNSegBottleneck and isinstance(b, smp.UNetSeg) and b.encoder.out_shapes == (2048, 1024, 512, 256, 64)
    for kw, match in (({'encoder_weights': 'imagenet'}, 'encoder_weights'), ({'activation': 'softmax'}, 'activation'),
                      ({'precision': 'mx'}, 'parity.*speed'), ({'decoder_pyramid_channels': 128}, 'decoder_pyramid_channels'),
                      ({'decoder_segmentation_channels': 64}, 'decoder_segmentation_channels'), ({'final_upsampling': 2}, 'final_upsampling'),
                      ({'dropout': 1.0}, 'dropout'), ({'dropout': -0.1}, 'dropout')):
        with pytest.raises(ValueError, match=match):
            smp.FPN('resnet18', **kw)
    with pytest.raises(ValueError, match='encoder_name'):
        smp.FPN('vgg16')
    assert smp.FPN('resnet18', precision='speed', dropout=0.0).decoder.dropout.p == 0.0
    # the fixed arguments are compared by value: smp's defaults in another number type pass
    assert type(smp.FPN('resnet18', decoder_pyramid_channels=256.0, decoder_segmentation_channels=128.0, final_upsampling=np.int64(4))) is smp.FPNSeg


@pytest.mark.parametrize('name,make', [('resnet18', lambda: W.make_fpn_state_dict(31, R18, 4)),
                                       ('resnet50', lambda: W.make_fpn_bottleneck_state_dict(31, R50, 4))])
def test_training_mode_forward_matches_the_spec(name, make):
    """torch-op forward (BatchNorm and Dropout in eval mode) at (2, 3, 64, 64) against the float64 oracle: fp32 rounding (1e-5 of the
    maximum, the bound tests/test_linknet_cpu.py uses; the oracle's own fp32 evaluation is held to it too)."""
    from wsi_segmentation_pipeline_amd import unet
    sd = make()
    model = unet.FPN(name, classes=4)
    model.load_state_dict(sd, strict=True)
    model.train()
    for m in model.modules():
        if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.Dropout2d)):
            m.eval()
    x = R.normalize_u8(W.make_u8_patches(41, (2, 3, 64, 64)))
    with torch.no_grad():
        ref, ref_enc = FO.forward(sd, x)
        ref32 = FO.decoder(sd, ref_enc, torch.float32)
        got_enc = model.encoder(x)
        got = model.decoder(got_enc)
        whole = model(x)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (2, 4, 64, 64) and len(got_enc) == 5
    scale = float(ref.abs().max())
    errs = [float((t.double() - ref).abs().max()) / scale for t in (ref32, got, whole)]
    print('fpn %s torch-op forward: spec fp32 %.2e, decoder(encoder(x)) %.2e, model(x) %.2e of the maximum (bound 1e-5)' % (name, *errs))
    assert max(errs) <= 1e-5
    for a, b in zip(got_enc, ref_enc):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    model.eval()
    with pytest.raises(RuntimeError, match='GPU'):
        model(x)                                                                     # eval mode: HIP kernels only, no CPU fallback


def test_header_declares_the_fpn_entries():
    lib = _lib()
    assert lib.wsi_hip_abi_version() == native.ABI_VERSION == 9                       # additive entries: no bump
    text = open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(wsi_\w+)\s*\(', hdr))
    new = set(ENTRIES) | {e.replace('wsi_fpn_', 'wsi_fpn_bneck_') for e in ENTRIES} | set(SINGLE)
    assert new <= declared and declared == set(native.SIGNATURES)
    for name in new:
        assert hasattr(lib, name), name
    assert 'wsi_fpn_decoder_weights' in hdr
    for cite in ('eval.py:22', 'eval_tumorbed.py:21-28', 'utils/eval.py:51', ':196-200', 'myargs.py:9'):
        assert cite in text[text.index('---- FPN'):], cite
    for name in ENTRIES:                                                             # the four mirror wsi_unet_* argument for argument
        for fpn, unet_name in ((name, name.replace('_fpn', '_unet')), (name.replace('wsi_fpn_', 'wsi_fpn_bneck_'), name.replace('wsi_fpn_', 'wsi_unet_bneck_'))):
            (res, args), (res0, args0) = native.SIGNATURES[fpn], native.SIGNATURES[unet_name]
            assert res is res0 and len(args) == len(args0)
            assert [a for a in args if a is not C.POINTER(native.WsiFpnDecoderWeights)] == [a for a in args0 if a is not C.POINTER(native.WsiUnetDecoderWeights)]


def test_single_op_entries_refuse_bad_arguments():
    lib = _lib()
    fake, other = C.c_void_p(4096), C.c_void_p(8192)
    g = lambda *a: lib.wsi_groupnorm_relu_up2(*a)
    ok = [fake, other, fake, fake, 1, 4, 4, 128, 32, 1e-5, 1, 2, fake, None]

    def bad(i, v):
        a = list(ok)
        a[i] = v
        return g(*a)
    for i in (0, 1, 2, 3, 12):
        assert bad(i, None) == -22                                                   # a NULL pointer
    assert bad(1, fake) == -22                                                       # in == out
    assert bad(4, 0) == -22 and bad(5, 0) == -22 and bad(6, -1) == -22
    assert bad(7, 64) == -22 and bad(7, 256) == -22                                  # the kernels are built for 128 channels
    assert bad(8, 24) == -22 and bad(8, 0) == -22 and bad(8, 16) == -22              # groups not dividing the width; not 32
    assert bad(9, 0.0) == -22 and bad(10, 2) == -22
    assert bad(11, 3) == -22 and bad(11, 0) == -22
    assert lib.wsi_groupnorm_scratch_bytes(1, 1, 1) == (1 + 1) * 32 * 2 * 4
    assert lib.wsi_groupnorm_scratch_bytes(2, 64, 64) == (2 * 64 + 2) * 32 * 2 * 4
    assert lib.wsi_groupnorm_scratch_bytes(0, 4, 4) == 0 and lib.wsi_groupnorm_scratch_bytes(1, 0, 4) == 0
    maps = (C.c_void_p * 4)(*[4096] * 4)
    m = lambda *a: lib.wsi_fpn_merge_head_up4(*a)
    okm = [C.byref(maps), fake, fake, 1, 8, 8, 128, 4, fake, other, 2, None]

    def badm(i, v):
        a = list(okm)
        a[i] = v
        return m(*a)
    for i in (0, 1, 2, 8, 9):
        assert badm(i, None) == -22
    assert badm(9, fake) == -22                                                      # the scratch is not the output
    assert badm(3, 0) == -22 and badm(4, 0) == -22 and badm(6, 64) == -22 and badm(7, 0) == -22 and badm(7, 17) == -22 and badm(10, 3) == -22
    maps[2] = None
    assert m(*okm) == -22
    u = lib.wsi_upsample2_nearest
    assert u(None, other, 1, 4, 4, 256, 2, None) == -22 and u(fake, None, 1, 4, 4, 256, 2, None) == -22 and u(fake, fake, 1, 4, 4, 256, 2, None) == -22
    assert u(fake, other, 1, 4, 4, 48, 2, None) == -22 and u(fake, other, 1, 4, 4, 32, 1, None) == -22 and u(fake, other, 1, 4, 4, 256, 3, None) == -22
    assert u(fake, other, 0, 4, 4, 256, 2, None) == -22 and u(fake, other, 1, 0, 4, 256, 2, None) == -22


@pytest.mark.parametrize('arch', ['basic', 'bottleneck'])
def test_entries_refuse_bad_arguments_before_any_device_work(arch):
    """As tests/test_linknet_cpu.py: every pointer is the fake address 4096 and every call carries exactly one defect, so a call that got
    past validation would fault on the first memset."""
    from wsi_segmentation_pipeline_amd import unet
    lib = _lib()
    fake = C.c_void_p(4096)
    bneck = arch == 'bottleneck'
    wt = (native.WsiBneckWeights if bneck else native.WsiTrunkWeights)()
    wt.planes = 2
    wt.stem_w = wt.stem_b = 4096
    for i in range((3 if bneck else 2) * native.TRUNK_MAX_BLOCKS):
        wt.conv_w[i] = wt.conv_b[i] = 4096
    for i in range(4 if bneck else 3):
        wt.down_w[i] = wt.down_b[i] = 4096
    for i in range(4):
        wt.blocks[i] = R34[i]
    ec = unet.ENC_CH[arch]
    table = [(ec[0], 256), (ec[1], 256), (ec[2], 256), (ec[3], 256)] + [(c, 128) for c in SEG_CIN]
    dw = native.WsiFpnDecoderWeights()
    for i, (cin, cout) in enumerate(table):
        dw.conv_w[i] = dw.conv_b[i] = 4096
        dw.cin[i], dw.cout[i] = cin, cout
    for i in range(7):
        dw.gn_w[i] = dw.gn_b[i] = 4096
    dw.groups, dw.eps, dw.classes = 32, 1e-5, 4
    dw.head_w = dw.head_b = 4096
    encs = (C.c_void_p * 5)(*[4096] * 5)
    pre = 'wsi_fpn_bneck_' if bneck else 'wsi_fpn_'
    ws_bytes, ws_init, fwd, decode = (getattr(lib, pre + s) for s in ('workspace_bytes', 'workspace_init', 'forward', 'decoder'))
    trunk_bytes = lib.wsi_bneck_workspace_bytes if bneck else lib.wsi_trunk_workspace_bytes

    def sizes(h=64, w=64, planes=2, n=1):
        return ws_bytes(C.byref(dw), n, h, w, planes)

    def calls(h=64, w=64, src=fake, planes=2, n=1, cap=1):
        """(init, forward, decoder) return codes"""
        wt.planes = planes
        try:
            return (ws_init(C.byref(dw), fake, n, h, w, planes, None),
                    fwd(C.byref(wt), C.byref(dw), src, None, 0, 0, 0, None, None, n, h, w, fake, cap, fake, None, None),
                    decode(C.byref(dw), C.byref(encs), n, h, w, planes, fake, cap, fake, None))
        finally:
            wt.planes = 2

    assert sizes() > trunk_bytes(1, 64, 64, 2) > 0
    assert 0 < sizes(planes=1) < sizes() and sizes(n=2) > sizes() and sizes(64, 96) > sizes()
    assert sizes(32, 32) > 0                                                         # c5 is 1 x 1
    # planes 3 (no mx), planes 0, h % 32, w % 32, n = 0, workspace_n < n
    assert sizes(planes=3) == 0 and calls(planes=3) == (-22, -22, -22)
    assert sizes(planes=0) == 0 and calls(planes=0) == (-22, -22, -22)
    assert sizes(h=48) == 0 and calls(h=48) == (-22, -22, -22)
    assert sizes(w=72) == 0 and calls(w=72) == (-22, -22, -22)
    assert sizes(n=0) == 0 and calls(n=0, cap=0) == (-22, -22, -22)
    assert calls(n=2, cap=1)[1:] == (-22, -22)
    # a width table that disagrees with the spec, one entry at a time; groups, eps, classes
    for i in (0, 3, 4, 10):
        dw.cin[i] += 64
        assert sizes() == 0 and calls() == (-22, -22, -22)
        dw.cin[i] -= 64
        dw.cout[i] = 64
        assert sizes() == 0 and calls() == (-22, -22, -22)
        dw.cout[i] = table[i][1]
    for field, wrong, right in (('groups', 16, 32), ('groups', 24, 32), ('eps', 0.0, 1e-5), ('classes', 0, 4), ('classes', 17, 4)):
        setattr(dw, field, wrong)
        assert sizes() == 0 and calls() == (-22, -22, -22), field
        setattr(dw, field, right)
    assert sizes() > 0

    def without(tab, i):
        keep, tab[i] = tab[i], None
        try:
            return calls()
        finally:
            tab[i] = keep
    assert without(wt.conv_b, 0)[1] == -22 and without(wt.down_b, 2)[1] == -22
    for tab, i in ((dw.conv_w, 0), (dw.conv_b, 3), (dw.conv_w, 10), (dw.gn_w, 0), (dw.gn_b, 6)):
        assert without(tab, i)[1:] == (-22, -22)
    for field in ('head_w', 'head_b'):
        setattr(dw, field, None)
        assert calls()[1:] == (-22, -22)
        setattr(dw, field, 4096)
    wt.stem_b = None
    assert calls()[1] == -22
    wt.stem_b = 4096
    assert calls(src=None)[1] == -22                                                 # neither in_f32 nor slide
    for blocks in ((0, 4, 6, 3), (3, -1, 6, 3), (native.TRUNK_MAX_BLOCKS + 1, 1, 1, 1)):
        for i in range(4):
            wt.blocks[i] = blocks[i]
        assert calls()[1] == -22, blocks
    for i in range(4):
        wt.blocks[i] = R34[i]
    # NULL workspace / outputs / maps; the decoder never reads x0, so only the first four maps are required
    assert ws_init(C.byref(dw), None, 1, 64, 64, 2, None) == -22 and ws_init(None, fake, 1, 64, 64, 2, None) == -22
    assert fwd(C.byref(wt), C.byref(dw), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, None, None, None) == -22
    assert fwd(C.byref(wt), C.byref(dw), fake, None, 0, 0, 0, None, None, 1, 64, 64, None, 1, fake, None, None) == -22
    assert fwd(None, C.byref(dw), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, fake, None, None) == -22
    assert fwd(C.byref(wt), None, fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, fake, None, None) == -22
    assert decode(C.byref(dw), None, 1, 64, 64, 2, fake, 1, fake, None) == -22
    assert decode(C.byref(dw), C.byref(encs), 1, 64, 64, 2, fake, 1, None, None) == -22
    encs[3] = None
    assert decode(C.byref(dw), C.byref(encs), 1, 64, 64, 2, fake, 1, fake, None) == -22


def _variance_models(x, weight, bias):
    """relu(group_norm(x)) in NumPy fp32 with the variance taken two ways: a bare E[x^2] - E[x]^2, and two-pass (centred)"""
    n, c, h, w = x.shape
    xg = x.reshape(n, FO.GROUPS, -1)
    m = xg.mean(-1, dtype=np.float32)
    d = xg - m[..., None]
    outs = []
    for var in ((xg * xg).mean(-1, dtype=np.float32) - m * m, (d * d).mean(-1, dtype=np.float32)):
        rstd = (np.float32(1) / np.sqrt(var + np.float32(FO.EPS))).astype(np.float32)
        y = (d * rstd[..., None]).reshape(n, c, h, w) * weight.reshape(1, c, 1, 1) + bias.reshape(1, c, 1, 1)
        outs.append(np.maximum(y, 0))
    return outs


@pytest.mark.parametrize('shape', [(2, 128, 8, 12), (1, 128, 64, 64)])
def test_variance_case(shape):
    """The GPU test's "offset group" (fpn_oracle.gn_input with offset_k = OFFSET_K: one group whose mean is ~128 standard deviations),
    chosen here: against float64 F.group_norm of the fp32 input, a bare fp32 E[x^2] - E[x]^2 breaks the per-op bound TOL_PARITY, and
    the two-pass variance holds it even with the input rounded to the parity line format (what the kernel reads)."""
    weight, bias = FO.gn_affine(3)
    x = FO.gn_input(shape, 77, FO.OFFSET_K)
    n, c, h, w = shape
    grp = x.reshape(n, FO.GROUPS, -1)[:, FO.OFFSET_GROUP]
    assert 100 < float(grp.mean() / grp.std()) < 160
    ref = FO.gn_relu(x, weight, bias).numpy()
    lines = P.decode(P.encode(np.ascontiguousarray(x.permute(0, 2, 3, 1).reshape(-1, 32).numpy()), 2), 2)
    xr = np.ascontiguousarray(lines.reshape(n, h, w, c).transpose(0, 3, 1, 2))
    bare = _variance_models(x.numpy(), weight.numpy(), bias.numpy())[0]
    two_pass = _variance_models(xr, weight.numpy(), bias.numpy())[1]
    scale = np.abs(ref).max()
    e_bare, e_two = float(np.abs(bare - ref).max() / scale), float(np.abs(two_pass - ref).max() / scale)
    print('offset group k = %d at %s: bare E[x^2] - E[x]^2 %.3e, two-pass on parity lines %.3e of the maximum (bound %.0e)'
          % (FO.OFFSET_K, shape, e_bare, e_two, TOL_PARITY))
    assert e_bare > TOL_PARITY and e_two <= TOL_PARITY
