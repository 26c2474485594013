"""CPU-side checks of the PSPNet 'seg' model (``unet.PSPNet``, smp's pyramid-pooling decoder on all four encoders): key list and shapes
against an independently built module of the spec (tests/pspnet_oracle.py), the factory's defaults and refusals, the torch-op forward
against the oracle, the host fold of the fusing conv (column order and BatchNorm fold, in float64), the packer's padded bias-only row, the
header and the argument validation of the C entries (-22 before any device work: no GPU needed, no pointer is ever followed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import pspnet_oracle as PO
from oracle import resnet_oracle as R
from wsi_segmentation_pipeline_amd import native
from wsi_segmentation_pipeline_amd import synthetic as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R18, R34, R50 = [2, 2, 2, 2], [3, 4, 6, 3], [3, 4, 6, 3]
ENTRIES = ['wsi_pspnet_workspace_bytes', 'wsi_pspnet_workspace_init', 'wsi_pspnet_forward', 'wsi_pspnet_decoder']
SINGLE = ['wsi_pyramid_pool', 'wsi_pspnet_stage_project', 'wsi_pyramid_expand', 'wsi_pspnet_head_up8']


def _lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


@pytest.mark.parametrize('name,arch,make', [('resnet18', 'basic', lambda: W.make_pspnet_state_dict(31, R18, 4)),
                                            ('resnet50', 'bottleneck', lambda: W.make_pspnet_bottleneck_state_dict(31, [1, 1, 1, 1], 4))])
def test_keys_shapes_and_strict_load(name, arch, make):
    """The structure of the spec gives 2 + 3 x 6 + 6 + 2 = 28 decoder keys (every BatchNorm brings num_batches_tracked)."""
    from wsi_segmentation_pipeline_amd import unet
    c = unet.ENC_CH[arch][2]
    spec = PO.SpecDecoder(4, arch).state_dict()
    want = [('decoder.' + k, tuple(v.shape)) for k, v in spec.items()]
    assert len(want) == 28
    assert [(k, tuple(s)) for k, s, _ in unet.pspnet_decoder_key_shapes(4, unet.ENC_CH[arch])] == want
    assert want[0] == ('decoder.psp.stages.0.pool.1.block.0.weight', (c // 4, c, 1, 1)) and want[1][0] == 'decoder.psp.stages.0.pool.1.block.0.bias'
    assert want[2] == ('decoder.psp.stages.1.pool.1.block.0.weight', (c // 4, c, 1, 1)) and want[7][0].endswith('stages.1.pool.1.block.1.num_batches_tracked')
    assert want[20] == ('decoder.conv.block.0.weight', (512, 2 * c, 1, 1)) and want[26:] == [('decoder.final_conv.weight', (4, 512, 3, 3)), ('decoder.final_conv.bias', (4,))]
    dec = unet.PSPNetDecoder(4, enc_ch=unet.ENC_CH[arch])
    assert [(k, tuple(v.shape)) for k, v in dec.state_dict().items()] == [(k[len('decoder.'):], s) for k, s in want]
    assert isinstance(dec.dropout, torch.nn.Dropout2d) and dec.dropout.p == 0.2
    sd = make()
    assert [(k, tuple(v.shape)) for k, v in sd.items() if k.startswith('decoder.')] == want
    if arch == 'basic':
        model = unet.PSPNet(name, encoder_weights=None, classes=4, activation=None)
        assert list(sd.keys()) == list(model.state_dict().keys())
        model.load_state_dict(sd, strict=True)                                        # layers 3 and 4 included: smp checkpoints carry them
        assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
        assert any(k.startswith('encoder.layer4.') for k in sd)
        enc = W.make_resnet_state_dict(31, R18, with_fc=False)
        assert all(torch.equal(sd['encoder.' + k], v) for k, v in enc.items() if not k.startswith('fc'))
    else:
        dec.load_state_dict({k[len('decoder.'):]: v for k, v in sd.items() if k.startswith('decoder.')}, strict=True)


def test_factory_defaults_refusals_and_model_name_switch():
    from wsi_segmentation_pipeline_amd import unet as smp
    m = smp.PSPNet()                                                                 # smp's defaults: resnet34, 21 classes, dropout 0.2
    assert type(m) is smp.PSPNetSeg and m.encoder_name == 'resnet34' and m.classes == 21 and m.decoder.dropout.p == 0.2
    assert tuple(m.decoder.final_conv.weight.shape) == (21, 512, 3, 3)
    m = getattr(smp, 'PSPNet')('resnet18', encoder_weights=None, classes=4, activation=None)   # the reference's eval('smp.' + args.model_name)(...)
    assert type(m) is smp.PSPNetSeg and isinstance(m, smp.UNetSeg) and m.classes == 4 and m.ENGINE is smp.PSPNetEngine
    for name in ('Unet', 'Linknet', 'FPN', 'PSPNet'):                                # the four names of myargs.py:9-10
        assert isinstance(getattr(smp, name)('resnet18', encoder_weights=None, classes=2, activation=None), smp.UNetSeg)
    for name in ('resnet50', 'resnet101'):
        b = smp.PSPNet(name, classes=2)
        assert type(b) is smp.PSPNetSegBottleneck and isinstance(b, smp.UNetSeg) and b.encoder.out_shapes == (2048, 1024, 512, 256, 64)
        assert tuple(b.decoder.conv.block[0].weight.shape) == (512, 1024, 1, 1)
    assert smp.PSPNetEngine.ENTRY == {'basic': 'wsi_pspnet', 'bottleneck': 'wsi_pspnet_bneck'}
    for kw, match in (({'encoder_weights': 'imagenet'}, 'encoder_weights'), ({'activation': 'softmax'}, 'activation'),
                      ({'precision': 'mx'}, 'parity.*speed'), ({'psp_in_factor': 4}, 'psp_in_factor'), ({'psp_in_factor': 16}, 'psp_in_factor'),
                      ({'psp_out_channels': 256}, 'psp_out_channels'), ({'psp_use_batchnorm': False}, 'psp_use_batchnorm'),
                      ({'psp_aux_output': True}, 'psp_aux_output'), ({'dropout': 1.0}, 'dropout'), ({'dropout': -0.1}, 'dropout')):
        with pytest.raises(ValueError, match=match):
            smp.PSPNet('resnet18', **kw)
    with pytest.raises(ValueError, match='encoder_name'):
        smp.PSPNet('vgg16')
    assert smp.PSPNet('resnet18', precision='speed', dropout=0.0).decoder.dropout.p == 0.0


@pytest.mark.parametrize('name,make', [('resnet18', lambda: W.make_pspnet_state_dict(31, R18, 4)),
                                       ('resnet50', lambda: W.make_pspnet_bottleneck_state_dict(31, R50, 4))])
def test_training_mode_forward_matches_the_spec(name, make):
    """torch-op forward (BatchNorm and Dropout in eval mode) at (2, 3, 64, 64) against the float64 oracle: fp32 rounding (1e-5 of the
    maximum, the bound tests/test_fpn_cpu.py uses; the oracle's own fp32 evaluation is held to it too)."""
    from wsi_segmentation_pipeline_amd import unet
    sd = make()
    model = unet.PSPNet(name, classes=4)
    model.load_state_dict(sd, strict=True)
    model.train()
    for m in model.modules():
        if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.Dropout2d)):
            m.eval()
    x = R.normalize_u8(W.make_u8_patches(41, (2, 3, 64, 64)))
    with torch.no_grad():
        ref, ref_enc = PO.forward(sd, x)
        ref32 = PO.decoder(sd, ref_enc, torch.float32)
        got_enc = model.encoder(x)
        got = model.decoder(got_enc)
        only = model.decoder([None, None, got_enc[2], None, None])                   # the decoder reads x2 alone
        whole = model(x)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (2, 4, 64, 64) and len(got_enc) == 5
    assert torch.equal(only, got)
    scale = float(ref.abs().max())
    errs = [float((t.double() - ref).abs().max()) / scale for t in (ref32, got, whole)]
    print('pspnet %s torch-op forward: spec fp32 %.2e, decoder(encoder(x)) %.2e, model(x) %.2e of the maximum (bound 1e-5)' % (name, *errs))
    assert max(errs) <= 1e-5
    for a, b in zip(got_enc, ref_enc):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    model.eval()
    with pytest.raises(RuntimeError, match='GPU'):
        model(x)                                                                     # eval mode: HIP kernels only, no CPU fallback


@pytest.mark.parametrize('shape', [(2, 128, 4, 4), (1, 128, 8, 12), (2, 512, 4, 4), (1, 512, 8, 12)], ids=lambda s: 'x'.join(map(str, s)))
def test_fold_identity_in_float64(shape):
    """What the device computes - Wf . f + shift + expand(W_I . relu(stage_I(pool(f)))) with the host-folded matrices of `pspnet_fold` -
    equals the literal concat + conv + BatchNorm (+ ReLU) of the spec to 1e-12 of the maximum: this pins the column order of decoder.conv
    (stages first, the feature map last), both BatchNorm folds and the bin order, without a GPU.  The oracle's own piecewise helpers
    (the references of the single-op GPU tests) are held to the same bound."""
    from wsi_segmentation_pipeline_amd import unet
    n, c, h, w = shape
    arch = 'basic' if c == 128 else 'bottleneck'
    sd = (W.make_pspnet_state_dict if c == 128 else W.make_pspnet_bottleneck_state_dict)(17, [1, 1, 1, 1], 4)
    f = torch.randn(shape, generator=torch.Generator().manual_seed(h * w + c)).abs_()
    ref = PO.fuse(sd, f)
    fold = unet.pspnet_fold(sd, c)
    assert [a.dtype for a in fold['stage_w'] + fold['proj_w']] == [np.float64] * 8
    assert [a.shape for a in fold['stage_w']] == [(c // 4, c)] * 4 and [a.shape for a in fold['proj_w']] == [(512, c // 4)] * 4
    assert fold['wf'].shape == (512, c) and fold['shift'].shape == (512,)
    pooled = PO.pyramid_pool(f)
    assert tuple(pooled.shape) == (n, 50, c)
    terms, at = [], 0
    for i, s in enumerate(PO.SIZES):
        mid = torch.relu(pooled[:, at:at + s * s] @ torch.from_numpy(fold['stage_w'][i]).T + torch.from_numpy(fold['stage_b'][i]))
        terms.append(mid @ torch.from_numpy(fold['proj_w'][i]).T)
        at += s * s
    terms = torch.cat(terms, 1)
    lin = torch.einsum('oc,nchw->nohw', torch.from_numpy(fold['wf']), f.double()) + torch.from_numpy(fold['shift']).reshape(1, -1, 1, 1)
    got = torch.relu(lin + PO.expand(terms, (h, w)))
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max()) / scale
    err_helpers = float((terms - PO.stage_terms(sd, pooled)).abs().max()) / float(terms.abs().max())
    print('pspnet fold identity %s: %.2e of the maximum; stage_terms helper %.2e (bound 1e-12)' % (shape, err, err_helpers))
    assert float((ref > 0).double().mean()) > 0.2 and err <= 1e-12 and err_helpers <= 1e-12
    # the description states the same columns for the packer: the last C of 2C
    rows = unet.pspnet_decoder(unet.ENC_CH[arch], classes=4).rows
    assert rows[4].prefix == 'decoder.conv.block' and rows[4].real == (512, 2 * c) and rows[4].stored == (512, c) and rows[4].place == [(c, 2 * c, 0)]


@pytest.mark.parametrize('planes,line', [(2, 32), (1, 64)])
def test_packer_pads_the_bias_only_head_row(planes, line):
    """The head row is stored wider than it is (classes -> one line of output channels): its pack equals the pack of the zero-padded
    weight, and its bias is the conv's bias followed by zeros.  The fusing row's pack equals the pack of the last C columns."""
    from wsi_segmentation_pipeline_amd import engine as E
    from wsi_segmentation_pipeline_amd import unet
    lib = _lib()
    sd = W.make_pspnet_state_dict(19, [1, 1, 1, 1], 3)
    dec = unet.pspnet_decoder(unet.ENC_CH['basic'], planes, 3)
    assert dec.rows[5].real == (3, 512) and dec.rows[5].stored == (line, 512) and dec.head_cin is None
    pk = unet.pack_decoder(lib, sd, dec._replace(rows=dec.rows[4:]), planes, 3)
    assert pk.cin == [128, 512] and pk.cout == [512, line] and pk.head_w is None and pk.head_b is None and pk.tail is None
    wp = np.zeros((line, 512, 3, 3), np.float32)
    wp[:3] = sd['decoder.final_conv.weight'].numpy()
    want, zero = E.pack_conv(lib, wp, None, planes)
    assert np.array_equal(pk.convs[1][0], want) and not zero.any()
    assert np.array_equal(pk.convs[1][1][:3], sd['decoder.final_conv.bias'].numpy()) and not pk.convs[1][1][3:].any() and pk.convs[1][1].shape == (line,)
    wf = np.ascontiguousarray(sd['decoder.conv.block.0.weight'].numpy()[:, 128:])
    bn = [sd['decoder.conv.block.1.' + k].numpy() for k in E.BN_KEYS]
    want_w, want_b = E.pack_conv(lib, wf, bn, planes)
    assert np.array_equal(pk.convs[0][0], want_w) and np.array_equal(pk.convs[0][1], want_b)
    shift = unet.pspnet_fold(sd, 128)['shift']
    assert float(np.abs(want_b - shift).max()) <= 1e-6 * float(np.abs(shift).max())
    gn_row = unet.Conv('decoder.final_conv', 'conv3', (3, 512), (line, 512), [(0, 512, 0)], 'gn')
    with pytest.raises(ValueError, match='GroupNorm'):
        unet.pack_decoder(lib, sd, dec._replace(rows=[gn_row]), planes, 3)


def test_header_declares_the_pspnet_entries():
    lib = _lib()
    assert lib.wsi_hip_abi_version() == native.ABI_VERSION == 9                       # additive entries: no bump
    text = open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(wsi_\w+)\s*\(', hdr))
    new = set(ENTRIES) | {e.replace('wsi_pspnet_', 'wsi_pspnet_bneck_') for e in ENTRIES} | set(SINGLE)
    assert len(new) == 12 and new <= declared and declared == set(native.SIGNATURES)
    for name in new:
        assert hasattr(lib, name), name
    assert 'wsi_pspnet_decoder_weights' in hdr
    block = text[text.index('---- PSPNet'):]
    for cite in ('eval.py:22', 'eval_tumorbed.py:21-28', 'utils/eval.py:51', ':196-200', 'myargs.py:9-10'):
        assert cite in block, cite
    prof = text[text.index('wsi_prof_begin arms'):text.index('int wsi_prof_begin')]
    for kind in ('18 = pyramid pool', '19 = stage projection', '20 = pyramid expand', '21 = head x8 upsample'):
        assert kind in prof, kind
    for name in ENTRIES:                                                             # the four mirror wsi_fpn_* argument for argument
        for psp, fpn in ((name, name.replace('_pspnet', '_fpn')),
                         (name.replace('wsi_pspnet_', 'wsi_pspnet_bneck_'), name.replace('wsi_pspnet_', 'wsi_fpn_bneck_'))):
            (res, args), (res0, args0) = native.SIGNATURES[psp], native.SIGNATURES[fpn]
            assert res is res0 and len(args) == len(args0)
            assert [a for a in args if a is not C.POINTER(native.WsiPspnetDecoderWeights)] == [a for a in args0 if a is not C.POINTER(native.WsiFpnDecoderWeights)]


def test_single_op_entries_refuse_bad_arguments():
    lib = _lib()
    fake, other, third = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(12288)

    def bad_of(fn, ok):
        def bad(i, v):
            a = list(ok)
            a[i] = v
            return fn(*a)
        return bad

    bad = bad_of(lib.wsi_pyramid_pool, [fake, other, 1, 4, 4, 128, 2, None])
    assert bad(0, None) == -22 and bad(1, None) == -22
    assert bad(2, 0) == -22 and bad(3, 0) == -22 and bad(4, -1) == -22
    assert bad(5, 0) == -22 and bad(5, 48) == -22 and bad(5, 100) == -22             # not whole lines
    assert bad(6, 3) == -22 and bad(6, 0) == -22
    assert lib.wsi_pyramid_pool(fake, other, 1, 4, 4, 96, 1, None) == -22            # a line is 64 channels in speed mode
    mats = [(C.c_void_p * 4)(*[4096 + 64 * i] * 4) for i in range(3)]
    okp = [fake, C.byref(mats[0]), C.byref(mats[1]), C.byref(mats[2]), other, third, 1, 128, None]
    bad = bad_of(lib.wsi_pspnet_stage_project, okp)
    for i in (0, 1, 2, 3, 4, 5):
        assert bad(i, None) == -22                                                   # a NULL pointer or table
    assert bad(5, other) == -22 and bad(4, fake) == -22 and bad(5, fake) == -22      # aliased buffers
    assert bad(6, 0) == -22 and bad(7, 64) == -22 and bad(7, 256) == -22 and bad(7, 0) == -22
    for tab in mats:
        keep, tab[2] = tab[2], None
        assert lib.wsi_pspnet_stage_project(*okp) == -22                             # a NULL matrix
        tab[2] = keep
    bad = bad_of(lib.wsi_pyramid_expand, [fake, other, 1, 4, 4, 512, 2, None])
    assert bad(0, None) == -22 and bad(1, None) == -22
    assert bad(2, 0) == -22 and bad(3, 0) == -22 and bad(4, 0) == -22 and bad(5, 256) == -22 and bad(5, 128) == -22
    assert bad(6, 3) == -22 and bad(6, 0) == -22
    bad = bad_of(lib.wsi_pspnet_head_up8, [fake, fake, fake, other, third, 1, 4, 4, 512, 4, 2, None])
    for i in (0, 1, 2, 3, 4):
        assert bad(i, None) == -22
    assert bad(3, fake) == -22                                                       # the scratch is not the input
    assert bad(5, 0) == -22 and bad(6, 0) == -22 and bad(7, 0) == -22 and bad(8, 128) == -22
    assert bad(9, 0) == -22 and bad(9, 17) == -22 and bad(10, 3) == -22 and bad(10, 0) == -22


@pytest.mark.parametrize('arch', ['basic', 'bottleneck'])
def test_entries_refuse_bad_arguments_before_any_device_work(arch):
    """As tests/test_fpn_cpu.py: every pointer is the fake address 4096 and every call carries exactly one defect, so a call that got past
    validation would fault on the first memset."""
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
    c = unet.ENC_CH[arch][2]
    table = {2: [(c, 512), (512, 32)], 1: [(c, 512), (512, 64)]}
    dw = native.WsiPspnetDecoderWeights()
    for i in range(2):
        dw.conv_w[i] = dw.conv_b[i] = 4096
    for i in range(4):
        dw.stage_w[i] = dw.stage_b[i] = dw.proj_w[i] = 4096
    dw.classes, dw.feat_c = 4, c

    def widths(planes):
        for i, (cin, cout) in enumerate(table[planes]):
            dw.cin[i], dw.cout[i] = cin, cout
    widths(2)
    encs = (C.c_void_p * 5)(None, None, 4096, None, None)                            # the decoder reads x2 alone
    pre = 'wsi_pspnet_bneck_' if bneck else 'wsi_pspnet_'
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
    assert sizes(n=2) > sizes() and sizes(64, 96) > sizes() and sizes(32, 32) > 0
    widths(1)
    assert 0 < sizes(planes=1) and sizes(planes=2) == 0                              # the head's stored line follows the precision mode
    widths(2)
    assert sizes(planes=1) == 0
    # planes 3 (no mx), planes 0, h % 32, w % 32, n = 0, workspace_n < n
    assert sizes(planes=3) == 0 and calls(planes=3) == (-22, -22, -22)
    assert sizes(planes=0) == 0 and calls(planes=0) == (-22, -22, -22)
    assert sizes(h=48) == 0 and calls(h=48) == (-22, -22, -22)
    assert sizes(w=72) == 0 and calls(w=72) == (-22, -22, -22)
    assert sizes(n=0) == 0 and calls(n=0, cap=0) == (-22, -22, -22)
    assert calls(n=2, cap=1)[1:] == (-22, -22)
    # a width table that disagrees with the encoder, one entry at a time; feat_c; classes
    for i in (0, 1):
        dw.cin[i] += 64
        assert sizes() == 0 and calls() == (-22, -22, -22)
        dw.cin[i] -= 64
        dw.cout[i] = 128
        assert sizes() == 0 and calls() == (-22, -22, -22)
        dw.cout[i] = table[2][i][1]
    for field, wrong, right in (('feat_c', 640 - c, c), ('feat_c', 0, c), ('classes', 0, 4), ('classes', 17, 4), ('classes', -1, 4)):
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
    for tab, i in ((dw.conv_w, 0), (dw.conv_b, 0), (dw.conv_w, 1), (dw.conv_b, 1), (dw.stage_w, 0), (dw.stage_b, 3), (dw.proj_w, 2)):
        assert without(tab, i)[1:] == (-22, -22)                                     # a NULL weight pointer when logits are asked for
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
    # NULL workspace / outputs / maps; of the five maps only x2 is required
    assert ws_init(C.byref(dw), None, 1, 64, 64, 2, None) == -22 and ws_init(None, fake, 1, 64, 64, 2, None) == -22
    assert fwd(C.byref(wt), C.byref(dw), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, None, None, None) == -22
    assert fwd(C.byref(wt), C.byref(dw), fake, None, 0, 0, 0, None, None, 1, 64, 64, None, 1, fake, None, None) == -22
    assert fwd(None, C.byref(dw), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, fake, None, None) == -22
    assert fwd(C.byref(wt), None, fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, fake, None, None) == -22
    assert decode(C.byref(dw), None, 1, 64, 64, 2, fake, 1, fake, None) == -22
    assert decode(C.byref(dw), C.byref(encs), 1, 64, 64, 2, fake, 1, None, None) == -22
    encs[2] = None
    assert decode(C.byref(dw), C.byref(encs), 1, 64, 64, 2, fake, 1, fake, None) == -22
