"""CPU-only: BasicBlock ResNets of any depth (ResNet-34 = [3, 4, 6, 3]) through the drop-in surface, the synthetic generators, the
depth-general restatement (tests/depth_oracle.py) and the C ABI's depth table.  tests/golden/resnet34_bag64.npz was written by the
reference's own ResNet at that depth (tools/gen_golden_resnet34.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import depth_oracle as D
from oracle import resnet_oracle as R
from wsi_segmentation_pipeline_amd import native
from wsi_segmentation_pipeline_amd import synthetic as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R34 = [3, 4, 6, 3]


@pytest.fixture(scope='module')
def g34(golden_dir):
    return np.load(os.path.join(golden_dir, 'resnet34_bag64.npz'))


@pytest.fixture(scope='module')
def sd34():
    return W.make_resnet_state_dict(11, R34)


def test_resnet34_constructs_with_the_reference_keys(g34):
    import resnets_shift
    want = [str(k) for k in g34['state_dict_keys']]
    assert len(want) == 226
    for net in (resnets_shift.ResNet(resnets_shift.BasicBlock, R34), resnets_shift.resnet34()):
        assert list(net.state_dict().keys()) == want
        assert [len(getattr(net, 'layer%d' % L)) for L in (1, 2, 3, 4)] == R34
    assert [k for k, _, _ in W.resnet_key_shapes(R34)] == want
    assert 'resnet34' in resnets_shift.__all__ and 'resnet34' in resnets_shift.model_urls
    assert len(resnets_shift.resnet18().state_dict()) == 130                  # the default depth is what it was


def test_zero_init_residual_at_depth():
    import resnets_shift
    net = resnets_shift.ResNet(resnets_shift.BasicBlock, [1, 3, 1, 2], zero_init_residual=True)
    blocks = [m for m in net.modules() if isinstance(m, resnets_shift.BasicBlock)]
    assert len(blocks) == 7 and all(float(b.bn2.weight.detach().abs().max()) == 0.0 for b in blocks)


def test_unsupported_nets_raise_with_what_is_supported():
    import resnets_shift

    class Bottleneck(torch.nn.Module):
        expansion = 4

    with pytest.raises(NotImplementedError, match=r'BasicBlock ResNets.*Bottleneck nets \(ResNet-50 and deeper\) are not implemented'):
        resnets_shift.ResNet(Bottleneck, [3, 4, 6, 3])
    for layers in ([2, 2, 2], [0, 2, 2, 2], [2, 2, -1, 2], [10, 10, 10, 10], [native.TRUNK_MAX_BLOCKS, 1, 1, 1], 'abcd'):
        with pytest.raises(NotImplementedError, match=r'four positive block counts.*resnet34\(\) = \[3, 4, 6, 3\]'):
            resnets_shift.ResNet(resnets_shift.BasicBlock, layers)
    assert resnets_shift.MAX_BLOCKS == native.TRUNK_MAX_BLOCKS
    resnets_shift.ResNet(resnets_shift.BasicBlock, [native.TRUNK_MAX_BLOCKS - 3, 1, 1, 1])      # the largest net the ABI carries


def test_torch_forward_reproduces_the_reference_fixture(g34, sd34):
    """The training-mode (torch-op) forward of the drop-in at [3, 4, 6, 3] against the reference's own outputs; BatchNorm in eval
    state (running statistics), as the fixture was made."""
    import resnets_shift
    net = resnets_shift.resnet34()
    net.load_state_dict(sd34)
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    shape = tuple(int(v) for v in g34['input_shape'])
    assert shape == (2, 16, 3, 64, 64) and int(g34['weight_seed']) == 11 and int(g34['input_seed']) == 12
    u8 = W.make_u8_patches(int(g34['input_seed']), shape)
    xs = R.normalize_u8(u8.reshape(-1, *shape[2:])).view(*shape)
    with torch.no_grad():
        singles, ens = net(xs)
        rs, re_ = D_forward(sd34, xs)
    assert float(np.abs(g34['singles']).max()) <= 16.0 and float(np.abs(g34['ensemble']).max()) <= 16.0
    assert float(np.abs(singles.numpy() - g34['singles']).max()) <= 1e-5
    assert float(np.abs(ens.numpy() - g34['ensemble']).max()) <= 1e-5
    # ... and the depth-general restatement, which the GPU tests compare against, against the same fixture: logits and every tap
    assert float(np.abs(rs.numpy() - g34['singles']).max()) <= 1e-5 and float(np.abs(re_.numpy() - g34['ensemble']).max()) <= 1e-5
    taps = {}
    with torch.no_grad():
        D.trunk(sd34, xs[0, :1], taps)
    cs, ss = int(g34['tap_cstride']), int(g34['tap_sstride'])
    names = D.tap_names(R34)
    assert len(names) == 17
    for name in names:
        ref = g34['tap_' + name.replace('.', '_')]
        got = taps[name][0, ::cs, ::ss, ::ss].numpy()
        assert got.shape == ref.shape and float(np.abs(got - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max())), name


def D_forward(sd, xs):
    """resnet_oracle.resnet_forward with the depth-general trunk"""
    import torch.nn.functional as F
    B, P = xs.shape[:2]
    feats = [torch.flatten(F.adaptive_avg_pool2d(D.trunk(sd, xs[:, p]), 1), 1) for p in range(P)]
    singles = torch.cat([F.linear(f, sd['fc0.weight'], sd['fc0.bias']) for f in feats], 0)
    h = F.relu(F.linear(torch.cat(feats, 1).view(B, -1), sd['fc.0.weight'], sd['fc.0.bias']))
    return singles, F.linear(h, sd['fc.2.weight'], sd['fc.2.bias'])


def test_generators_at_resnet18_depth_are_the_old_ones():
    a, b = W.make_resnet_state_dict(11, [2, 2, 2, 2]), W.make_resnet18_state_dict(11)
    assert list(a.keys()) == list(b.keys()) and len(a) == 130
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert W.resnet_key_shapes([2, 2, 2, 2]) == W.resnet18_key_shapes()
    ua, ub = W.make_unet_resnet_state_dict(7, [2, 2, 2, 2], 4), W.make_unet_state_dict(7, 4)
    assert list(ua.keys()) == list(ub.keys()) and all(torch.equal(ua[k], ub[k]) for k in ua)
    u34 = W.make_unet_resnet_state_dict(7, R34, 4)
    assert sum(k.startswith('encoder.layer3.') and k.endswith('conv1.weight') for k in u34) == 6
    assert all(torch.equal(u34[k], ub[k]) for k in ub if k.startswith('decoder.'))       # the decoder draw does not depend on the depth
    with pytest.raises(ValueError):
        W.resnet_key_shapes([2, 2, 2])


def test_restatement_at_resnet18_depth_is_the_oracle():
    sd = W.make_resnet18_state_dict(11, with_fc=False)
    x = R.normalize_u8(W.make_u8_patches(3, (2, 3, 64, 96)))
    ta, tb = {}, {}
    with torch.no_grad():
        a, b = D.trunk(sd, x, ta), R.trunk(sd, x, tb)
    assert torch.equal(a, b) and set(ta) == set(tb) and all(torch.equal(ta[k], tb[k]) for k in ta)
    assert D.layers_of(sd) == [2, 2, 2, 2] and D.tap_names([2, 2, 2, 2]) == ['pool'] + ['layer%d.%d' % (l, b) for l in (1, 2, 3, 4) for b in (0, 1)]


def test_trunk_layers_reads_the_depth_and_refuses_what_it_cannot_run(sd34):
    from wsi_segmentation_pipeline_amd.engine import AutoTrunkEngine, trunk_layers
    assert trunk_layers(sd34) == R34
    assert trunk_layers(W.make_resnet18_state_dict(11, with_fc=False)) == [2, 2, 2, 2]
    gap = {k: v for k, v in sd34.items() if not k.startswith('layer3.2.')}
    with pytest.raises(ValueError, match='gaps in the blocks of layer3'):
        trunk_layers(gap)
    with pytest.raises(ValueError, match='Bottleneck'):
        trunk_layers(dict(sd34, **{'layer1.0.conv3.weight': torch.zeros(256, 64, 1, 1)}))
    with pytest.raises(ValueError, match='at most %d' % native.TRUNK_MAX_BLOCKS):
        trunk_layers({k: torch.zeros(1) for k, _, _ in W.resnet_key_shapes([3, 4, 30, 3])})
    with pytest.raises(ValueError, match='no layer4.0.conv1.weight'):
        trunk_layers({k: v for k, v in sd34.items() if not k.startswith('layer4.')})
    # the static fp16-range check of the auto policy sees every 4-D weight, whatever the depth
    assert AutoTrunkEngine._static_check(sd34) is None
    hot = dict(sd34)
    hot['layer3.5.conv2.weight'] = sd34['layer3.5.conv2.weight'] * 1e7
    assert 'layer3.5.conv2.weight' in AutoTrunkEngine._static_check(hot)


def test_unet_module_surface_takes_the_encoder_name():
    from wsi_segmentation_pipeline_amd.unet import UNetSeg
    sd = W.make_unet_resnet_state_dict(7, R34, 4)
    model = UNetSeg(classes=4, encoder='resnet34')
    model.load_state_dict(sd, strict=True)
    assert list(model.state_dict().keys()) == list(sd.keys())
    assert list(UNetSeg(4).state_dict().keys()) == list(W.make_unet_state_dict(7, 4).keys())       # default: resnet18, as before
    assert model.encoder.out_shapes == (512, 256, 128, 64, 64)
    with pytest.raises(ValueError, match='resnet34'):
        UNetSeg(4, encoder='resnet50')
    # training-mode (torch-op) forward == restatement + oracle decoder
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    x = R.normalize_u8(W.make_u8_patches(41, (1, 3, 64, 64)))
    with torch.no_grad():
        ref, ref_enc = D.unet_forward(sd, x)
        got_enc = model.encoder(x)
        got = model.decoder(got_enc)
    assert [tuple(t.shape) for t in got_enc] == [tuple(t.shape) for t in ref_enc]
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_abi_9_and_depth_table_validation():
    """The library reports ABI 9 and the struct mirror agrees with the header; a trunk call whose depth table is out of range is
    refused by argument validation (-22) - before any device work, so this runs without a GPU (no pointer is ever followed).
    So is one with a valid table that lacks a pointer the run would read (a conv, a downsample bias, the stem bias) or an input
    source: wsi_trunk_forward, wsi_trunk_forward_tap and wsi_unet_forward return -22 before the workspace's layout tag is rewritten and
    before any memset or launch.  (Before the entries shared one rule, these calls got as far as hipMemsetAsync on the fake
    workspace: that part of the test is not meant to be run against older libraries.)"""
    if not os.path.exists(native.LIB_PATH):
        native.build()
    lib = native.load()
    hdr = open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read()
    assert lib.wsi_hip_abi_version() == native.ABI_VERSION == 9
    assert int(re.search(r'#define WSI_TRUNK_MAX_BLOCKS (\d+)', hdr).group(1)) == native.TRUNK_MAX_BLOCKS >= 16 + 8
    wt = native.WsiTrunkWeights()
    assert len(wt.conv_w) == len(wt.conv_b) == 2 * native.TRUNK_MAX_BLOCKS and len(wt.blocks) == 4 and len(wt.down_w) == 3
    # 4 pointers + 6 floats + 4 ints, then the pointer tables: the layout the C compiler gives the header's struct
    assert native.WsiTrunkWeights.blocks.offset == 56 and native.WsiTrunkWeights.conv_w.offset == 72
    assert C.sizeof(wt) == 72 + 8 * (4 * native.TRUNK_MAX_BLOCKS + 6) + 8 + 8 + 4 + 4
    wt.planes = 2
    fake = C.c_void_p(4096)                                   # stands for every device pointer: validation fails before one is used
    for f in ('stem_w', 'stem_b'):
        setattr(wt, f, 4096)
    mx = native.TRUNK_MAX_BLOCKS
    for blocks in ((0, 2, 2, 2), (2, 2, 2, 0), (2, -1, 2, 2), (mx + 1, 1, 1, 1), (1, 1, 1, mx + 1), (10, 10, 10, 10), (mx - 2, 1, 1, 1),
                   (2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30)):
        for i in range(4):
            wt.blocks[i] = blocks[i]
        assert lib.wsi_trunk_forward(C.byref(wt), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, fake, None, None, None) == -22, blocks
        assert lib.wsi_trunk_forward_tap(C.byref(wt), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, 0, fake, None) == -22, blocks
    # stop_after beyond the net's block count is refused whatever the (valid) table says
    for i in range(4):
        wt.blocks[i] = R34[i]
    assert lib.wsi_trunk_forward_tap(C.byref(wt), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, 17, fake, None) == -22
    assert lib.wsi_trunk_forward_tap(C.byref(wt), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, -1, fake, None) == -22
    # a valid table, but a pointer the run would read is missing, or the input source: -22 before the workspace is touched
    for i in range(2 * native.TRUNK_MAX_BLOCKS):
        wt.conv_w[i] = wt.conv_b[i] = 4096
    for i in range(3):
        wt.down_w[i] = wt.down_b[i] = 4096
    dw = native.WsiUnetDecoderWeights()
    for i, (cin, cout) in enumerate(((768, 256), (256, 256), (384, 128), (128, 128), (192, 64), (64, 64), (128, 32), (32, 32), (32, 32), (32, 32))):
        dw.conv_w[i] = dw.conv_b[i] = 4096
        dw.cin[i], dw.cout[i] = cin, cout
    dw.head_w = dw.head_b = 4096
    dw.head_cin, dw.classes = 16, 4
    assert lib.wsi_unet_workspace_bytes(C.byref(dw), 1, 64, 64, 2) > 0                     # (the decoder table itself is accepted)

    def calls(src=fake):
        return (lib.wsi_trunk_forward(C.byref(wt), src, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, fake, None, None, None),
                lib.wsi_trunk_forward_tap(C.byref(wt), src, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, 3, fake, None),
                lib.wsi_unet_forward(C.byref(wt), C.byref(dw), src, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, fake, None, None))

    def without(table, i):
        keep, table[i] = table[i], None
        try:
            return calls()
        finally:
            table[i] = keep
    assert without(wt.conv_w, 2 * 16 - 1) == (-22, -22, -22)
    assert without(wt.conv_b, 0) == (-22, -22, -22)
    assert without(wt.down_b, 2) == (-22, -22, -22)
    wt.stem_b = None
    assert calls() == (-22, -22, -22)
    wt.stem_b = 4096
    assert calls(src=None) == (-22, -22, -22)                                              # neither in_f32 nor slide
    assert lib.wsi_trunk_forward(C.byref(wt), None, fake, 0, 64, 64, None, fake, 1, 64, 64, fake, 1, fake, None, None, None) == -22  # a slide without tile corners
