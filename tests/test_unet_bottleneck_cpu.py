"""CPU-side checks of the U-Net on Bottleneck encoders (ResNet-50 / ResNet-101): the smp-signature factory ``unet.Unet``, key lists and
shapes, the torch-op forward against the spec (tests/unet_bottleneck_oracle.py), what is refused, and the argument validation of the
four wsi_unet_bneck_* entries (-22 before any device work: no GPU needed, no pointer is ever followed)."""
import ctypes as C
import os
import re

import pytest
import torch

import unet_bottleneck_oracle as UB
from oracle import resnet_oracle as R
from wsi_segmentation_pipeline_amd import native
from wsi_segmentation_pipeline_amd import synthetic as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R50, R101 = [3, 4, 6, 3], [3, 4, 23, 3]
ENTRIES = ['wsi_unet_bneck_workspace_bytes', 'wsi_unet_bneck_workspace_init', 'wsi_unet_bneck_forward', 'wsi_unet_bneck_decoder']
# (cin, cout) of the ten decoder convs on a Bottleneck encoder in parity mode: cat([up2(x), skip]) of (2048, 1024), (256, 512), (128, 256),
# (64, 64), (32, 0); outputs 256 / 128 / 64 / 32 / 16 stored on whole 32-channel lines
DEC_TABLE = ((3072, 256), (256, 256), (768, 128), (128, 128), (384, 64), (64, 64), (128, 32), (32, 32), (32, 32), (32, 32))


def _expected_keys(layers, classes):
    """the Bottleneck keys of resnets_shift under 'encoder.' (no fc*), then the decoder's names with the published widths"""
    keys = [('encoder.' + k, tuple(s)) for k, s, _ in W.bottleneck_key_shapes(layers) if not k.startswith('fc')]
    cprev = 2048
    for L, (skip, cout) in enumerate(zip((1024, 512, 256, 64, 0), (256, 128, 64, 32, 16)), start=1):
        for j, cin in enumerate((cprev + skip, cout)):
            p = 'decoder.layer%d.block.%d.block' % (L, j)
            keys.append((p + '.0.weight', (cout, cin, 3, 3)))
            keys += [('%s.1.%s' % (p, s), (cout,)) for s in ('weight', 'bias', 'running_mean', 'running_var')]
            keys.append((p + '.1.num_batches_tracked', ()))
        cprev = cout
    return keys + [('decoder.final_conv.weight', (classes, 16, 1, 1)), ('decoder.final_conv.bias', (classes,))]


@pytest.mark.parametrize('name,layers', [('resnet50', R50), ('resnet101', R101)])
def test_factory_keys_shapes_and_strict_load(name, layers):
    from wsi_segmentation_pipeline_amd import unet
    model = unet.Unet(name, encoder_weights=None, classes=4, activation=None)        # the call shape of the reference's eval_tumorbed.py
    assert isinstance(model, unet.UNetSeg) and type(model) is unet.UNetSegBottleneck
    want = _expected_keys(layers, 4)
    got = model.state_dict()
    assert list(got.keys()) == [k for k, _ in want]
    assert all(tuple(got[k].shape) == s for k, s in want)
    sd = W.make_unet_bottleneck_state_dict(21, layers, 4)
    assert list(sd.keys()) == [k for k, _ in want] and all(tuple(sd[k].shape) == s for k, s in want)
    model.load_state_dict(sd, strict=True)
    assert model.encoder.out_shapes == (2048, 1024, 512, 256, 64)
    from models.models import Classifier
    assert Classifier(model.encoder.out_shapes[0], 4).fc[0].in_features == 2048
    # the encoder half is the Bottleneck generator's draw, tensor for tensor
    enc = W.make_bottleneck_state_dict(21, layers, with_fc=False)
    assert all(torch.equal(sd['encoder.' + k], v) for k, v in enc.items() if not k.startswith('fc'))


def test_factory_keeps_the_basicblock_models_and_refuses_the_rest():
    from wsi_segmentation_pipeline_amd import unet
    m = unet.Unet()                                                                  # smp's defaults: resnet34, one class
    assert type(m) is unet.UNetSeg and m.encoder_name == 'resnet34' and m.classes == 1
    assert type(unet.Unet('resnet18', classes=4)) is unet.UNetSeg
    assert list(unet.Unet('resnet18', classes=4).state_dict().keys()) == list(W.make_unet_state_dict(7, 4).keys())
    assert unet.Unet('resnet101').encoder_name == 'resnet101'
    with pytest.raises(ValueError, match=r"resnet18.*resnet34.*resnet50.*resnet101"):
        unet.Unet('resnet152')
    with pytest.raises(ValueError, match='encoder_weights'):
        unet.Unet('resnet50', encoder_weights='imagenet')
    with pytest.raises(ValueError, match='resnet34'):
        unet.UNetSeg(4, encoder='resnet50')                                          # the BasicBlock class keeps its refusal
    with pytest.raises(ValueError, match='parity.*speed'):
        unet.Unet('resnet50', classes=4, precision='mx')
    with pytest.raises(ValueError, match='resnet50'):
        unet.UNetSegBottleneck(4, encoder='resnet34')
    assert unet.decoder_key_shapes(4) == unet.decoder_key_shapes(4, (512, 256, 128, 64, 64))          # the default is the BasicBlock one
    assert unet.decoder_key_shapes(4, (2048, 1024, 512, 256, 64))[0][1] == (256, 3072, 3, 3)


def test_training_mode_forward_matches_the_spec():
    """torch-op forward with BatchNorm in eval mode against bottleneck_oracle taps + oracle.unet_oracle.decoder: 1e-5 relative, the bound
    of the ResNet-34 test (tests/test_resnet_depth_cpu.py)."""
    from wsi_segmentation_pipeline_amd import unet
    sd = W.make_unet_bottleneck_state_dict(21, R50, 4)
    model = unet.Unet('resnet50', classes=4)
    model.load_state_dict(sd, strict=True)
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    x = R.normalize_u8(W.make_u8_patches(41, (1, 3, 64, 64)))
    with torch.no_grad():
        ref, ref_enc = UB.unet_forward(sd, x)
        got_enc = model.encoder(x)
        got = model.decoder(got_enc)
        whole = model(x)
    assert [tuple(t.shape) for t in got_enc] == [tuple(t.shape) for t in ref_enc] \
        == [(1, 2048, 2, 2), (1, 1024, 4, 4), (1, 512, 8, 8), (1, 256, 16, 16), (1, 64, 32, 32)]
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert float((whole - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    for a, b in zip(got_enc, ref_enc):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    model.eval()
    with pytest.raises(RuntimeError, match='GPU'):
        model(x)                                                                     # eval mode: HIP kernels only, no CPU fallback


def _lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


def test_header_declares_what_the_library_exports():
    lib = _lib()
    assert lib.wsi_hip_abi_version() == native.ABI_VERSION == 9                       # additive entries: no bump
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read(), flags=re.S)
    assert int(re.search(r'#define WSI_HIP_ABI_VERSION (\d+)', hdr).group(1)) == 9
    declared = set(re.findall(r'\b(wsi_\w+)\s*\(', hdr))
    assert set(ENTRIES) <= declared and declared == set(native.SIGNATURES)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    # argument lists: the four mirror wsi_unet_* with wsi_bneck_weights in the trunk's place
    for name in ENTRIES:
        res, args = native.SIGNATURES[name]
        res0, args0 = native.SIGNATURES[name.replace('_bneck', '')]
        assert res is res0 and len(args) == len(args0)
        assert [a for a in args if a is not C.POINTER(native.WsiBneckWeights)] == [a for a in args0 if a is not C.POINTER(native.WsiTrunkWeights)]


def test_entries_refuse_bad_arguments_before_any_device_work():
    """Modelled on tests/test_resnet_depth_cpu.py::test_abi_9_and_depth_table_validation: every pointer is the fake address 4096 and every
    call carries exactly one defect, so a call that got past validation would fault on the first memset."""
    lib = _lib()
    fake = C.c_void_p(4096)
    wt = native.WsiBneckWeights()
    wt.planes = 2
    wt.stem_w = wt.stem_b = 4096
    for i in range(3 * native.TRUNK_MAX_BLOCKS):
        wt.conv_w[i] = wt.conv_b[i] = 4096
    for i in range(4):
        wt.down_w[i] = wt.down_b[i] = 4096
        wt.blocks[i] = R50[i]
    dw = native.WsiUnetDecoderWeights()
    for i, (cin, cout) in enumerate(DEC_TABLE):
        dw.conv_w[i] = dw.conv_b[i] = 4096
        dw.cin[i], dw.cout[i] = cin, cout
    dw.head_w = dw.head_b = 4096
    dw.head_cin, dw.classes = 16, 4
    encs = (C.c_void_p * 5)(*[4096] * 5)

    def sizes(h=64, w=64, planes=2, n=1):
        return lib.wsi_unet_bneck_workspace_bytes(C.byref(dw), n, h, w, planes)

    def calls(h=64, w=64, src=fake, planes=2, n=1, cap=1):
        """(init, forward, decoder) return codes"""
        wt.planes = planes
        try:
            return (lib.wsi_unet_bneck_workspace_init(C.byref(dw), fake, n, h, w, planes, None),
                    lib.wsi_unet_bneck_forward(C.byref(wt), C.byref(dw), src, None, 0, 0, 0, None, None, n, h, w, fake, cap, fake, None, None),
                    lib.wsi_unet_bneck_decoder(C.byref(dw), C.byref(encs), n, h, w, planes, fake, cap, fake, None))
        finally:
            wt.planes = 2

    # the tables themselves are accepted: a size comes back, larger than the encoder's own workspace and smaller in speed mode's 2 bytes
    assert sizes() > lib.wsi_bneck_workspace_bytes(1, 64, 64, 2) > 0
    assert sizes(planes=1) == 0                                                      # 32-channel outputs are no whole line at planes 1
    assert sizes(n=2) > sizes() and sizes(64, 96) > sizes()
    # planes 3, h % 32, w % 32, n = 0
    assert sizes(planes=3) == 0 and calls(planes=3) == (-22, -22, -22)
    assert sizes(planes=0) == 0 and calls(planes=0) == (-22, -22, -22)
    assert sizes(h=48) == 0 and calls(h=48) == (-22, -22, -22)
    assert sizes(w=72) == 0 and calls(w=72) == (-22, -22, -22)
    assert sizes(n=0) == 0 and calls(n=0, cap=0) == (-22, -22, -22)
    assert calls(n=2, cap=1)[1:] == (-22, -22)                                       # workspace_n < n
    # a decoder cin table that disagrees with the Bottleneck widths: the BasicBlock model's table, and one wrong entry
    keep = [(dw.cin[i], dw.cout[i]) for i in range(10)]
    for i, (cin, cout) in enumerate(((768, 256), (256, 256), (384, 128), (128, 128), (192, 64), (64, 64), (128, 32), (32, 32), (32, 32), (32, 32))):
        dw.cin[i], dw.cout[i] = cin, cout
    assert lib.wsi_unet_workspace_bytes(C.byref(dw), 1, 64, 64, 2) > 0                # (that one belongs to wsi_unet_*)
    assert sizes() == 0 and calls() == (-22, -22, -22)
    for i, (cin, cout) in enumerate(keep):
        dw.cin[i], dw.cout[i] = cin, cout
    assert lib.wsi_unet_workspace_bytes(C.byref(dw), 1, 64, 64, 2) == 0               # and the Bottleneck table does not fit the BasicBlock entries
    dw.cin[2] = 640
    assert sizes() == 0 and calls() == (-22, -22, -22)
    dw.cin[2] = 768
    assert sizes() > 0

    def without(table, i):
        keep, table[i] = table[i], None
        try:
            return calls()
        finally:
            table[i] = keep
    # a NULL conv pointer: of the encoder (forward only reads those), of the decoder (forward and decoder)
    assert without(wt.conv_w, 3 * 16 - 1)[1] == -22
    assert without(wt.conv_b, 0)[1] == -22
    assert without(wt.down_b, 3)[1] == -22
    assert without(dw.conv_w, 0)[1:] == (-22, -22)
    assert without(dw.conv_b, 9)[1:] == (-22, -22)
    wt.stem_b = None
    assert calls()[1] == -22
    wt.stem_b = 4096
    assert calls(src=None)[1] == -22                                                 # neither in_f32 nor slide
    # a bad depth table
    mx = native.TRUNK_MAX_BLOCKS
    for blocks in ((0, 4, 6, 3), (3, 4, 6, 0), (3, -1, 6, 3), (mx + 1, 1, 1, 1), (3, 8, 36, 3), (2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30)):
        for i in range(4):
            wt.blocks[i] = blocks[i]
        assert calls()[1] == -22, blocks
    for i in range(4):
        wt.blocks[i] = R50[i]
    # NULL workspace / outputs / maps
    assert lib.wsi_unet_bneck_workspace_init(C.byref(dw), None, 1, 64, 64, 2, None) == -22
    assert lib.wsi_unet_bneck_workspace_init(None, fake, 1, 64, 64, 2, None) == -22
    assert lib.wsi_unet_bneck_forward(C.byref(wt), C.byref(dw), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, None, None, None) == -22
    assert lib.wsi_unet_bneck_forward(C.byref(wt), C.byref(dw), fake, None, 0, 0, 0, None, None, 1, 64, 64, None, 1, fake, None, None) == -22
    assert lib.wsi_unet_bneck_forward(None, C.byref(dw), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, fake, None, None) == -22
    assert lib.wsi_unet_bneck_decoder(C.byref(dw), None, 1, 64, 64, 2, fake, 1, fake, None) == -22
    encs[3] = None
    assert lib.wsi_unet_bneck_decoder(C.byref(dw), C.byref(encs), 1, 64, 64, 2, fake, 1, fake, None) == -22
