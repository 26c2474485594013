"""GPU parity of the U-Net on Bottleneck encoders (ResNet-50 / ResNet-101; wsi_unet_bneck_forward / _decoder) in parity mode: the encoder
maps against the reference's own outputs (tests/golden/resnet50_bag64.npz), the logits against the CPU spec
(tests/unet_bottleneck_oracle.py) under the project's ABSOLUTE 1e-3 contract at max |logit| 16, the routes the launches take, the u8 slide
path, and predict_tumorbed(mode='seg') with the model the smp-signature factory returns."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import seg_model_checks as M
import unet_bottleneck_oracle as UB
from oracle import resnet_oracle as R
from seg_model_checks import LOGIT_TOL, SPEED_TOL, U8_TOL
from wsi_segmentation_pipeline_amd import synthetic as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R50, R101 = [3, 4, 6, 3], [3, 4, 23, 3]
# the spec under the names the shared checks use (its decoder lists no maps)
SPEC = types.SimpleNamespace(forward=UB.unet_forward, decoder=lambda sd, enc, maps=None: UB.U.decoder(sd, enc))
TAP_TOL = M.TAP_TOL['bottleneck']      # tests/test_gpu_resnet50.py TAP_TOL: relative to the map's maximum
# Measured on an MI355X (profiles/unet_resnet50_parity.json); the bounds above were set before and are not derived from these.
ENC_MEASURED = {'x1 vs fixture': 1.27e-06, 'x2 vs fixture': 1.88e-06, 'x3 vs fixture': 1.80e-06, 'x4 vs fixture': 1.91e-06,
                'x4': 1.63e-06, 'x3': 1.22e-06, 'x2': 1.23e-06, 'x1': 9.63e-07, 'x0': 7.24e-07}
LOGIT_MEASURED = {'resnet50 3x64x64': 9.918e-05, 'resnet50 2x32x32': 6.068e-05, 'resnet50 2x64x96': 1.297e-04, '[1, 1, 1, 1] 2x64x64': 8.202e-05,
                  'resnet101 2x64x64': 1.020e-04}
LOGIT_CASES = [('resnet50 3x64x64', R50, (3, 64, 64)), ('resnet50 2x32x32', R50, (2, 32, 32)),          # 32 x 32: x4 is 1 x 1
               ('resnet50 2x64x96', R50, (2, 64, 96)), ('[1, 1, 1, 1] 2x64x64', [1, 1, 1, 1], (2, 64, 64)),
               ('resnet101 2x64x64', R101, (2, 64, 64))]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def sd():
    """seed 21: the encoder half is the checkpoint of tests/golden/resnet50_bag64.npz"""
    return W.make_unet_bottleneck_state_dict(21, R50, 4)


@pytest.fixture(scope='module')
def bag6():
    """the first six images of the fixture's input bag, normalised"""
    u8 = W.make_u8_patches(22, (2, 16, 3, 64, 64)).reshape(-1, 3, 64, 64)
    return R.normalize_u8(u8[:6])


def _rel(got, ref):
    return float((got.cpu() - ref).abs().max() / ref.abs().max())


def test_encoder_maps_vs_reference_fixture(dev, sd, bag6, golden_dir):
    """model.encoder(x) of the factory's model: x1..x4 of image 0 against the reference's own block outputs (the fixture keeps every
    tap_cstride-th channel), all six images and x0 against the spec."""
    from wsi_segmentation_pipeline_amd import unet
    g = np.load(os.path.join(golden_dir, 'resnet50_bag64.npz'))
    assert int(g['weight_seed']) == 21 and int(g['input_seed']) == 22 and list(g['layers']) == R50
    cs, ss = int(g['tap_cstride']), int(g['tap_sstride'])
    model = unet.Unet('resnet50', encoder_weights=None, classes=4, activation=None)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    with torch.no_grad():
        enc = model.encoder(bag6.to(dev))
        enc_sd = {k[8:]: v for k, v in sd.items() if k.startswith('encoder.')}
        ref = UB.encoder(enc_sd, bag6)
    assert [tuple(t.shape[1:]) for t in enc] == [(2048, 2, 2), (1024, 4, 4), (512, 8, 8), (256, 16, 16), (64, 32, 32)]
    report = {}
    for name, tap, got in (('x1', 'tap_layer1_2', enc[3]), ('x2', 'tap_layer2_3', enc[2]), ('x3', 'tap_layer3_5', enc[1]), ('x4', 'tap_layer4_2', enc[0])):
        want = torch.from_numpy(g[tap])
        sub = got[0, ::cs, ::ss, ::ss]
        assert sub.shape == want.shape, name
        report[name + ' vs fixture'] = _rel(sub, want)
    for name, got, want in zip(('x4', 'x3', 'x2', 'x1', 'x0'), enc, ref):
        report[name] = _rel(got, want)
    print('unet resnet50 encoder maps, rel to max:', {k: '%.2e' % v for k, v in report.items()})
    assert max(report.values()) <= TAP_TOL, report


def _checkpoint(layers):
    """The seeded U-Net checkpoint of an encoder depth.  The seeded draw (BatchNorm scale 0.75 ... 1.25 on every residual branch, statistics
    that do not match the data) grows by ~1.4 x per block through layer 3: at 23 blocks (ResNet-101) the spec's layer3.22 reaches 1.6e5,
    past the largest fp16 (65504) the parity mode's line format can hold, which no trained net does.  So that depth halves bn3's weight and
    bias in layer 3 (the residual branch's scale, as zero_init_residual sets it to 0): every map stays under 1e3."""
    sd = W.make_unet_bottleneck_state_dict(21, layers, 4)
    if layers[2] > 6:
        for key in sd:
            if key.startswith('encoder.layer3.') and key.endswith(('.bn3.weight', '.bn3.bias')):
                sd[key] = sd[key] * 0.5
    return sd


@pytest.mark.parametrize('name,layers,shape', LOGIT_CASES, ids=[c[0] for c in LOGIT_CASES])
def test_logits_hold_the_absolute_contract(dev, name, layers, shape):
    """Whole forward, and model.decoder(model.encoder(x)) through fp32 NCHW maps, against the spec at max |logit| 16."""
    from wsi_segmentation_pipeline_amd.unet import UNetEngine
    n, h, w = shape
    x = R.normalize_u8(W.make_u8_patches(41 + h + w, (n, 3, h, w)))
    sd, ref, ref_enc, _ = M.scaled_to_logit(SPEC, _checkpoint(layers), x)
    assert abs(float(ref.abs().max()) - 16.0) < 1e-3
    assert max(float(t.abs().max()) for t in ref_enc) < 6e4                         # inside the fp16 range of the line format
    eng = UNetEngine(sd, dev, planes=2)
    assert eng.arch == 'bottleneck' and eng.trunk.layers == layers and eng.dw.tail_w
    got, enc = eng.forward_f32(x.to(dev), logits=True, enc=True)
    two = eng.decode(enc)
    assert got.shape == ref.shape == (n, 4, h, w)
    err, err2 = float((got.cpu() - ref).abs().max()), float((two.cpu() - ref).abs().max())
    d12 = float((two - got).abs().max())
    enc_err = [_rel(a, b) for a, b in zip(enc, ref_enc)]
    print('unet %s parity: max |logit - spec| %.3e (decoder(encoder(x)): %.3e, between the two %.3e) ABSOLUTE at max |logit| 16; '
          'encoder maps rel err %s' % (name, err, err2, d12, ['%.1e' % e for e in enc_err]))
    assert max(enc_err) <= TAP_TOL
    assert err <= LOGIT_TOL and err2 <= LOGIT_TOL and d12 <= LOGIT_TOL
    assert float((got.cpu().argmax(1) != ref.argmax(1)).float().mean()) <= 0.002


def test_u8_slide_path_equals_f32_path(dev, sd):
    """forward_tiles on a 200 x 260 slide, four 64 x 64 tiles, one hanging over the edge (the integer stem, which also stores x0),
    against forward_f32 of the gathered tiles."""
    from wsi_segmentation_pipeline_amd.unet import UNetEngine
    M.u8_slide_path_equals_f32_path(UNetEngine, SPEC, sd, dev)


@pytest.mark.parametrize('shape', [(2, 2048, 1024, 256, 4, 4), (1, 2048, 1024, 256, 6, 10), (2, 256, 512, 128, 8, 8), (2, 128, 256, 64, 16, 16)])
def test_fused_upsample_concat_conv_is_bit_identical_at_the_bottleneck_shapes(dev, shape):
    """The first conv of decoder blocks 1-3 on a Bottleneck encoder, (n, c_up, c_skip, cout, h, w) of the OUTPUT map (block 4 is the
    BasicBlock model's (64, 64) shape): the fused upsample + concat route is taken (rc 0, not -22) and gives the same bits as running the
    same kernel on a materialised cat(up2(x), skip) - written as tests/test_gpu_unet.py::test_fused_upsample_concat_conv_is_bit_identical,
    parity mode; a ragged tile among them."""
    import torch.nn.functional as F
    from wsi_segmentation_pipeline_amd import native, engine as E
    lib = native.load()
    n, cu, cs, co, h, w = shape
    planes = 2
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(n * 13 + cu + h)
    xu = torch.randn(n, cu, h // 2, w // 2, generator=g).abs_()
    xs = torch.randn(n, cs, h, w, generator=g).abs_()
    wt = torch.randn(co, cu + cs, 3, 3, generator=g) * (2.0 / (9 * (cu + cs))) ** 0.5
    cat = torch.cat([F.interpolate(xu, scale_factor=2, mode='nearest'), xs], 1)
    wpk, bias = E.prepack_conv(wt, None, planes, dev)
    up_pf, sk_pf, cat_pf = E.pf_pack(xu.to(dev), planes), E.pf_pack(xs.to(dev), planes), E.pf_pack(cat.to(dev), planes)
    out = E.pf_zeros(n, co, h, w, planes, dev)
    rc = lib.wsi_conv3x3_up_concat_bn_act(up_pf.data_ptr(), sk_pf.data_ptr(), out.data_ptr(), wpk.data_ptr(), bias.data_ptr(),
                                          n, h, w, cu, cs, co, 1, planes, st)
    assert rc == 0, (shape, rc)
    ref = E.pf_zeros(n, co, h, w, planes, dev)
    cfg = 30 if co % 128 == 0 else 31
    rc = lib.wsi_conv3x3_bn_act_cfg(cat_pf.data_ptr(), ref.data_ptr(), None, wpk.data_ptr(), bias.data_ptr(), n, h, w, cu + cs, co, 1, 1, planes, cfg, st)
    assert rc == 0, (shape, cfg, rc)
    assert torch.equal(out, ref), shape
    got = E.pf_unpack(out, n, co, h, w, planes)
    want = F.relu(F.conv2d(cat, wt, None, 1, 1))
    err = float((got.cpu() - want).abs().max() / want.abs().max())
    print('fused upsample + concat conv %s: rel err vs fp32 conv2d %.2e' % (shape, err))
    assert err <= 2e-4


def test_routes_of_one_forward(dev, sd):
    """The profiler's record kinds of one (3, 64, 64) forward: the encoder's 1x1 convs on the pointwise kernel (kind 11: two per block and
    layer 1's downsample), every decoder block's first conv on the fused upsample + concat route (no refused launch, kind 9, and no concat
    pass, kind 7, once the decoder has begun - the one 7 before it is the stem conv for x0), the fused tail (10) last."""
    from wsi_segmentation_pipeline_amd import native
    from wsi_segmentation_pipeline_amd.unet import UNetEngine
    x = R.normalize_u8(W.make_u8_patches(43, (3, 3, 64, 64))).to(dev)
    eng = UNetEngine(sd, dev, planes=2)
    eng.forward_f32(x)                                                              # (plans the workspace outside the recording)
    kinds = [k for k, _ in native.profiled(lambda: eng.forward_f32(x))[1]]       # (a ResNet-50 U-Net forward makes 66 launches)
    print('prof kinds, unet resnet50:', kinds)
    first_dec = kinds.index(6)
    assert 9 not in kinds and 7 not in kinds[first_dec:] and kinds[:first_dec].count(7) == 1
    assert kinds.count(10) == 1 and kinds[-1] == 10 and 8 not in kinds
    assert kinds.count(6) == 8 and kinds[first_dec:-1] == [6] * 8
    blocks = sum(R50)
    assert kinds.count(11) == 2 * blocks + 1 and kinds.count(3) == 3 and kinds.count(1) + kinds.count(2) == blocks and kinds[0] == 4


def test_speed_mode_is_sane(dev, sd, bag6):
    """planes 1 (single-pass bf16): outside the contract; finite logits, and x4, within 0.1 of the spec's maximum, on the first three
    images of the fixture's bag."""
    from wsi_segmentation_pipeline_amd.unet import UNetEngine
    M.speed_mode_is_sane(UNetEngine, SPEC, sd, dev, bag6[:3], enc_index=0)


def test_predict_tumorbed_seg_with_the_factory_model(dev, sd, tmp_path, monkeypatch):
    """predict_tumorbed(mode='seg') with unet.Unet('resnet50', ...) on the smallest slide of
    tests/test_gpu_unet.py::test_predict_tumorbed_seg_and_predict_wsis_with_unet: the class map against the CPU chain (spec -> float64
    stitch -> threshold), and the fused tile path (the engine reads the tiles from the device-resident level) is the one taken.  The
    class map only: no heat map and no near-tie rule here."""
    from wsi_segmentation_pipeline_amd import unet
    model = unet.Unet('resnet50', encoder_weights=None, classes=4, activation=None)
    M.predict_tumorbed_seg(model, lambda eng: eng.arch == 'bottleneck', SPEC, sd, tmp_path, monkeypatch, heat=False, near_tie_max=None)


def test_recorded_bounds_match_the_profile():
    """profiles/unet_resnet50_parity.json holds the measured values; they are inside the bounds above."""
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'unet_resnet50_parity.json')))
    assert rec['encoder_maps_rel_err'] == ENC_MEASURED and rec['encoder_map_bound'] == TAP_TOL
    assert rec['logit_abs_err'] == LOGIT_MEASURED and rec['logit_bound'] == LOGIT_TOL
    assert rec['u8_slide_vs_f32_path']['bound_times_scale'] == U8_TOL and rec['speed_mode']['bound'] == SPEED_TOL
    assert set(LOGIT_MEASURED) == {c[0] for c in LOGIT_CASES}
    assert max(ENC_MEASURED.values()) <= TAP_TOL and max(LOGIT_MEASURED.values()) <= LOGIT_TOL
