"""GPU parity of the Linknet 'seg' model (BasicBlock ResNet encoder + smp's transposed-conv decoder on HIP kernels: csrc/linknet.hip,
wsi_linknet_*) against the float64 CPU spec tests/linknet_oracle.py: the transposed conv alone, the 1x1 conv with the skip added after the
ReLU on both of its routes, the whole model under the project's ABSOLUTE 1e-3 contract at max |logit| 16, the launches one forward makes,
the u8 slide path, speed mode, and predict_tumorbed(mode='seg') with the model the smp-signature factory returns.
In parity mode the decoder's last block and head run as one fused kernel (csrc/linknet.hip linknet_tail_kernel); the three launches + head
kernel behind WSI_CONV_MODE_LINKNET_NO_TAIL are held to the same bounds."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import linknet_oracle as LO
import seg_model_checks as M
from oracle import resnet_oracle as R
from seg_model_checks import LOGIT_TOL, SPEED_TOL, TOL_PARITY, TOL_SPEED, U8_TOL
from wsi_segmentation_pipeline_amd import synthetic as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R18, R34 = [2, 2, 2, 2], [3, 4, 6, 3]
TAP_TOL = M.TAP_TOL['basic']      # encoder maps of a BasicBlock trunk, relative to the map's maximum
# Measured on an MI355X (profiles/linknet_parity.json); the bounds above are the project's own, set before and not derived from these.
TCONV_MEASURED = {'1x128x2x2 planes 2': 3.141e-07, '1x128x2x2 planes 1': 2.139e-03, '3x64x4x4 planes 2': 2.829e-07, '3x64x4x4 planes 1': 3.486e-03,
                  '2x64x8x12 planes 2': 4.505e-07, '2x64x8x12 planes 1': 3.217e-03, '1x16x32x32 planes 2': 2.082e-07, '1x16x32x32 planes 1': 4.003e-03,
                  '2x64x5x7 planes 2': 2.773e-07, '2x64x5x7 planes 1': 3.778e-03}
SKIP_ADD_MEASURED = {'2x64->64x8x8 planes 2': 1.169e-07, '2x64->64x8x8 planes 1': 3.939e-03,
                  '2x128->256x4x4 planes 2': 1.247e-07, '2x128->256x4x4 planes 1': 3.623e-03}
LOGIT_MEASURED = {'resnet18 3x64x64': 4.176e-05, 'resnet18 2x64x96': 4.458e-05, 'resnet18 1x128x128': 5.419e-05,
                  'resnet34 2x64x64': 4.876e-05, '[1, 1, 1, 1] 1x64x64': 3.366e-05}
ENC_MEASURED = {'resnet18 3x64x64': 1.520e-06, 'resnet18 2x64x96': 1.300e-06, 'resnet18 1x128x128': 1.560e-06,
                  'resnet34 2x64x64': 1.980e-06, '[1, 1, 1, 1] 1x64x64': 1.240e-06}        # the worst of the five maps
TCONV_CASES = [('1x128x2x2', 1, 128, 2, 2), ('3x64x4x4', 3, 64, 4, 4), ('2x64x8x12', 2, 64, 8, 12), ('1x16x32x32', 1, 16, 32, 32),
               ('2x64x5x7', 2, 64, 5, 7)]        # every pixel a border; image boundaries; more than one tile; 16 real channels padded; odd and ragged
LOGIT_CASES = [('resnet18 3x64x64', R18, (3, 64, 64)), ('resnet18 2x64x96', R18, (2, 64, 96)), ('resnet18 1x128x128', R18, (1, 128, 128)),
               ('resnet34 2x64x64', R34, (2, 64, 64)), ('[1, 1, 1, 1] 1x64x64', [1, 1, 1, 1], (1, 64, 64))]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def sd():
    return W.make_linknet_state_dict(21, R18, 4)


def _bn(c, g):
    return (torch.rand(c, generator=g) * 0.5 + 0.75, torch.randn(c, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1,
            torch.rand(c, generator=g) * 0.5 + 0.75)


def _tconv(dev, n, c, h, w, planes, seed, wscale=None, xscale=1.0):
    """(GPU result, float64 reference) of relu(bn(conv_transpose2d(x))) on c real channels stored on max(64, c)"""
    from wsi_segmentation_pipeline_amd import engine as E
    cs = max(64, c)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g).abs_() * xscale
    wt = torch.randn(c, c, 4, 4, generator=g) * (2.0 / (4 * c)) ** 0.5
    if wscale is not None:
        wt = wt * wscale.reshape(1, c, 1, 1)
    bn = _bn(c, g)
    ref = LO.tconv_bn_relu(x, wt, bn)
    xp, wp = torch.zeros(n, cs, h, w), torch.zeros(cs, cs, 4, 4)
    xp[:, :c], wp[:c, :c] = x, wt
    bnp = [torch.cat([t, torch.full((cs - c,), f)]) for t, f in zip(bn, (1.0, 0.0, 0.0, 1.0))]
    wpk, bias = E.prepack_tconv(wp, bnp, planes, dev)
    out = E.tconv4x4s2_bn_relu(E.pf_pack(xp.to(dev), planes), n, h, w, cs, wpk, bias, planes)
    got = E.pf_unpack(out, n, cs, 2 * h, 2 * w, planes).cpu()
    assert not got[:, c:].any()                                                      # padding channels: relu(0) = 0
    return got[:, :c].double(), ref


@pytest.mark.parametrize('name,n,c,h,w', TCONV_CASES, ids=[t[0] for t in TCONV_CASES])
def test_transposed_conv_matches_float64(dev, name, n, c, h, w):
    errs = {}
    for planes, tol in ((2, TOL_PARITY), (1, TOL_SPEED)):
        got, ref = _tconv(dev, n, c, h, w, planes, 100 + h * w + c)
        assert got.shape == ref.shape == (n, c, 2 * h, 2 * w)
        errs[planes] = float((got - ref).abs().max() / ref.abs().max())
        print('tconv4x4s2 %s planes %d: rel err to max %.3e (bound %.0e)' % (name, planes, errs[planes], tol))
    assert errs[2] <= TOL_PARITY and errs[1] <= TOL_SPEED


def test_transposed_conv_with_large_weights_and_past_the_fp16_range(dev):
    """Per-channel weight magnitudes from 2^-12 to 2^12 (the planes-2 pack carries one power-of-two scale per output channel), and an
    output past 65504, which the fp16 pair clamps: 65504 exactly, never inf."""
    c = 64
    ws = torch.pow(2.0, torch.linspace(-12, 12, c))
    got, ref = _tconv(dev, 2, c, 6, 6, 2, 7, wscale=ws)
    rel = ((got - ref).abs().amax((0, 2, 3)) / ref.abs().amax((0, 2, 3)).clamp_min(1e-30))       # every channel against its OWN maximum
    print('tconv4x4s2 large weights: worst per-channel rel err %.3e (bound %.0e)' % (float(rel.max()), TOL_PARITY))
    assert float(ref.abs().max()) < 6e4 and float(rel.max()) <= TOL_PARITY
    got, ref = _tconv(dev, 1, c, 4, 4, 2, 8, wscale=torch.full((c,), 4.0), xscale=1e4)        # inputs up to ~4e4: inside the format themselves
    assert float(ref.max()) > 65504.0 and torch.isfinite(got).all()
    assert float(got.max()) == 65504.0
    want = ref.clamp(max=65504.0)
    err = float((got - want).abs().max() / want.abs().max())
    print('tconv4x4s2 past the fp16 range: max %.1f, rel err to the clamped reference %.3e' % (float(got.max()), err))
    assert err <= TOL_PARITY


@pytest.mark.parametrize('name,n,cin,cout,h,w', [('2x64->64x8x8', 2, 64, 64, 8, 8), ('2x128->256x4x4', 2, 128, 256, 4, 4)])
def test_conv1x1_with_the_skip_added_after_the_relu(dev, name, n, cin, cout, h, w):
    """relu(bn(conv1x1(x))) + skip on the gather route (64 output channels) and on the pointwise kernel (a multiple of 128), against float64;
    the skip is negative where it matters, so relu(a) + s and relu(a + s) differ by far more than the bound."""
    from wsi_segmentation_pipeline_amd import engine as E
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(n, cin, h, w, generator=g).abs_()
    wt = torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cout) ** 0.5
    bn = _bn(cout, g)
    skip = -torch.randn(n, cout, h, w, generator=g).abs_() * 2.0
    a = F.batch_norm(F.conv2d(x.double(), wt.double()), bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(), False, 0.0, R.BN_EPS)
    ref, other = F.relu(a) + skip.double(), F.relu(a + skip.double())
    assert float((ref - other).abs().max()) > 0.1 * float(ref.abs().max())
    errs = {}
    for planes, tol in ((2, TOL_PARITY), (1, TOL_SPEED)):
        wpk, bias = E.prepack_conv(wt, bn, planes, dev)
        out = E.conv1x1_bn_relu_add(E.pf_pack(x.to(dev), planes), E.pf_pack(skip.to(dev), planes), n, h, w, cin, cout, wpk, bias, planes)
        got = E.pf_unpack(out, n, cout, h, w, planes).cpu().double()
        errs[planes] = float((got - ref).abs().max() / ref.abs().max())
        print('conv1x1 + relu + skip %s planes %d: rel err to max %.3e (bound %.0e)' % (name, planes, errs[planes], tol))
        # the existing epilogue on the same inputs keeps its meaning: act(bn(conv) + resid)
        keep = E.conv1x1_bn_act(E.pf_pack(x.to(dev), planes), n, h, w, cin, cout, wpk, bias, resid_pf=E.pf_pack(skip.to(dev), planes), planes=planes)
        kerr = float((E.pf_unpack(keep, n, cout, h, w, planes).cpu().double() - other).abs().max() / max(float(other.abs().max()), 1e-30))
        assert kerr <= tol
    assert errs[2] <= TOL_PARITY and errs[1] <= TOL_SPEED


def _checkpoint(layers):
    return W.make_linknet_state_dict(21, layers, 4)


@pytest.mark.parametrize('name,layers,shape', LOGIT_CASES, ids=[c[0] for c in LOGIT_CASES])
def test_logits_hold_the_absolute_contract(dev, name, layers, shape):
    """Whole forward, and model.decoder(model.encoder(x)) through fp32 NCHW maps, against the float64 spec at max |logit| 16."""
    from wsi_segmentation_pipeline_amd.unet import LinknetEngine
    n, h, w = shape
    x = R.normalize_u8(W.make_u8_patches(41 + h + w, (n, 3, h, w)))
    sd, ref, ref_enc, maps = M.scaled_to_logit(LO, _checkpoint(layers), x)
    assert abs(float(ref.abs().max()) - 16.0) < 1e-3
    assert max(float(t.abs().max()) for t in list(ref_enc) + maps) < 6e4             # inside the fp16 range of the line format
    eng = LinknetEngine(sd, dev, planes=2)
    assert eng.arch == 'basic' and eng.trunk.layers == layers and eng.dw.tail_w
    got, enc = eng.forward_f32(x.to(dev), logits=True, enc=True)
    two = eng.decode(enc)
    assert got.shape == ref.shape == (n, 4, h, w)
    err, err2 = float((got.cpu().double() - ref).abs().max()), float((two.cpu().double() - ref).abs().max())
    d12 = float((two - got).abs().max())
    enc_err = [float((a.cpu() - b).abs().max() / b.abs().max()) for a, b in zip(enc, ref_enc)]
    flips = float((got.cpu().argmax(1) != ref.argmax(1)).float().mean())
    print('linknet %s parity: max |logit - spec| %.3e (decoder(encoder(x)): %.3e, between the two %.3e) ABSOLUTE at max |logit| 16; '
          'encoder maps rel err %s; arg-max flips %.5f' % (name, err, err2, d12, ['%.2e' % e for e in enc_err], flips))
    assert max(enc_err) <= TAP_TOL
    assert err <= LOGIT_TOL and err2 <= LOGIT_TOL and d12 <= LOGIT_TOL
    assert flips <= 0.002


ROUTE_CASES = [('3x64x64 4 classes', (3, 64, 64), 4), ('2x64x96 2 classes', (2, 64, 96), 2), ('1x128x128 4 classes', (1, 128, 128), 4),
               ('1x32x288 4 classes', (1, 32, 288), 4)]           # the last one is wider than the fused kernel takes: three launches either way


@pytest.mark.parametrize('name,shape,classes', ROUTE_CASES, ids=[c[0] for c in ROUTE_CASES])
def test_fused_tail_and_three_launches_both_hold_the_contract(dev, name, shape, classes):
    """The fused last block + head (default) and the three launches + head kernel (ConvMode.LINKNET_NO_TAIL) on the same inputs: each within
    LOGIT_TOL of the float64 spec at max |logit| 16; their mutual difference is printed.  Several bands per image (128 rows: 16), fewer
    classes than the blob's four, and a tile wider than 256, which the fused kernel refuses (the routes then give the same bits)."""
    from wsi_segmentation_pipeline_amd import native
    from wsi_segmentation_pipeline_amd.unet import LinknetEngine
    n, h, w = shape
    x = R.normalize_u8(W.make_u8_patches(90 + h + w, (n, 3, h, w)))
    sd, ref, _, _ = M.scaled_to_logit(LO, W.make_linknet_state_dict(23, R18, classes), x)
    eng = LinknetEngine(sd, dev, planes=2)
    assert eng.dw.tail_w
    fused = eng.forward_f32(x.to(dev))[0]
    with native.conv_mode(native.ConvMode.LINKNET_NO_TAIL):
        plain = eng.forward_f32(x.to(dev))[0]
    assert fused.shape == plain.shape == (n, classes, h, w) and torch.isfinite(fused).all()
    assert torch.equal(fused, eng.forward_f32(x.to(dev))[0])                          # no hand-over between workgroups: the same bits every run
    e_f, e_p = float((fused.cpu().double() - ref).abs().max()), float((plain.cpu().double() - ref).abs().max())
    d = float((fused - plain).abs().max())
    print('linknet routes %s: fused tail %.3e, three launches %.3e from the spec; between the two %.3e' % (name, e_f, e_p, d))
    assert e_f <= LOGIT_TOL and e_p <= LOGIT_TOL
    if w // 2 > 128:
        assert torch.equal(fused, plain)
    else:
        assert d > 0                                                              # another arithmetic, not the same launches


def test_routes_of_one_forward(dev, sd):
    """The profiler's records of one (3, 64, 64) forward.  Default route: the trunk's, the x0 glue (7), then per decoder block 1-4 [1x1 (12),
    transposed conv (13), 1x1 (12)] and the fused last block + head (14) last: four transposed-conv records plus the tail.  Under
    LINKNET_NO_TAIL: five [12, 13, 12] and the head kernel (8).  No refused launch (9) either way; the transposed convs' FLOPs are
    2 N 2H 2W c c 4 on the stored widths."""
    from wsi_segmentation_pipeline_amd import native
    from wsi_segmentation_pipeline_amd.unet import LinknetEngine
    x = R.normalize_u8(W.make_u8_patches(43, (3, 3, 64, 64))).to(dev)
    eng = LinknetEngine(sd, dev, planes=2)
    eng.forward_f32(x)                                                              # (plans the workspace outside the recording)
    rec = native.profiled(lambda: eng.forward_f32(x))[1]
    with native.conv_mode(native.ConvMode.LINKNET_NO_TAIL):
        rec3 = native.profiled(lambda: eng.forward_f32(x))[1]
    kinds, kinds3 = [k for k, _ in rec], [k for k, _ in rec3]
    print('prof kinds, linknet resnet18: fused %r, three launches %r' % (kinds, kinds3))
    first = kinds.index(12)
    assert kinds[:first] == kinds3[:first] and kinds[:first].count(7) == 1 and kinds[0] == 4
    for k in (kinds, kinds3):
        assert 9 not in k and 6 not in k and 10 not in k
    assert kinds[first:] == [12, 13, 12] * 4 + [14] and kinds3[first:] == [12, 13, 12] * 5 + [8]
    want = [2.0 * 3 * (4 << L) * (4 << L) * c * c * 4 for L, c in enumerate((128, 64, 64, 64, 64))]
    assert [f for k, f in rec3 if k == 13] == want and [f for k, f in rec if k == 13] == want[:4]
    assert rec[-1][1] == 2.0 * 3 * 64 * 64 * (64 * 16 / 4 + 4 * 16 * 16 + 16 * 32 + 32 * 4)


def test_u8_slide_path_equals_f32_path(dev, sd):
    """forward_tiles on a 200 x 260 slide, four 64 x 64 tiles, one hanging over the edge (the integer stem, which also stores x0),
    against forward_f32 of the gathered tiles."""
    from wsi_segmentation_pipeline_amd.unet import LinknetEngine
    M.u8_slide_path_equals_f32_path(LinknetEngine, LO, sd, dev)


def test_speed_mode_is_sane(dev, sd):
    """planes 1 (single-pass bf16): outside the contract; finite logits, and x4, within 0.1 of the spec's maximum."""
    from wsi_segmentation_pipeline_amd.unet import LinknetEngine
    M.speed_mode_is_sane(LinknetEngine, LO, sd, dev, R.normalize_u8(W.make_u8_patches(45, (3, 3, 64, 64))), enc_index=0)


def test_module_surface_and_mx_refusal(dev, sd):
    """model(x), model.encoder(x), model.decoder(encoding) in eval mode run on the engine; a CPU tensor is refused."""
    from wsi_segmentation_pipeline_amd import unet
    M.module_surface_and_mx_refusal(unet.Linknet, unet.LinknetEngine, LO, sd, dev)


def test_predict_tumorbed_seg_with_the_factory_model(dev, sd, tmp_path, monkeypatch):
    """predict_tumorbed(mode='seg') with unet.Linknet('resnet18', classes=4) on the slide of
    tests/test_gpu_unet.py::test_predict_tumorbed_seg_and_predict_wsis_with_unet: the fused tile path is the one taken (the Linknet engine
    reads the tiles from the device-resident level), the class map and the heat map against the CPU chain (float64 spec -> float64 stitch
    -> threshold / heat map): heat pixels off by more than 1 LSB and class flips at most the 0.002 share the U-Net test allows.  No
    near-tie rule here: the flips are asserted whatever the spec's margins are."""
    from wsi_segmentation_pipeline_amd import unet
    model = unet.Linknet('resnet18', encoder_weights=None, classes=4, activation=None)
    M.predict_tumorbed_seg(model, lambda eng: type(eng) is unet.LinknetEngine, LO, sd, tmp_path, monkeypatch, heat=True, near_tie_max=None)


def test_recorded_bounds_match_the_profile():
    """profiles/linknet_parity.json holds the measured values; they are inside the bounds above."""
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'linknet_parity.json')))
    assert rec['tconv_rel_err'] == TCONV_MEASURED and rec['tconv_bound'] == {'parity': TOL_PARITY, 'speed': TOL_SPEED}
    assert rec['skip_add_rel_err'] == SKIP_ADD_MEASURED
    assert rec['logit_abs_err'] == LOGIT_MEASURED and rec['logit_bound'] == LOGIT_TOL
    assert rec['encoder_maps_worst_rel_err'] == ENC_MEASURED and rec['encoder_map_bound'] == TAP_TOL
    assert rec['u8_slide_vs_f32_path']['bound_times_scale'] == U8_TOL and rec['speed_mode']['bound'] == SPEED_TOL
    assert set(rec['routes_logit_abs_err']) == {c[0] for c in ROUTE_CASES}
    assert all(max(v['fused_tail'], v['three_launches']) <= LOGIT_TOL for v in rec['routes_logit_abs_err'].values())
    assert set(LOGIT_MEASURED) == set(ENC_MEASURED) == {c[0] for c in LOGIT_CASES}
    assert set(TCONV_MEASURED) == {'%s planes %d' % (c[0], p) for c in TCONV_CASES for p in (2, 1)}
    assert max(LOGIT_MEASURED.values()) <= LOGIT_TOL and max(ENC_MEASURED.values()) <= TAP_TOL
    assert all(v <= (TOL_PARITY if k.endswith('planes 2') else TOL_SPEED) for k, v in list(TCONV_MEASURED.items()) + list(SKIP_ADD_MEASURED.items()))
