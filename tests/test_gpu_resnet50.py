"""GPU parity of Bottleneck trunks on the HIP path (wsi_bneck_forward, the pointwise kernel): ResNet-50 = [3, 4, 6, 3] against the
reference's own outputs (tests/golden/resnet50_bag64.npz, tools/gen_golden_resnet50.py) and against the CPU restatement
(tests/bottleneck_oracle.py); [1, 1, 1, 1], the smallest net.
Contract (BASELINE.json north_star): max abs logit error <= 1e-3 vs the reference fp32 CPU path, stated for |logit| <= 16."""
import json
import os

import numpy as np
import pytest
import torch

import bottleneck_oracle as B
from oracle import resnet_oracle as R
from oracle import wsi_oracle as WO
from wsi_segmentation_pipeline_amd import synthetic as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_TOL = 1e-3          # BASELINE.json north_star: "within 1e-3 on the output logits"
R50 = [3, 4, 6, 3]
# Per-tap bound, relative to the tap's maximum: the project's loosest existing per-tap bound (tests/test_gpu_resnet34.py TAP_TOL[3]),
# chosen before anything at 53 convs had been measured and NOT tightened from this code's own output (a wrong index or block order is
# O(1)).  Measured on an MI355X (64 x 64, N = 6, parity mode; profiles/resnet50_parity.json): worst tap TAP_MEASURED (layer4.0);
# logits against the reference fixture at max |logit| 10.5 / 8.2: LOGIT_MEASURED.
TAP_TOL = 2e-4
TAP_MEASURED = 1.74e-06
LOGIT_MEASURED = {'singles': 1.62e-05, 'ensemble': 8.58e-06}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def sd():
    return W.make_bottleneck_state_dict(21, R50, with_fc=False)


@pytest.fixture(scope='module')
def eng(sd, dev):
    from wsi_segmentation_pipeline_amd.engine import BottleneckEngine
    return BottleneckEngine(sd, dev, planes=2)


@pytest.fixture(scope='module')
def bag():
    """the fixture's input bag: u8 (32, 3, 64, 64), image index b * P + p, and its normalised form"""
    u8 = W.make_u8_patches(22, (2, 16, 3, 64, 64)).reshape(-1, 3, 64, 64)
    return u8, R.normalize_u8(u8)


@pytest.fixture(scope='module')
def ref_taps(sd, bag):
    """restatement taps of the first six bag images, computed once"""
    taps = {}
    with torch.no_grad():
        B.trunk(sd, bag[1][:6], taps)
    return taps


def _rel(got, ref):
    return float((got.cpu() - ref).abs().max() / ref.abs().max())


def test_taps_vs_restatement_64(dev, eng, bag, ref_taps):
    """Every tap 0..16: weight indexing, block order and the residual choice down to the 2 x 2 maps of layer 4."""
    assert eng.layers == R50 and eng.FEAT_C == 2048
    x = bag[1][:6].to(dev)
    names = B.tap_names(R50)
    assert len(names) == 17
    report = []
    for i, name in enumerate(names):
        got = eng.forward_f32(x, tap=i)
        assert got.shape == ref_taps[name].shape, name
        report.append((name, _rel(got, ref_taps[name])))
    print('resnet50 parity tap errors (rel to max):', report, 'worst %.3e' % max(e for _, e in report))
    with pytest.raises(ValueError):
        eng.forward_f32(x, tap=18)
    with pytest.raises(ValueError):
        eng.forward_f32(x, tap=17)
    for name, err in report:
        assert err <= TAP_TOL, report


def test_engine_routing_and_refusals(dev, sd):
    from wsi_segmentation_pipeline_amd.engine import BottleneckEngine, TrunkEngine
    small = W.make_bottleneck_state_dict(21, [1, 1, 1, 1], with_fc=False)
    with pytest.raises(ValueError, match='BasicBlock'):
        BottleneckEngine(W.make_resnet18_state_dict(11, with_fc=False), dev, planes=2)
    with pytest.raises(NotImplementedError, match='mx'):
        BottleneckEngine(small, dev, planes=3)
    with pytest.raises(ValueError, match='Bottleneck'):
        TrunkEngine(small, dev, planes=2)
    with pytest.raises(ValueError, match='2048'):
        BottleneckEngine(small, dev, planes=2, head=(torch.zeros(4, 512), torch.zeros(4)))


def test_smallest_net(dev):
    """[1, 1, 1, 1]: every block is a stage's first block (downsample residual everywhere); full run and last tap."""
    from wsi_segmentation_pipeline_amd.engine import BottleneckEngine
    sd1 = W.make_bottleneck_state_dict(21, [1, 1, 1, 1], with_fc=False)
    x = R.normalize_u8(W.make_u8_patches(61, (4, 3, 64, 64)))
    with torch.no_grad():
        ref = B.trunk(sd1, x)
    e1 = BottleneckEngine(sd1, dev, planes=2)
    assert e1.layers == [1, 1, 1, 1]
    got = e1.forward_f32(x.to(dev), fmap=True)[2]
    tap = e1.forward_f32(x.to(dev), tap=4)
    err, terr = _rel(got, ref), _rel(tap, ref)
    print('[1,1,1,1] bottleneck: full run rel err %.2e, tap 4 rel err %.2e' % (err, terr))
    assert got.shape == ref.shape == (4, 2048, 2, 2)
    assert err <= TAP_TOL and terr <= TAP_TOL


def test_full_run_equals_last_tap_and_gather_route(dev, eng, sd):
    """forward_f32(fmap=True) against tap 16, and against itself with every stride-1 1x1 conv on the gather kernel (PW_GATHER).  N = 5,
    then N = 3 on the same engine (a workspace planned for the larger batch); 64 x 288 with N = 2 (maps 16 x 72 ... 2 x 9)."""
    from wsi_segmentation_pipeline_amd import native
    for n, h, w in ((5, 64, 64), (3, 64, 64), (2, 64, 288)):
        x = R.normalize_u8(W.make_u8_patches(50 + n + w, (n, 3, h, w))).to(dev)
        full = eng.forward_f32(x, fmap=True)[2].clone()
        tap = eng.forward_f32(x, tap=16).clone()
        again = eng.forward_f32(x, fmap=True)[2].clone()
        with native.conv_mode(native.ConvMode.PW_GATHER):
            gat = eng.forward_f32(x, fmap=True)[2].clone()
        with torch.no_grad():
            ref = B.trunk(sd, x.cpu()) if (n, w) == (2, 288) else None
        assert full.shape == tap.shape == gat.shape == (n, 2048, h // 32, w // 32)
        err = float((full - tap).abs().max() / tap.abs().max())
        gerr = float((full - gat).abs().max() / gat.abs().max())
        print('resnet50 N=%d %dx%d: full run vs tap 16 rel err %.2e, vs the gather route %.2e' % (n, h, w, err, gerr))
        assert torch.equal(full, again)
        assert err <= TAP_TOL and gerr <= TAP_TOL
        if ref is not None:
            rerr = _rel(full, ref)
            print('resnet50 64x288 vs restatement: %.2e' % rerr)
            assert rerr <= TAP_TOL
    assert len(eng._ws) == 2                                                # one workspace per patch shape: N = 3 reused N = 5's


def test_u8_slide_path_equals_f32_path(dev, eng):
    """forward_tiles on a 200 x 260 slide, four 64 x 64 tiles, one hanging over the edge, against forward_f32 of the gathered tiles
    (the bound of tests/test_gpu_resnet34.py::test_u8_slide_path_equals_f32_path in parity mode)."""
    rng = np.random.default_rng(7)
    slide = rng.integers(0, 256, (200, 260, 3), dtype=np.uint8)
    xy = np.array([[0, 0], [100, 50], [260 - 64, 200 - 64], [230, 170]], np.int32)
    tiles = np.stack([WO.read_tile(slide, int(x), int(y), 64, 64) for x, y in xy]).transpose(0, 3, 1, 2)
    x = R.normalize_u8(tiles)
    sl, xyd = torch.from_numpy(slide).to(dev), torch.from_numpy(xy).to(dev)
    b = eng.forward_f32(x.to(dev), feat=True)[0].clone()
    a = eng.forward_tiles(sl, xyd, 64, 64, feat=True, logits=False)[0].clone()
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    print('resnet50 u8 slide path vs f32 path: %.2e of scale %.2e' % (err, scale))
    assert a.shape == (4, 2048)
    assert err <= 2e-5 * scale


def test_bag_forward_vs_reference_fixture(dev, sd, bag, golden_dir):
    """resnets_shift.resnet50 in 'parity' and 'auto' precision against the reference's outputs; 'auto' reports parity; the same module
    as the encoder of utils.eval.SlideClassifierModel with a Classifier(2048, 4).  The one GPU test that builds fc (32768 x 16384)."""
    import resnets_shift
    g = np.load(os.path.join(golden_dir, 'resnet50_bag64.npz'))
    full = W.make_bottleneck_state_dict(int(g['weight_seed']), R50, head_scales=(float(g['fc0_scale']), float(g['fc2_scale'])))
    model = resnets_shift.resnet50(precision='parity')
    model.load_state_dict(full)
    del full
    model = model.cuda().eval()
    xs = bag[1].view(2, 16, 3, 64, 64).to(dev)
    for precision in ('parity', 'auto'):
        model.precision = precision
        with torch.no_grad():
            singles, ens = model(xs)
        e1 = float(np.abs(singles.cpu().numpy() - g['singles']).max())
        e2 = float(np.abs(ens.cpu().numpy() - g['ensemble']).max())
        report = getattr(model.hip_engine(), 'report', None)
        print('resnet50 bag64 %s: max abs err singles %.2e ensemble %.2e (max |logit| %.1f / %.1f) %s'
              % (precision, e1, e2, float(np.abs(g['singles']).max()), float(np.abs(g['ensemble']).max()), report))
        assert e1 <= LOGIT_TOL and e2 <= LOGIT_TOL
        if precision == 'auto':
            assert report['mode'] == 'parity' and 'mx' in report['reason']
    with torch.no_grad():
        f = model.features(xs[0, :2])
    assert f.shape == (2, 2048, 2, 2)
    # the composition predict_tumorbed(mode='cls') drives: encoder surface and the classifier fused behind the average pool
    import utils.eval as val
    from models.models import Classifier
    cls_sd = W.make_head_state_dict(22, 'classifier', num_features=2048)
    x = bag[1][:4]
    with torch.no_grad():
        fm = B.trunk(sd, x)
        s = 1.0
        while float(R.classifier(cls_sd, fm).abs().max()) * s > 16.0:       # the contract is stated for |logit| <= 16
            s *= 0.5
        cls_sd = {k: v * s for k, v in cls_sd.items()}
        ref = R.classifier(cls_sd, fm)
    head = Classifier(2048, 4)
    head.load_state_dict(cls_sd)
    scm = val.SlideClassifierModel(model, head).cuda().eval()
    assert scm.encoder.out_shapes[0] == 2048
    with torch.no_grad():
        enc = scm.encoder(x.to(dev))
        plain = scm.classifier(enc[0])
        fused = scm.fused_engine(dev).forward_f32(x.to(dev), logits=True)[1]
    assert len(enc) == 1 and enc[0].shape == (4, 2048, 2, 2)
    e1, e2 = float((plain.cpu() - ref).abs().max()), float((fused.cpu() - ref).abs().max())
    print('SlideClassifierModel(resnet50, Classifier(2048, 4)): classifier(encoder(x)) err %.2e, fused engine err %.2e' % (e1, e2))
    assert e1 <= LOGIT_TOL and e2 <= LOGIT_TOL


def test_classifier_2048_head(dev, eng, sd, bag):
    """models.Classifier(2048, 4): through set_head (fused after the average pool) and as a module on the feature map."""
    from models.models import Classifier
    cls_sd = W.make_head_state_dict(22, 'classifier', num_features=2048)
    x = bag[1][:6]
    with torch.no_grad():
        fm = B.trunk(sd, x)
        s = 1.0
        while float(R.classifier(cls_sd, fm).abs().max()) * s > 16.0:       # the contract is stated for |logit| <= 16: a power of two, so exact
            s *= 0.5
        cls_sd = {k: v * s for k, v in cls_sd.items()}
        ref = R.classifier(cls_sd, fm)
    head = Classifier(2048, 4)
    head.load_state_dict(cls_sd)
    head = head.cuda().eval()
    try:
        eng.set_head((head.fc[0].weight, head.fc[0].bias))
        feat, logits, fmap = eng.forward_f32(x.to(dev), feat=True, logits=True, fmap=True)
    finally:
        eng.set_head(None)
    with torch.no_grad():
        mod = head(fmap)
    e1, e2 = float((logits.cpu() - ref).abs().max()), float((mod.cpu() - ref).abs().max())
    print('Classifier(2048, 4): fused head err %.2e, module err %.2e at max |logit| %.2f' % (e1, e2, float(ref.abs().max())))
    assert float(ref.abs().max()) <= 16.0 and logits.shape == (6, 4) and feat.shape == (6, 2048)
    assert e1 <= LOGIT_TOL and e2 <= LOGIT_TOL
    with pytest.raises(RuntimeError, match='no head'):
        eng.forward_f32(x.to(dev), logits=True)


def test_speed_mode_is_sane(dev, sd, bag, ref_taps):
    """planes 1 (single-pass bf16) through 53 convs: outside the contract; a finite result within 0.1 of the tap's maximum."""
    from wsi_segmentation_pipeline_amd.engine import BottleneckEngine
    e = BottleneckEngine(sd, dev, planes=1)
    got = e.forward_f32(bag[1][:6].to(dev), tap=16)
    err = _rel(got, ref_taps['layer4.2'])
    print('resnet50 speed mode: last tap rel err %.2e' % err)
    assert np.isfinite(err) and err <= 0.1


def test_recorded_bounds_match_the_profile():
    """profiles/resnet50_parity.json holds the measured values; they are inside the bounds above."""
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'resnet50_parity.json')))
    assert rec['taps_worst_rel_err']['parity'] == TAP_MEASURED and rec['tap_bound']['parity'] == TAP_TOL
    assert rec['logit_abs_err']['parity'] == LOGIT_MEASURED and rec['logit_bound'] == LOGIT_TOL
    assert TAP_MEASURED <= TAP_TOL and max(LOGIT_MEASURED.values()) <= LOGIT_TOL
