"""GPU parity of BasicBlock trunks deeper (and shallower) than ResNet-18 on the HIP path: ResNet-34 = [3, 4, 6, 3] against the
reference's own outputs (tests/golden/resnet34_bag64.npz, tools/gen_golden_resnet34.py) and against the depth-general CPU
restatement (tests/depth_oracle.py); [1, 1, 1, 1], where every strided block is also its stage's last block.
Contract (BASELINE.json north_star): max abs logit error <= 1e-3 vs the reference fp32 CPU path."""
import json
import os

import numpy as np
import pytest
import torch

import depth_oracle as D
from oracle import resnet_oracle as R
from oracle import wsi_oracle as WO
from wsi_segmentation_pipeline_amd import synthetic as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_TOL = 1e-3          # BASELINE.json north_star: "within 1e-3 on the output logits"
R34 = [3, 4, 6, 3]
# Worst tap of the 17 (pool + 16 blocks), relative to the tap's maximum, measured on an MI355X against the restatement (64 x 64, N = 6;
# profiles/resnet34_parity.json): parity TAP_MEASURED[2], mx TAP_MEASURED[3].  The bound is 3 x the measured value rounded up to one
# digit, the headroom tests/test_gpu_trunk.py documents for the 8-block net (2e-4 there).  Measured: parity 2.09e-6 (layer4.0), mx
# 5.62e-5 (layer2.1) - no growth with depth beyond the 8-block net's 7e-5 in mx.
TAP_MEASURED = {2: 2.09e-6, 3: 5.62e-5}
TAP_TOL = {2: 7e-6, 3: 2e-4}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def sd():
    return W.make_resnet_state_dict(11, R34)


@pytest.fixture(scope='module')
def bag():
    """the fixture's input bag: u8 (32, 3, 64, 64), image index b * P + p, and its normalised form"""
    u8 = W.make_u8_patches(12, (2, 16, 3, 64, 64)).reshape(-1, 3, 64, 64)
    return u8, R.normalize_u8(u8)


@pytest.fixture(scope='module')
def ref_taps(sd, bag):
    """restatement taps of the first six bag images, computed once"""
    taps = {}
    with torch.no_grad():
        D.trunk(sd, bag[1][:6], taps)
    return taps


def _rel(got, ref):
    return float((got.cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('planes', [2, 3])
def test_taps_vs_restatement_64(dev, sd, bag, ref_taps, planes):
    """Every tap 0..16 on the ordinary-PF route: weight indexing and block order down to the 2 x 2 maps of layer 4."""
    from wsi_segmentation_pipeline_amd.engine import TrunkEngine
    eng = TrunkEngine(sd, dev, planes=planes)
    assert eng.layers == R34
    x = bag[1][:6].to(dev)
    names = D.tap_names(R34)
    assert len(names) == 17
    report = []
    for i, name in enumerate(names):
        got = eng.forward_f32(x, tap=i)
        assert got.shape == ref_taps[name].shape, name
        report.append((name, _rel(got, ref_taps[name])))
    print('planes=%d tap errors (rel to max):' % planes, report, 'worst %.3e' % max(e for _, e in report))
    with pytest.raises(ValueError):
        eng.forward_f32(x, tap=18)
    for name, err in report:
        assert err <= TAP_TOL[planes], report


def _bag_forward(dev, sd, bag, precision, golden_dir):
    import resnets_shift
    g = np.load(os.path.join(golden_dir, 'resnet34_bag64.npz'))
    model = resnets_shift.resnet34(precision=precision)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    with torch.no_grad():
        singles, ens = model(bag[1].view(2, 16, 3, 64, 64).to(dev))
    return (float(np.abs(singles.cpu().numpy() - g['singles']).max()), float(np.abs(ens.cpu().numpy() - g['ensemble']).max()), model)


def test_bag_forward_parity_vs_reference_fixture(dev, sd, bag, golden_dir):
    """resnets_shift.ResNet.forward at [3, 4, 6, 3], full run (phase-split hand-overs), against the reference's outputs."""
    e1, e2, _ = _bag_forward(dev, sd, bag, 'parity', golden_dir)
    print('resnet34 bag64 parity: max abs err singles %.2e ensemble %.2e' % (e1, e2))
    assert e1 <= LOGIT_TOL and e2 <= LOGIT_TOL


def test_bag_forward_auto_vs_reference_fixture(dev, sd, bag, golden_dir):
    e1, e2, model = _bag_forward(dev, sd, bag, 'auto', golden_dir)
    report = model.hip_engine().report
    print('resnet34 bag64 auto: max abs err singles %.2e ensemble %.2e; mode %s (%s)' % (e1, e2, report['mode'], report['reason']))
    assert report['mode'] in ('mx', 'parity')
    assert e1 <= LOGIT_TOL and e2 <= LOGIT_TOL


def test_bag_forward_mx_vs_reference_fixture(dev, sd, bag, golden_dir):
    """Raw mx (96-byte lines in layer 1, phase-split hand-overs, folded downsamples) at this depth and logit scale (|logit| up to 15).
    Measured on an MI355X (profiles/resnet34_parity.json): singles 1.13e-3, ensemble 2.4e-4 - above 5e-4, the auto policy's own
    threshold of half the contract, so nothing is asserted for raw mx here beyond a sane result: at 16 blocks and |logit| 15 the default
    ('auto', probe error 1.12e-3) resolves to parity, which test_bag_forward_auto_vs_reference_fixture holds to the contract
    (DESIGN.md section 3).  The figures are printed for the record."""
    e1, e2, _ = _bag_forward(dev, sd, bag, 'mx', golden_dir)
    print('resnet34 bag64 mx: max abs err singles %.2e ensemble %.2e' % (e1, e2))
    assert np.isfinite(e1) and np.isfinite(e2) and e1 <= 0.1 and e2 <= 0.1         # (a wrong weight index or block order is O(1))


@pytest.mark.parametrize('planes', [2, 3])
def test_full_run_equals_last_tap(dev, sd, planes):
    """forward_f32(fmap=True) - 96-byte lines, phase-split hand-overs, folds: the routes taps 0..15 never take - against tap 16.  The
    last tap runs every block, so by the library's rule ('all blocks' = the full route) it takes the same hand-overs and measured
    identical to the bit; the ordinary-PF route is therefore also asked for explicitly: tap 16 with 128-byte layer-1 lines, no
    phase split and no downsample fold (the routes every earlier tap takes), and a tap in the middle of a stage in between, which
    re-tags the stage-0 layout.  N = 5, then N = 3 on the same engine (a workspace planned for a larger batch); 64 x 288 with
    N = 2: layer 1's output is 36 wide, so stage 0 hands over ordinary 128-byte lines while the deeper stages still split."""
    from wsi_segmentation_pipeline_amd import native
    from wsi_segmentation_pipeline_amd.engine import TrunkEngine
    M = native.ConvMode
    eng = TrunkEngine(sd, dev, planes=planes)
    for n, h, w in ((5, 64, 64), (3, 64, 64), (2, 64, 288)):
        x = R.normalize_u8(W.make_u8_patches(50 + n + w, (n, 3, h, w))).to(dev)
        full = eng.forward_f32(x, fmap=True)[2].clone()
        tap = eng.forward_f32(x, tap=16).clone()
        eng.forward_f32(x, tap=2)                                           # 128-byte lines in the stage-0 buffers, then back
        again = eng.forward_f32(x, fmap=True)[2].clone()
        with native.conv_mode(M.NO_S2_SPLIT | M.L1_LINES128 | M.NO_DS_FOLD):
            plain = eng.forward_f32(x, tap=16).clone()
        assert full.shape == tap.shape == plain.shape == (n, 512, h // 32, w // 32)
        err = float((full - tap).abs().max() / tap.abs().max())
        perr = float((full - plain).abs().max() / plain.abs().max())
        print('planes=%d N=%d %dx%d: full run vs tap 16 rel err %.2e, vs tap 16 on the ordinary-PF route %.2e' % (planes, n, h, w, err, perr))
        assert torch.equal(full, again)
        assert err <= TAP_TOL[planes] and perr <= TAP_TOL[planes]


def test_u8_slide_path_equals_f32_path(dev, sd):
    """forward_tiles on a 200 x 260 slide, four 64 x 64 tiles, one hanging over the edge, against forward_f32 of the gathered tiles
    (tolerances of tests/test_gpu_trunk.py::test_u8_slide_path_equals_f32_path)."""
    from wsi_segmentation_pipeline_amd.engine import TrunkEngine
    rng = np.random.default_rng(7)
    slide = rng.integers(0, 256, (200, 260, 3), dtype=np.uint8)
    xy = np.array([[0, 0], [100, 50], [260 - 64, 200 - 64], [230, 170]], np.int32)
    tiles = np.stack([WO.read_tile(slide, int(x), int(y), 64, 64) for x, y in xy]).transpose(0, 3, 1, 2)
    x = R.normalize_u8(tiles)
    for planes in (2, 3):
        eng = TrunkEngine(sd, dev, planes=planes)
        sl, xyd = torch.from_numpy(slide).to(dev), torch.from_numpy(xy).to(dev)
        b = eng.forward_f32(x.to(dev), feat=True)[0].clone()
        a = eng.forward_tiles(sl, xyd, 64, 64, feat=True, logits=False)[0].clone()
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        print('planes=%d u8 slide path vs f32 path: %.2e of scale %.2e' % (planes, err, scale))
        assert err <= (2e-5 if planes == 2 else 1e-3) * scale


@pytest.mark.parametrize('planes', [2, 3])
def test_single_block_stages(dev, planes):
    """[1, 1, 1, 1]: the strided block is the stage's last block, so the folded downsample and the phase-split output meet in one
    conv and the fold must win (the next stage then enters through the unsplit stride-2 kernel)."""
    from wsi_segmentation_pipeline_amd.engine import TrunkEngine
    sd1 = W.make_resnet_state_dict(11, [1, 1, 1, 1], with_fc=False)
    x = R.normalize_u8(W.make_u8_patches(61, (4, 3, 64, 64)))
    with torch.no_grad():
        ref = D.trunk(sd1, x)
    eng = TrunkEngine(sd1, dev, planes=planes)
    assert eng.layers == [1, 1, 1, 1]
    got = eng.forward_f32(x.to(dev), fmap=True)[2]
    tap = eng.forward_f32(x.to(dev), tap=4)
    err, terr = _rel(got, ref), _rel(tap, ref)
    print('planes=%d [1,1,1,1]: full run rel err %.2e, tap 4 rel err %.2e' % (planes, err, terr))
    assert got.shape == ref.shape
    assert err <= TAP_TOL[planes] and terr <= TAP_TOL[planes]


def test_unet_resnet34_encoder(dev):
    """UNetSeg(classes=4, encoder='resnet34'), parity mode, 64 x 64, N = 3: logits against oracle.unet_oracle.decoder on the
    restatement's encoder maps, ABSOLUTE 1e-3 at max |logit| 16 (the bound of tests/test_gpu_unet.py at its smallest shape, final
    conv scaled the same way); the five encoder maps within the tap bound."""
    from wsi_segmentation_pipeline_amd.unet import UNetSeg
    sd = W.make_unet_resnet_state_dict(7, R34, 4)
    x = R.normalize_u8(W.make_u8_patches(41, (3, 3, 64, 64)))
    with torch.no_grad():
        s = 16.0 / float(D.unet_forward(sd, x)[0].abs().max())
    for key in ('decoder.final_conv.weight', 'decoder.final_conv.bias'):
        sd[key] = sd[key] * s
    with torch.no_grad():
        ref, ref_enc = D.unet_forward(sd, x)
    model = UNetSeg(classes=4, encoder='resnet34')
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    with torch.no_grad():
        got = model(x.cuda())
        enc = model.encoder(x.cuda())
    scale = float(ref.abs().max())
    assert abs(scale - 16.0) < 1e-3 and got.shape == ref.shape == (3, 4, 64, 64)
    err = float((got.cpu() - ref).abs().max())
    enc_err = [_rel(a, b) for a, b in zip(enc, ref_enc)]
    print('unet resnet34 parity: max |logit - spec| %.2e ABSOLUTE at max |logit| %.1f; encoder maps rel err %s' % (err, scale, ['%.1e' % e for e in enc_err]))
    assert [tuple(t.shape[1:]) for t in enc] == [(512, 2, 2), (256, 4, 4), (128, 8, 8), (64, 16, 16), (64, 32, 32)]
    assert err <= 1e-3
    assert max(enc_err) <= TAP_TOL[2]


def test_recorded_bounds_match_the_profile():
    """profiles/resnet34_parity.json holds the measured values the bounds above come from."""
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'resnet34_parity.json')))
    for planes, mode in ((2, 'parity'), (3, 'mx')):
        assert rec['taps_worst_rel_err'][mode] == TAP_MEASURED[planes]
        assert rec['tap_bound'][mode] == TAP_TOL[planes] and 3 * TAP_MEASURED[planes] <= TAP_TOL[planes] <= 6 * TAP_MEASURED[planes]
