"""GPU tests of the cellularity scoring path: the view producer (wsi_tile_views_u8 / wsi_views_f32) byte for byte against the host
model, the MLP head over views (wsi_mlp_views) against a float64 model inside the a-priori fp32 bound and its mean / clamp bit for
bit, engine.forward_views and the drivers of utils.eval against the reference's own outputs (tests/golden/cellularity_views.npz,
tools/gen_golden_cellularity.py).  Contract: max abs output error <= 1e-3 vs the reference fp32 CPU path, stated for |output| <= 16."""
import json
import os

import numpy as np
import pytest
import torch

import bottleneck_oracle as B
import views_oracle as VO
from oracle import resnet_oracle as R
from wsi_segmentation_pipeline_amd import engine as E
from wsi_segmentation_pipeline_amd import synthetic as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3
U = 2.0 ** -24
XY = [(1, 1), (5, 7), (103, 43)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def fx():
    return VO.load_fixture()


def _view_lists(ph, pw):
    return [list(range(8))] if ph == pw else [[0, 2, 4, 6], [1, 3, 5, 7], [5, 1, 1]]


# ------------------------------------------------------------------------------------------------------------------ view bytes
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('ph,pw', [(32, 32), (32, 64), (96, 64)])
def test_tile_views_u8_bytes(dev, ph, pw, n):
    rng = np.random.default_rng(100 * ph + pw + n)
    padded = rng.integers(0, 256, (140, 208, 3), dtype=np.uint8)
    slide = torch.from_numpy(padded).to(dev)[:, :200]                    # 140 x 200, row pitch 624 > 3 * 200
    assert slide.stride(0) == 624 and tuple(slide.shape) == (140, 200, 3)
    xy = np.array(XY[:n], np.int32)
    tiles = [padded[y:y + ph, x:x + pw] for x, y in xy]
    for views in _view_lists(ph, pw):
        atlas, axy = E.tile_views(slide, torch.from_numpy(xy).to(dev), ph, pw, views)
        hv, wv = VO.view_shape(views[0], ph, pw)
        assert tuple(atlas.shape) == (len(views) * n * hv, wv, 3) and atlas.dtype == torch.uint8 and atlas.is_contiguous()
        want = np.concatenate([VO.apply_view(t, v) for v in views for t in tiles])
        assert np.array_equal(atlas.cpu().numpy(), want), views
        assert np.array_equal(axy.cpu().numpy(), np.array([(0, i * hv) for i in range(len(views) * n)], np.int32))
    if ph != pw:
        with pytest.raises(ValueError):
            E.tile_views(slide, torch.from_numpy(xy).to(dev), ph, pw, [0, 1])


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('h,w', [(32, 32), (32, 64), (96, 64)])
def test_views_f32_bits(dev, h, w, n):
    rng = np.random.default_rng(7 * h + w + n)
    x = rng.standard_normal((n, 3, h, w)).astype(np.float32)
    for views in _view_lists(h, w):
        got = E.views_f32(torch.from_numpy(x).to(dev), views)
        want = np.concatenate([VO.apply_view(x, v, (2, 3)) for v in views])
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), views


# ------------------------------------------------------------------------------------------------------------------ MLP head
def _mlp_case(f, j, k, nviews, n, seed, spread=1.0, shift=0.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nviews * n, f)).astype(np.float32)
    last = j if j else f
    w2 = (rng.uniform(-1, 1, (k, last)) * spread / np.sqrt(last)).astype(np.float32)
    b2 = (rng.uniform(-0.05, 0.05, k) + shift).astype(np.float32)
    if not j:
        return x, (w2, b2)
    w1 = (rng.uniform(-1, 1, (j, f)) / np.sqrt(f)).astype(np.float32)
    b1 = rng.uniform(-0.05, 0.05, j).astype(np.float32)
    return x, (w1, b1, w2, b2)


def _mlp_f64(x, mlp):
    """(outputs, a-priori fp32 bound) of the float64 model, both (rows, k)"""
    x = x.astype(np.float64)
    if len(mlp) == 2:
        w2, b2 = (a.astype(np.float64) for a in mlp)
        f = x.shape[1]
        return x @ w2.T + b2, 2 * (f + 2) * U * (np.abs(x) @ np.abs(w2).T + np.abs(b2))
    w1, b1, w2, b2 = (a.astype(np.float64) for a in mlp)
    f, j = w1.shape[1], w1.shape[0]
    e1 = (f + 2) * U * (np.abs(x) @ np.abs(w1).T + np.abs(b1))
    y1 = np.maximum(x @ w1.T + b1, 0.0)
    return y1 @ w2.T + b2, 2 * ((j + 2) * U * ((y1 + e1) @ np.abs(w2).T + np.abs(b2)) + e1 @ np.abs(w2).T)


def _check_mlp(dev, x, mlp, nviews, n, clamp=None):
    mean, pv = E.mlp_views(torch.from_numpy(x).to(dev), n, nviews, [torch.from_numpy(a) for a in mlp], clamp=clamp, per_view=True)
    mean, pv = mean.cpu().numpy(), pv.cpu().numpy()
    ref, bound = _mlp_f64(x, mlp)
    err = np.abs(pv - ref)
    print('mlp_views: worst error / bound %.3f (max error %.2e)' % (float((err / bound).max()), float(err.max())))
    assert pv.shape == ref.shape and (err <= bound).all()
    k = pv.shape[1]
    want = VO.mean_views(pv.reshape(nviews, n, k).transpose(1, 0, 2))
    if clamp is not None:
        want = np.minimum(np.maximum(want, np.float32(clamp[0])), np.float32(clamp[1]))
    assert np.array_equal(mean.view(np.uint32), want.view(np.uint32))
    mean_only = E.mlp_views(torch.from_numpy(x).to(dev), n, nviews, [torch.from_numpy(a) for a in mlp], clamp=clamp)[0]
    assert np.array_equal(mean_only.cpu().numpy().view(np.uint32), mean.view(np.uint32))       # views_out is optional
    return mean, pv


@pytest.mark.parametrize('n', [1, 3, 65])
@pytest.mark.parametrize('nviews', [1, 3, 4])
@pytest.mark.parametrize('f,j,k', [(64, 16, 1), (512, 128, 1), (2048, 512, 4), (512, 0, 4)])
def test_mlp_views(dev, f, j, k, nviews, n):
    x, mlp = _mlp_case(f, j, k, nviews, n, seed=f + 7 * j + 13 * k + 101 * nviews + n)
    _check_mlp(dev, x, mlp, nviews, n)


def test_mlp_views_clamp(dev):
    """Scores below 0, inside (0, 1) and above 1 before the clamp; nviews = 3 exercises the division.  The views of a patch are small
    perturbations of one feature row (as orientations of one patch are), and fc.2.bias centres the scores on 0.5."""
    for nviews in (3, 4):
        x, mlp = _mlp_case(64, 16, 1, nviews, 65, seed=5 + nviews, spread=6.0)
        rng = np.random.default_rng(nviews)
        x = (np.tile(x[:65], (nviews, 1)) + 0.05 * rng.standard_normal(x.shape)).astype(np.float32)
        centre = np.median(_mlp_f64(x, mlp)[0].reshape(nviews, 65).mean(0))
        mlp = mlp[:3] + ((mlp[3] + 0.5 - centre).astype(np.float32),)
        ref = _mlp_f64(x, mlp)[0].reshape(nviews, 65).mean(0)
        assert (ref < -0.05).any() and ((ref > 0.05) & (ref < 0.95)).any() and (ref > 1.05).any()      # a property of the inputs
        mean, _ = _check_mlp(dev, x, mlp, nviews, 65, clamp=(0.0, 1.0))
        assert (mean == 0.0).any() and (mean == 1.0).any() and ((mean > 0.0) & (mean < 1.0)).any()


# ------------------------------------------------------------------------------------------------------------------ engine
def _slide_of(u8_nchw, dev):
    """The patches at unaligned corners of one u8 slide: (slide (SH, SW, 3) on the device, tile_xy (N, 2) int32 on the device)"""
    n, _, h, w = u8_nchw.shape
    rng = np.random.default_rng(3)
    slide = rng.integers(0, 256, (h + 9, n * (w + 5) + 7, 3), dtype=np.uint8)
    xy = np.array([(3 + i * (w + 5), 1 + (i * 3) % 8) for i in range(n)], np.int32)
    for (x, y), p in zip(xy, u8_nchw):
        slide[y:y + h, x:x + w] = p.transpose(1, 2, 0)
    return torch.from_numpy(slide).to(dev), torch.from_numpy(xy).to(dev)


def _mlp_of(sd):
    """(w1, b1, w2, b2) of a Regressor state dict, (w, b) of a Classifier's"""
    return tuple(sd[k] for k in ('fc.0.weight', 'fc.0.bias', 'fc.2.weight', 'fc.2.bias') if k in sd)


@pytest.fixture(scope='module')
def eng18(fx, dev):
    return E.TrunkEngine(fx['sd'], dev, planes=E.PARITY)


def _check_against_fixture(fx, name, mean, pv, clamped, cls_pv):
    errs = {'reg_views': np.abs(pv[..., 0] - fx['reg_views_' + name]).max(), 'reg_mean': np.abs(mean[:, 0] - fx['reg_mean_' + name]).max(),
            'reg_clamped': np.abs(clamped[:, 0] - fx['reg_clamped_' + name]).max(), 'cls_views': np.abs(cls_pv - fx['cls_views_' + name]).max()}
    print('forward_views %s vs the reference: %s' % (name, {k: '%.2e' % v for k, v in errs.items()}))
    assert all(v <= TOL for v in errs.values()), errs


@pytest.mark.parametrize('name', ['sq', 'ns'])
@pytest.mark.parametrize('path', ['x', 'u8'])
def test_forward_views_resnet18_parity(dev, fx, eng18, name, path):
    """Every per-view output, the mean and the clamped mean of the fixture (64 x 64: one trunk pass; 64 x 96: the two-pass route)."""
    u8 = fx['u8_' + name]
    if path == 'x':
        src = dict(x=R.normalize_u8(u8).to(dev))
    else:
        slide, xy = _slide_of(u8, dev)
        src = dict(slide_u8=slide, tile_xy=xy, ph=u8.shape[2], pw=u8.shape[3])
    mean, pv = eng18.forward_views(mlp=_mlp_of(fx['reg']), per_view=True, **src)
    assert tuple(mean.shape) == (len(u8), 1) and tuple(pv.shape) == (len(u8), 4, 1)
    clamped = eng18.forward_views(mlp=_mlp_of(fx['reg']), clamp=(0.0, 1.0), **src)
    _, cls_pv = eng18.forward_views(mlp=_mlp_of(fx['cls']), per_view=True, **src)
    _check_against_fixture(fx, name, mean.cpu().numpy(), pv.cpu().numpy(), clamped.cpu().numpy(), cls_pv.cpu().numpy())
    assert np.array_equal(clamped.cpu().numpy(), np.minimum(np.maximum(mean.cpu().numpy(), 0.0), 1.0))
    small = E.TrunkEngine(fx['sd'], dev, planes=E.PARITY, max_batch=8)   # chunks of two patches: the views of a patch stay together
    mean2, pv2 = small.forward_views(mlp=_mlp_of(fx['reg']), per_view=True, **src)
    assert float((mean2 - mean).abs().max()) <= 1e-5 and float((pv2 - pv).abs().max()) <= 1e-5


@pytest.mark.parametrize('name', ['sq', 'ns'])
def test_u8_view_features_bit_equal_torch_atlas(dev, fx, eng18, name):
    """The features of the u8 view path are those of forward_tiles on an atlas built with torch ops from the same tiles, in the same
    batches: same kernels, same bytes."""
    from utils.eval import torch_view
    u8 = fx['u8_' + name]
    n, _, h, w = u8.shape
    slide, xy = _slide_of(u8, dev)
    ids = list(E.VIEWS_REFERENCE)
    got = eng18.views_features(ids, None, slide, xy, h, w)
    assert tuple(got.shape) == (4 * n, 512)
    tiles = torch.from_numpy(u8).to(dev)
    want = [None] * 4
    for g in E.view_groups(ids, h, w):
        atlas = torch.cat([torch_view(tiles, ids[k]) for k in g]).permute(0, 2, 3, 1).contiguous()      # (V n, hv, wv, 3)
        rows, hv, wv = atlas.shape[0], atlas.shape[1], atlas.shape[2]
        axy = torch.tensor([(0, i * hv) for i in range(rows)], dtype=torch.int32, device=dev)
        f = eng18.forward_tiles(atlas.view(rows * hv, wv, 3), axy, hv, wv, feat=True, logits=False)[0]
        for i, k in enumerate(g):
            want[k] = f[i * n:(i + 1) * n]
    assert torch.equal(got, torch.cat(want))


def test_forward_views_auto_and_mx_measured(dev, fx):
    """'auto' and mx on the fixture: the error is measured and recorded (profiles/cellularity_parity.json) with the engine's report;
    it is asserted finite, not bounded - nothing had been measured when this test was written."""
    u8 = fx['u8_sq']
    slide, xy = _slide_of(u8, dev)
    out = {}
    auto = E.AutoTrunkEngine(fx['sd'], dev)
    for label, eng in (('auto', auto), ('mx', E.TrunkEngine(fx['sd'], dev, planes=E.MX))):
        for path, src in (('x', dict(x=R.normalize_u8(u8).to(dev))), ('u8', dict(slide_u8=slide, tile_xy=xy, ph=64, pw=64))):
            mean, pv = eng.forward_views(mlp=_mlp_of(fx['reg']), per_view=True, **src)
            out['%s_%s' % (label, path)] = {'reg_views_max_err': float(np.abs(pv.cpu().numpy()[..., 0] - fx['reg_views_sq']).max()),
                                            'reg_mean_max_err': float(np.abs(mean.cpu().numpy()[:, 0] - fx['reg_mean_sq']).max())}
    report = dict(auto.report)
    assert report['mode'] in ('mx', 'parity') and report.get('scope') == 'views'
    chosen = auto._chosen
    auto.forward_views(mlp=_mlp_of(fx['reg']), slide_u8=slide.clone(), tile_xy=xy, ph=64, pw=64)
    assert auto._chosen is chosen and auto.report == report                # a new atlas tensor does not probe again
    auto.reset()
    assert auto._chosen is None
    out['auto_report'] = report
    out['note'] = 'ResNet-18, fixture tests/golden/cellularity_views.npz (6 patches of 64 x 64, 4 views), max abs error against the reference'
    print('cellularity parity:', out)
    with open(os.path.join(ROOT, 'profiles', 'cellularity_parity.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    assert all(np.isfinite(v) for d in out.values() if isinstance(d, dict) for v in d.values() if isinstance(v, float))


def test_forward_views_bottleneck(dev):
    """ResNet(Bottleneck, [1, 1, 1, 1]) + Regressor(2048, 1) against the CPU restatement."""
    sd = W.make_bottleneck_state_dict(21, [1, 1, 1, 1], with_fc=False)
    reg = W.make_head_state_dict(41, 'regressor', 2048, 1)
    cls = W.make_head_state_dict(42, 'classifier', 2048, 4)
    u8 = W.make_u8_patches(43, (3, 3, 64, 64))
    ref, ref_cls = VO.restate(sd, reg, cls, u8, trunk=B.trunk)
    assert max(np.abs(ref).max(), np.abs(ref_cls).max()) <= 16.0
    eng = E.BottleneckEngine(sd, dev, planes=E.PARITY)
    slide, xy = _slide_of(u8, dev)
    for src in (dict(x=R.normalize_u8(u8).to(dev)), dict(slide_u8=slide, tile_xy=xy, ph=64, pw=64)):
        mean, pv = eng.forward_views(mlp=_mlp_of(reg), per_view=True, **src)
        err = max(float(np.abs(pv.cpu().numpy()[..., 0] - ref).max()), float(np.abs(mean.cpu().numpy()[:, 0] - VO.mean_views(ref)).max()))
        print('bottleneck forward_views max error %.2e' % err)
        assert err <= TOL


# ------------------------------------------------------------------------------------------------------------------ drivers
class _Generic(torch.nn.Module):
    """any GPU model with .encoder / .regressor / .classifier: the reference's module loop"""

    def __init__(self, net, classifier, regressor):
        super().__init__()
        from utils.eval import TrunkEncoder
        self.encoder, self.classifier, self.regressor = TrunkEncoder(net), classifier, regressor


@pytest.fixture(scope='module')
def models(fx, dev):
    import resnets_shift
    from models import models as M
    from utils import eval as val
    net = resnets_shift.resnet18(False, precision='parity')
    missing = net.load_state_dict(fx['sd'], strict=False)
    assert all(k.startswith('fc') for k in missing.missing_keys)
    reg, cls = M.Regressor(512, 1), M.Classifier(512, 4)
    reg.load_state_dict(fx['reg'])
    cls.load_state_dict(fx['cls'])
    return val.SlideClassifierModel(net, cls, reg).to(dev), _Generic(net, cls, reg).to(dev)


def _iterator(fx):
    """two batches of the square patches as the patch iterator yields them; items 1 and 4 are no classification items"""
    x = R.normalize_u8(fx['u8_sq'])
    is_cls = torch.tensor([True, False, True, True, False, True])
    code = torch.tensor([1, 0, 0, 1, 1, 2])
    lab = torch.zeros((6, 64, 64), dtype=torch.int64)
    f = torch.zeros(6, dtype=torch.bool)
    return [(x[a:b], lab[a:b], is_cls[a:b], f[a:b], f[a:b], code[a:b]) for a, b in ((0, 4), (4, 6))], is_cls.numpy(), code.numpy()


def test_predict_reg_and_cls(fx, models, capsys):
    from utils import eval as val
    it, is_cls, code = _iterator(fx)
    outs = []
    for model in models:
        model.train()
        r = val.predict_reg(model, it, 7)
        assert model.training
        assert np.array_equal(r['gts'], code) and r['preds'].shape == (6,)
        assert np.abs(r['preds'] - fx['reg_mean_sq']).max() <= TOL
        assert r['l1'] == pytest.approx(np.mean(np.abs(r['preds'] - code))) and r['mse'] == pytest.approx(np.mean((r['preds'] - code) ** 2))
        assert 'Ep. 7, l1 %.3f, mse %.3f, ' % (r['l1'], r['mse']) in capsys.readouterr().out
        c = val.predict_cls(model, it, 7)
        want = np.argmax(fx['cls_views_sq'][:, 0], 1)[is_cls]
        assert np.array_equal(c['gts'], code[is_cls]) and np.array_equal(c['preds'], want)
        assert (c['acc'], c['f1']) == val.cls_scores(code[is_cls], want)
        assert 'Ep. 7, acc %.3f,f1 %.3f' % (c['acc'], c['f1']) in capsys.readouterr().out
        outs.append(r['preds'])
    assert np.abs(outs[0] - outs[1]).max() <= 2e-3                        # fused path vs the module loop


def test_predict_breastpathq(fx, models, tmp_path, monkeypatch):
    from PIL import Image
    from myargs import args
    from utils import eval as val
    monkeypatch.setattr(args, 'tile_w', 64)
    monkeypatch.setattr(args, 'tile_h', 64)
    order = [(4, 2), (1, 1), (9, 3), (4, 1), (2, 2), (7, 7), (5, 1)]
    for (a, b), p in zip(order, fx['u8_sq']):
        Image.fromarray(np.ascontiguousarray(p.transpose(1, 2, 0))).save(str(tmp_path / ('%d_%d.tif' % (a, b))))
    big = W.make_u8_patches(77, (96, 80, 3))                              # 96 rows x 80 columns: really resized
    Image.fromarray(big).save(str(tmp_path / '5_1.tif'))
    resized = np.asarray(Image.fromarray(big).resize((64, 64), Image.BILINEAR))
    ref_big = VO.mean_views(VO.restate(fx['sd'], fx['reg'], fx['cls'], resized.transpose(2, 0, 1)[None])[0])
    want = np.concatenate([fx['reg_clamped_sq'], np.minimum(np.maximum(ref_big, 0.0), 1.0)])
    labels = tmp_path / 'labels.csv'
    labels.write_text('slide,rid,y\n' + ''.join('%d,%d,0.1\n' % ab for ab in order))
    got = []
    for k, model in enumerate(models):
        out = tmp_path / ('out%d.csv' % k)
        rows = val.predict_breastpathq(model, 2, str(tmp_path), str(labels), out_csv=str(out), batch=(None if k == 0 else 3))
        assert [(a, b) for a, b, _ in rows] == order
        p = np.array([v for _, _, v in rows], np.float32)
        assert np.abs(p - want).max() <= TOL and p.min() >= 0.0 and p.max() <= 1.0
        assert out.read_bytes().decode() == 'slide,rid,p\r\n' + ''.join('%d,%d,%s\r\n' % (a, b, v) for a, b, v in rows)
        got.append(p)
    assert (got[0] == 0.0).any() and ((got[0] > 0.0) & (got[0] < 1.0)).any()
    assert np.abs(got[0] - got[1]).max() <= 2e-3
