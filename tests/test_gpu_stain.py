"""GPU tests of the stain normalisation (csrc/stain.hip, wsi_segmentation_pipeline_amd/stain.py) against the float64 spec
(tests/stain_oracle.py): the fit kernels' moments and histograms, the two applies byte for byte, the fitted parameters end to end, and
the hooks of utils.dataset / utils.eval.

Shapes: 1 x 1 (one pixel), 1 x 17 (just past one 16-pixel piece), 7 x 9 (189 bytes), 64 x 64 (a clean chunk), 65 x 63 (a ragged one), each
as one image and as a batch of three whose image starts are misaligned and whose middle image is all white.  The oracle's results are
computed once per case."""
import math

import numpy as np
import pytest
import torch

import stain_oracle as SO
from wsi_segmentation_pipeline_amd import stain

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 17), (7, 9), (64, 64), (65, 63)]
CASES = [(h, w, n) for h, w in SHAPES for n in (1, 3)]
ANGLE_BIN = 2 * math.pi / stain.ANGLE_BINS
CONC_BIN = stain.CONC_MAX / stain.CONC_BINS


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


class Case:
    """n images of h x w cut from 128 x 128 parents at a tissue pixel (image 1 of a batch: all white), with the oracle's fit of every
    parent: parameters that are valid whatever the crop holds."""

    def __init__(self, h, w, n):
        parents = SO.shifted_he(40 + h + w, n, 128)
        self.imgs, self.fits = np.empty((n, h, w, 3), np.uint8), []
        for i, p in enumerate(parents):
            ys, xs = np.nonzero(SO.tissue(p))
            k = int(np.argmin((ys - 64) ** 2 + (xs - 64) ** 2))
            y0, x0 = min(int(ys[k]), 128 - h), min(int(xs[k]), 128 - w)
            self.imgs[i] = p[y0:y0 + h, x0:x0 + w]
            self.fits.append({'plane': SO.macenko_plane(p), 'macenko': SO.fit_macenko(p), 'reinhard': SO.fit_reinhard(p)})
        if n == 3:
            self.imgs[1] = 255
        self.target = SO.fit_reinhard(SO.shifted_he(7, 1, 128, (1.0, 1.0, 1.0))[0])
        self.n = [int(SO.tissue(im).sum()) for im in self.imgs]

    def macenko_params(self):
        return [stain.MacenkoParams(f['macenko'][0], f['macenko'][1], f['macenko'][2]) for f in self.fits]

    def reinhard_params(self):
        return [stain.ReinhardParams(f['reinhard'][0], f['reinhard'][1], f['reinhard'][2]) for f in self.fits]


_cases = {}


@pytest.fixture(params=CASES, ids=lambda c: '%dx%d-n%d' % c)
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(*request.param)
    return _cases[request.param]


def _batch(case, dev):
    x = torch.from_numpy(case.imgs).to(dev)
    return x if x.shape[0] > 1 else x[0]                        # N = 1 travels as (H, W, 3)


def _as4(x):
    return x if x.dim() == 4 else x.unsqueeze(0)


# ------------------------------------------------------------------------------------------------------------------------ moments
def test_moments(case, dev):
    """Both sides are float64 sums of the same values (od: the fp32 table; l-alpha-beta: float64 logarithms equal to a few units of 1e-16)
    over at most 4 225 pixels, so only the order of the sums differs: 1e-12 of the sum of the magnitudes (for the optical densities, which
    are all positive, that is 1e-12 relative).  The count is exact, two runs give the same bits, a white image gives zeros."""
    x = _as4(_batch(case, dev))
    for lab in (False, True):
        got = stain._moments(x, lab, stain.IO, stain.BETA)
        again = stain._moments(x, lab, stain.IO, stain.BETA)
        assert got.shape == (x.shape[0], 10) and np.array_equal(got.view(np.uint64), again.view(np.uint64))
        for i, im in enumerate(case.imgs):
            px = im[SO.tissue(im)]
            v = SO.lab_of(px) if lab else SO.od_of(px)
            want = SO.moments_vector(v.shape[0], v.sum(0), v.T @ v)
            scale = SO.moments_vector(v.shape[0], np.abs(v).sum(0), np.abs(v).T @ np.abs(v))
            err = np.abs(got[i] - want)
            print('%s image %d: n %d, worst moment error / scale %.2e' % ('lab' if lab else 'od', i, v.shape[0], float((err / np.maximum(scale, 1e-300)).max())))
            assert got[i, 0] == case.n[i] and (err <= 1e-12 * scale).all()
            if not lab:
                assert (err <= 1e-12 * np.abs(want)).all()
    if x.shape[0] == 3:
        assert case.n[1] == 0 and not got[1].any()


# --------------------------------------------------------------------------------------------------------------------- histograms
def _check_hist(dev_h, ref_h, n, what):
    assert int(dev_h.sum()) == int(ref_h.sum()) == n, what
    cd, cr = np.cumsum(dev_h), np.cumsum(ref_h)
    nxt = np.concatenate((ref_h[1:], [0]))
    moved = int(np.abs(dev_h - ref_h).sum()) // 2
    print('%s: %d of %d pixels in a neighbouring bin' % (what, moved, n))
    assert (np.abs(cd - cr) <= ref_h + nxt).all(), what         # a pixel may land in the bin next to the oracle's, never further


def test_histograms(case, dev):
    x = _as4(_batch(case, dev))
    nimg = x.shape[0]
    planes = np.stack([f['plane'] for f in case.fits])
    pinvs = np.stack([np.linalg.pinv(f['macenko'][0]) for f in case.fits])
    ah = stain._hist(x, False, planes.reshape(nimg, 6), stain.IO, stain.BETA)
    ch = stain._hist(x, True, pinvs.reshape(nimg, 6), stain.IO, stain.BETA)
    assert ah.shape == (nimg, stain.ANGLE_BINS) and ch.shape == (nimg, 2, stain.CONC_BINS)
    assert np.array_equal(ah, stain._hist(x, False, planes.reshape(nimg, 6), stain.IO, stain.BETA))
    assert np.array_equal(ch, stain._hist(x, True, pinvs.reshape(nimg, 6), stain.IO, stain.BETA))
    for i, im in enumerate(case.imgs):
        _check_hist(ah[i], SO.angle_hist(im, case.fits[i]['plane']), case.n[i], 'angle, image %d' % i)
        ref = SO.conc_hist(im, case.fits[i]['macenko'][0])
        for r in range(2):
            _check_hist(ch[i, r], ref[r], case.n[i], 'concentration %d, image %d' % (r, i))


# ------------------------------------------------------------------------------------------------------------------------ applies
def _run(case, x, method, background, out=None):
    if method == 'macenko':
        return stain.normalize_macenko(x, case.macenko_params() if x.dim() == 4 else case.macenko_params()[0], out=out, background=background)
    tgt = stain.ReinhardParams(case.target[0], case.target[1], case.target[2])
    return stain.normalize_reinhard(x, tgt, case.reinhard_params() if x.dim() == 4 else case.reinhard_params()[0], out=out, background=background)


def _oracle(case, method, background):
    out = []
    for im, f in zip(case.imgs, case.fits):
        if method == 'macenko':
            out.append(SO.apply_macenko(im, SO.macenko_matrix(f['macenko'][0], f['macenko'][1]), background))
        else:
            out.append(SO.apply_reinhard(im, f['reinhard'][:2], case.target[:2], background))
    return np.stack(out)


@pytest.mark.parametrize('background', ['keep', 'all'])
@pytest.mark.parametrize('method', ['macenko', 'reinhard'])
def test_apply_bytes(case, dev, method, background):
    """The oracle's parameters fed in: every byte within 1 of the oracle's, at most 1e-3 of them different (a condition: the fp32 host
    model of the kernel's arithmetic differs in 4e-5 of the bytes of this family at most); 'keep' copies the non-tissue bytes; in place equals
    out of place."""
    x = _batch(case, dev)
    src = x.clone()
    got = _run(case, x, method, background)
    assert torch.equal(x, src) and got.shape == x.shape and got.dtype == torch.uint8
    g = _as4(got).cpu().numpy()
    want = _oracle(case, method, background)
    diff = np.abs(g.astype(int) - want.astype(int))
    share = float((diff > 0).mean())
    print('%s %s: %d of %d bytes differ from the oracle (share %.2e), largest difference %d' % (method, background, int((diff > 0).sum()), diff.size, share, int(diff.max())))
    assert diff.max() <= 1 and share <= 1e-3
    if background == 'keep':
        bg = ~np.stack([SO.tissue(im) for im in case.imgs])
        assert np.array_equal(g[bg], case.imgs[bg])
    else:
        assert len(case.imgs) == 1 or (g[1] != 255).any()       # the white image is transformed too
    inplace = _run(case, x, method, background, out=x)
    assert inplace.data_ptr() == x.data_ptr() and torch.equal(x, got)


@pytest.mark.parametrize('method', ['macenko', 'reinhard'])
@pytest.mark.parametrize('src_off,dst_off', [(0, 64), (5, 69), (0, 61), (3, 64)])
def test_apply_guards_and_alignment(case, dev, method, src_off, dst_off):
    """Source and destination at chosen byte offsets of larger buffers: 16-byte aligned, misaligned alike (a head of pixels before the
    first 16-byte piece), and misaligned differently (bytes throughout).  The result is the aligned one's; the 64 guard bytes before and
    after the destination keep their fill."""
    n, h, w, _ = case.imgs.shape
    nbytes = case.imgs.size
    sbuf = torch.zeros(nbytes + 32, dtype=torch.uint8, device=dev)
    x = sbuf[src_off:src_off + nbytes].view(n, h, w, 3)
    x.copy_(torch.from_numpy(case.imgs).to(dev))
    dbuf = torch.full((nbytes + 192,), 0xa5, dtype=torch.uint8, device=dev)
    out = dbuf[dst_off:dst_off + nbytes].view(n, h, w, 3)
    assert x.data_ptr() % 16 == src_off % 16 and out.data_ptr() % 16 == dst_off % 16
    _run(case, x, method, 'keep', out=out)
    want = _as4(_run(case, _batch(case, dev), method, 'keep'))
    assert torch.equal(out, want)
    d = dbuf.cpu().numpy()
    assert (d[:dst_off] == 0xa5).all() and (d[dst_off + nbytes:] == 0xa5).all()


# ------------------------------------------------------------------------------------------------------------- fitted parameters
def _angle(a, b):
    return math.atan2(float(np.linalg.norm(np.cross(a, b))), float(a @ b))


def test_fit_end_to_end(case, dev):
    """fit_macenko / fit_reinhard on the device against the oracle's fit of the same image: HE columns within one angle bin, maxC within
    one concentration bin, the Reinhard mean and standard deviation within 1e-6 relative; an image the oracle refuses is flagged, and the
    other images of its batch get what they get alone."""
    x = _batch(case, dev)
    single = x.dim() == 3
    for name, fit, ofit in (('macenko', stain.fit_macenko, SO.fit_macenko), ('reinhard', stain.fit_reinhard, SO.fit_reinhard)):
        want = []
        for im in case.imgs:
            try:
                want.append(ofit(im))
            except ValueError:
                want.append(None)
        if single and want[0] is None:
            with pytest.raises(ValueError):
                fit(x)
            continue
        got = [fit(x)] if single else fit(x)
        assert len(got) == len(want)
        for i, (g, wnt) in enumerate(zip(got, want)):
            assert g.n == case.n[i]
            if wnt is None:
                assert g.error and g[0] is None
                continue
            assert g.error is None
            if name == 'macenko':
                da = [_angle(g.he[:, k], wnt[0][:, k]) for k in range(2)]
                dc = np.abs(g.max_c - wnt[1])
                print('image %d: HE columns %.2e, %.2e rad from the oracle (bin %.2e), maxC off by %.2e, %.2e (bin %.2e)' % (i, da[0], da[1], ANGLE_BIN, dc[0], dc[1], CONC_BIN))
                assert max(da) <= ANGLE_BIN * (1 + 1e-9) and (dc <= CONC_BIN * (1 + 1e-9)).all()      # (the slack: rounding of the comparison itself)
            else:
                rel = max(float(np.abs(g.mean / wnt[0] - 1).max()), float(np.abs(g.std / wnt[1] - 1).max()))
                print('image %d: Reinhard mean / std within %.2e relative' % (i, rel))
                assert rel <= 1e-6
            if not single:                                       # the neighbours of the white image: what the image gets alone, bit for bit
                alone = fit(x[i].contiguous())
                assert all(np.array_equal(a, b) for a, b in zip(alone[:2], g[:2])) and alone.n == g.n
    if not single:
        assert case.n[1] == 0 and stain.fit_macenko(x)[1].error and stain.fit_reinhard(x)[1].error
        same = stain.normalize_macenko(x)                        # fitted on itself: the flagged image is served as it is
        assert torch.equal(same[1], x[1])


# -------------------------------------------------------------------------------------------------------------------- integration
def _slide(seed, size=512):
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    l0 = SO.shifted_he(seed, 1, size)[0]
    s = ArraySlide([l0, l0[::4, ::4], l0[::16, ::16]], [1.0, 4.0, 16.0])
    s.name = 'stain.svs'
    return l0, s


def _args(monkeypatch, tmp_path):
    import myargs
    for k, v in (('scan_level', 0), ('scan_resize', 1), ('num_classes', 4), ('class_probs', [0., 0., 0., 0.]), ('tile_w', 64), ('tile_h', 64),
                 ('tile_stride_w', 64), ('tile_stride_h', 64), ('val_save_pth', str(tmp_path / 'out')), ('wsi_mask_pth', str(tmp_path / 'nomask'))):
        monkeypatch.setattr(myargs.args, k, v)


def test_dataset_wsis_serves_the_normalised_level(dev, tmp_path, monkeypatch):
    import utils.dataset as ds
    _args(monkeypatch, tmp_path)
    l0, slide = _slide(21)
    norm = stain.Normalizer('macenko')
    dataset = ds.Dataset_wsis({'stain.svs': slide}, {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}, bs=8, stain=norm)
    scan = dataset.wsis['stain.svs']['scan']
    assert isinstance(scan, stain.StainedSlide) and scan.scan is slide
    params = stain.fit_macenko(slide.device_level(2, dev))       # the fit level: min(2, level_count - 1)
    for level in (0, 1):
        want = stain.normalize_macenko(slide.device_level(level, dev), params)
        got = scan.device_level(level, dev)
        assert torch.equal(got, want) and not torch.equal(got, slide.device_level(level, dev))
        assert scan.device_level(level, dev) is got
    assert scan.stain_error is None and np.array_equal(scan.stain_params.he, params.he)
    assert np.array_equal(slide.device_level(0, dev).cpu().numpy(), l0)                          # the scan's own level stays raw
    # a slide without tissue: served as it is, the reason recorded
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    white = stain.StainedSlide(ArraySlide([np.full((64, 64, 3), 255, np.uint8)]), norm)
    assert torch.equal(white.device_level(0, dev), torch.full((64, 64, 3), 255, dtype=torch.uint8, device=dev)) and 'tissue' in white.stain_error


def test_predict_tumorbed_cls_on_a_stained_slide(dev, tmp_path, monkeypatch):
    """predict_tumorbed(mode='cls') through the hook equals, bit for bit, the run on a slide whose level 0 holds the pre-normalised bytes
    (the thumbnail levels, which read_region serves to the nuclei mask, stay raw in both); stain=None equals no keyword at all."""
    import resnets_shift
    import utils.dataset as ds
    import utils.eval as val
    from models.models import Classifier
    from wsi_segmentation_pipeline_amd import synthetic as W
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    _args(monkeypatch, tmp_path)
    l0, slide = _slide(22)
    net = resnets_shift.resnet18(False)
    net.load_state_dict(W.make_resnet18_state_dict(11, with_fc=False), strict=False)
    head = Classifier(512, 4)
    head.load_state_dict(W.make_head_state_dict(22, 'classifier'))
    model = val.SlideClassifierModel(net, head).to(dev)
    params = {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}

    def run(scan, **kw):
        dataset = ds.Dataset_wsis({'stain.svs': scan}, params, bs=16, **kw)
        assert len(dataset.wsis['stain.svs']['iterator'].dataset) > 4
        res = val.predict_tumorbed(model, dataset, 1, mode='cls', save=False)['stain.svs']
        return res['logits'].cpu().numpy(), np.asarray(res['heatmap']), np.asarray(res['classes'])
    norm = stain.Normalizer('macenko')
    stained = run(slide, stain=norm)
    pre0 = stain.normalize_macenko(slide.device_level(0, dev), stain.fit_macenko(slide.device_level(2, dev))).cpu().numpy()
    assert (pre0 != l0).any()
    pre = ArraySlide([pre0, l0[::4, ::4], l0[::16, ::16]], [1.0, 4.0, 16.0])
    pre.name = 'stain.svs'
    want = run(pre)
    for a, b in zip(stained, want):
        assert a.shape == b.shape and np.array_equal(a, b)
    raw, none = run(slide), run(slide, stain=None)
    for a, b in zip(raw, none):
        assert np.array_equal(a, b)
    assert not np.array_equal(raw[0], stained[0])               # and the normalisation does reach the model


def test_predict_breastpathq_with_stain(dev, tmp_path, monkeypatch):
    """predict_breastpathq(stain=...) on four small regions equals scoring the regions normalised one by one beforehand."""
    import resnets_shift
    from PIL import Image
    from models import models as M
    from myargs import args
    from utils import eval as val
    from wsi_segmentation_pipeline_amd import synthetic as W
    monkeypatch.setattr(args, 'tile_w', 64)
    monkeypatch.setattr(args, 'tile_h', 64)
    net = resnets_shift.resnet18(False, precision='parity')
    net.load_state_dict(W.make_resnet18_state_dict(11, with_fc=False), strict=False)
    reg, cls = M.Regressor(512, 1), M.Classifier(512, 4)
    reg.load_state_dict(W.make_head_state_dict(23, 'regressor', num_classes=1))
    cls.load_state_dict(W.make_head_state_dict(22, 'classifier'))
    model = val.SlideClassifierModel(net, cls, reg).to(dev)
    patches = SO.shifted_he(31, 4, 64)
    patches[2] = 255                                            # a region without tissue is scored as it is
    # the seeded regressor's outputs lie far outside [0, 1], where the clamp would hide every difference: rescale its last layer so that
    # the raw regions score 0.5 +- 0.2
    xy = torch.zeros((4, 2), dtype=torch.int32, device=dev)
    xy[:, 1] = torch.arange(4, dtype=torch.int32, device=dev) * 64
    with torch.no_grad():
        r = model.regress_views(slide_u8=torch.from_numpy(patches.reshape(256, 64, 3)).to(dev), tile_xy=xy, ph=64, pw=64).reshape(-1)
        mid, half = float((r.max() + r.min()) / 2), float((r.max() - r.min()) / 2)
        assert half > 0
        last = model.regressor.fc[2]
        last.weight.mul_(0.2 / half)
        last.bias.copy_((last.bias - mid) * (0.2 / half) + 0.5)
    order = [(3, 1), (1, 2), (7, 1), (2, 5)]
    norm = stain.Normalizer('macenko')
    raw_dir, pre_dir = tmp_path / 'raw', tmp_path / 'pre'
    for d in (raw_dir, pre_dir):
        d.mkdir()
    for (a, b), p in zip(order, patches):
        Image.fromarray(p).save(str(raw_dir / ('%d_%d.tif' % (a, b))))
        q = p if (p == 255).all() else stain.normalize_macenko(torch.from_numpy(p).to(dev)).cpu().numpy()
        Image.fromarray(q).save(str(pre_dir / ('%d_%d.tif' % (a, b))))
    labels = tmp_path / 'labels.csv'
    labels.write_text('slide,rid,y\n' + ''.join('%d,%d,0.1\n' % ab for ab in order))
    got = val.predict_breastpathq(model, 1, str(raw_dir), str(labels), out_csv=str(tmp_path / 'a.csv'), batch=3, stain=norm)
    want = val.predict_breastpathq(model, 1, str(pre_dir), str(labels), out_csv=str(tmp_path / 'b.csv'), batch=3)
    plain = val.predict_breastpathq(model, 1, str(raw_dir), str(labels), out_csv=str(tmp_path / 'c.csv'), batch=3, stain=None)
    assert [(a, b) for a, b, _ in got] == order and got == want
    p_plain, p_got = np.array([v for _, _, v in plain]), np.array([v for _, _, v in got])
    print('scores raw', p_plain, 'normalised', p_got)
    assert (p_plain > 0.25).all() and (p_plain < 0.75).all() and (p_got > 0).all() and (p_got < 1).all()
    assert p_plain[2] == p_got[2] and (np.delete(p_plain, 2) != np.delete(p_got, 2)).all()
