"""GPU tests of the stain normalisation (csrc/stain.hip, wsi_segmentation_pipeline_amd/stain.py) against the float64 spec
(tests/stain_oracle.py): the fit kernels' moments and histograms, the two applies byte for byte, the fitted parameters end to end, and
the hooks of utils.dataset / utils.eval.

The kernels walk an image in pieces of 16 pixels.  A workgroup owns a chunk of 2 048 pieces = 32 768 pixels and takes it in eight steps
of 256 pieces = 4 096 pixels, thread t piece chunk * 2048 + step * 256 + t; up to 15 head pixels in front of the first 16-byte aligned
piece go to thread 0 of chunk 0.  Shapes (h x w):
  1 x 1 (one pixel), 1 x 17 (just past one piece), 7 x 9 (189 bytes), 64 x 64 (4 096 pixels: exactly one step of one chunk),
  65 x 63 (4 095: one step, ragged), 65 x 64 (4 160: step 1 begins, pieces 256..259),
  181 x 181 (32 761, 7 short of a chunk: all eight steps, a ragged last piece),
  182 x 181 (32 942, 174 into chunk 1: a second, mostly idle workgroup, two partials to merge, histogram atomics from two workgroups),
  256 x 257 (65 792: three chunks, the last one 16 whole pieces),
each as one image and as a batch of three whose image starts are misaligned (3 x 182 x 181 bytes is 10 mod 16) and whose middle image
is all white; and 2897 x 2897 (8 392 609 pixels = 257 chunks: thread 0 of the merge adds chunks 0 and 256) for the fit kernels alone.
The oracle's results are computed once per case."""
import math

import numpy as np
import pytest
import torch

import stain_oracle as SO
from wsi_segmentation_pipeline_amd import stain

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 17), (7, 9), (64, 64), (65, 63), (65, 64), (181, 181), (182, 181), (256, 257)]
PARENT = 128                                                   # the side of the images the cases are cut from
STEP_PIXELS = 256 * 16                                         # one step of a workgroup: 256 threads x one piece of 16 pixels
CASES = [(h, w, n) for h, w in SHAPES for n in (1, 3)]
ANGLE_BIN = 2 * math.pi / stain.ANGLE_BINS
CONC_BIN = stain.CONC_MAX / stain.CONC_BINS


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


class Case:
    """n images of h x w cut from 128 x 128 parents at a tissue pixel (image 1 of a batch: all white), with the oracle's fit of every
    parent: parameters that are valid whatever the crop holds.  A shape past one step (4 096 pixels) is the corner of the parent repeated
    periodically: most such shapes fit no parent, the family itself is almost all background at a large size (0.08 % tissue at 2897
    against 31 % at 128), and the crop at a tissue pixel leaves the last step of 65 x 64 bare in one image.  From one step on, every
    step of every image but the white one, the last partial step too, holds tissue (steps as they fall in a batch whose first byte is
    16-byte aligned): a step that is skipped or read twice changes the count."""

    def __init__(self, h, w, n, seed=None):
        parents = SO.shifted_he(40 + h + w if seed is None else seed, n, PARENT)
        self.imgs, self.fits = np.empty((n, h, w, 3), np.uint8), []
        for i, p in enumerate(parents):
            if h * w <= STEP_PIXELS:
                ys, xs = np.nonzero(SO.tissue(p))
                k = int(np.argmin((ys - 64) ** 2 + (xs - 64) ** 2))
                y0, x0 = min(int(ys[k]), PARENT - h), min(int(xs[k]), PARENT - w)
                self.imgs[i] = p[y0:y0 + h, x0:x0 + w]
            else:
                self.imgs[i] = np.tile(p, (-(-h // PARENT), -(-w // PARENT), 1))[:h, :w]
            self.fits.append({'plane': SO.macenko_plane(p), 'macenko': SO.fit_macenko(p), 'reinhard': SO.fit_reinhard(p)})
        if n == 3:
            self.imgs[1] = 255
        self.target = SO.fit_reinhard(SO.shifted_he(7, 1, PARENT, (1.0, 1.0, 1.0))[0])
        self.n = [int(SO.tissue(im).sum()) for im in self.imgs]
        self.step_tissue = [step_tissue(im, i * h * w * 3) for i, im in enumerate(self.imgs) if not (n == 3 and i == 1)]
        for full, last in self.step_tissue:
            assert all(c > 0 for c in full) and (last is None or last > 0), (h, w, n)

    def macenko_params(self):
        return [stain.MacenkoParams(f['macenko'][0], f['macenko'][1], f['macenko'][2]) for f in self.fits]

    def reinhard_params(self):
        return [stain.ReinhardParams(f['reinhard'][0], f['reinhard'][1], f['reinhard'][2]) for f in self.fits]


def head_pixels(byte_offset):
    """the pixels in front of the first 16-byte aligned piece of an image that starts byte_offset bytes past a 16-byte boundary: the h
    of 0..15 with (byte_offset + 3 h) % 16 == 0"""
    return next(h for h in range(16) if (byte_offset + 3 * h) % 16 == 0)


def step_tissue(img, byte_offset):
    """([tissue pixels of every full step], tissue pixels of the last, partial step or None) of an image of one step or more that starts
    byte_offset bytes past a 16-byte boundary (in a batch whose first byte is aligned, as a tensor of its own is): step k covers pixels
    [head + 4096 k, head + 4096 (k + 1))"""
    t = SO.tissue(img).reshape(-1)[head_pixels(byte_offset):]
    full = [int(t[k * STEP_PIXELS:(k + 1) * STEP_PIXELS].sum()) for k in range(t.size // STEP_PIXELS)]
    return full, (int(t[len(full) * STEP_PIXELS:].sum()) if full and t.size % STEP_PIXELS else None)


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
def _check_moments(case, lab, got):
    for i, im in enumerate(case.imgs):
        px = im[SO.tissue(im)]
        v = SO.lab_of(px) if lab else SO.od_of(px)
        want = SO.moments_vector(*SO.moments_pairwise(v))
        scale = SO.moments_vector(*SO.moments_pairwise(np.abs(v)))
        err = np.abs(got[i] - want)
        print('%s image %d: n %d, worst moment error / scale %.2e' % ('lab' if lab else 'od', i, v.shape[0], float((err / np.maximum(scale, 1e-300)).max())))
        assert got[i, 0] == case.n[i] and (err <= 1e-12 * scale).all()
        if not lab:
            assert (err <= 1e-12 * np.abs(want)).all()


def test_moments(case, dev):
    """Both sides are float64 sums of the same values (od: the fp32 table; l-alpha-beta: float64 logarithms equal to a few units of 1e-16),
    so only the order of the sums differs, and the bound is 1e-12 of the sum of the magnitudes (for the optical densities, which are all
    positive, that is 1e-12 relative).  Where it comes from: on the device an addend passes through at most about 165 float64 additions
    at the sizes tested - 8 x 16 + 15 in its thread (eight pieces and the head), 6 shuffles and 3 wave adds in the workgroup, then
    2 + 6 + 3 in the merge of up to 512 chunks - so the sum is within 165 x 2^-53 = 1.8e-14 of the scale, plus one rounding
    per product and the few units of 2^-53 by which the two log10 differ; the oracle's pairwise sums (SO.moments_pairwise) add about
    32 x 2^-53 = 3.6e-15.  1e-12 leaves a factor of about 50.  The count is exact, two runs give the same bits, a white image gives zeros."""
    x = _as4(_batch(case, dev))
    for lab in (False, True):
        got = stain._moments(x, lab, stain.IO, stain.BETA)
        again = stain._moments(x, lab, stain.IO, stain.BETA)
        assert got.shape == (x.shape[0], 10) and np.array_equal(got.view(np.uint64), again.view(np.uint64))
        _check_moments(case, lab, got)
    if x.shape[0] == 3:
        assert case.n[1] == 0 and not got[1].any()


# ---------------------------------------------------------------------------------------------- the fit kernels past 256 chunks
@pytest.fixture(scope='module')
def big(dev):
    """2897 x 2897 = 8 392 609 pixels = 257 chunks, the smallest square at which thread 0 of moments_merge_kernel adds two partials
    (chunks 0 and 256); one image, resident once for the three tests"""
    case = Case(2897, 2897, 1, seed=77)                          # a parent with tissue in every pair of rows: 341 pixels a step at least
    assert -(-(2897 * 2897) // (8 * STEP_PIXELS)) == 257 and min(case.step_tissue[0][0]) > 0
    return case, torch.from_numpy(case.imgs).to(dev)


@pytest.mark.parametrize('lab', [False, True], ids=['od', 'lab'])
def test_moments_257_chunks(big, lab):
    """the bound of test_moments, unchanged: the merge's strided loop adds one addition per addend, and the oracle sums pairwise"""
    case, x = big
    got = stain._moments(x, lab, stain.IO, stain.BETA)
    assert np.array_equal(got.view(np.uint64), stain._moments(x, lab, stain.IO, stain.BETA).view(np.uint64))
    _check_moments(case, lab, got)


def test_histograms_257_chunks(big):
    """global 64-bit atomics from 257 workgroups into one image's bins"""
    case, x = big
    im, f = case.imgs[0], case.fits[0]
    ah = stain._hist(x, False, f['plane'].reshape(1, 6), stain.IO, stain.BETA)
    ch = stain._hist(x, True, np.linalg.pinv(f['macenko'][0]).reshape(1, 6), stain.IO, stain.BETA)
    _check_hist(ah[0], SO.angle_hist(im, f['plane']), case.n[0], 'angle')
    ref = SO.conc_hist(im, f['macenko'][0])
    for r in range(2):
        _check_hist(ch[0, r], ref[r], case.n[0], 'concentration %d' % r)


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
    out of place.  The model - apply_kernel's fma order in float32, np.exp2 / np.log2 in float32 - on the shapes past one step, against
    the same oracle: 0 bytes at 65 x 64 and 182 x 181; at 181 x 181 Macenko 0 (n = 1) and 1.0e-5 (n = 3), Reinhard 4.1e-5 and 2.0e-5; at
    256 x 257 Macenko 0, Reinhard 2.0e-5 and 1.4e-5 ('all'; 'keep': 0); never more than 1 off.  The condition leaves a factor of 25."""
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
