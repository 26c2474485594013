"""CPU-side checks of the stain normalisation: the C ABI (header, native.SIGNATURES, the built library, -22 before any device work),
the host functions of wsi_segmentation_pipeline_amd.stain, the spec itself (tests/stain_oracle.py) on images of known stains, and the
two hooks with nothing to normalise."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import stain_oracle as SO
from wsi_segmentation_pipeline_amd import native, stain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('wsi_stain_moments_scratch_bytes', 'wsi_stain_od_moments', 'wsi_stain_lab_moments', 'wsi_stain_angle_hist', 'wsi_stain_conc_hist',
           'wsi_stain_macenko_apply', 'wsi_stain_reinhard_apply')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


def test_entries_in_header_signatures_and_library(lib):
    hdr = open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read()
    block = hdr[hdr.index('stain normalisation'):]
    assert 'Macenko' in block and 'Reinhard' in block and 'no counterpart' in block
    declared = set(re.findall(r'\b(wsi_stain_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)))
    assert declared == set(ENTRIES) == {k for k in native.SIGNATURES if k.startswith('wsi_stain_')}
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert native.SIGNATURES[name][1][-1] is C.c_void_p or name.endswith('_bytes')           # void* stream last
    assert native.ABI_VERSION == 9 == lib.wsi_hip_abi_version()                                  # additive entries


def test_entries_refuse_bad_arguments_before_any_device_work(lib):
    """The idiom of tests/test_unet_bottleneck_cpu.py: every pointer is the fake address 4096 and every call carries exactly one defect, so
    a call that got past validation would fault on its first launch."""
    fake = C.c_void_p(4096)
    good = dict(img=fake, npix=100, n=2, v_max=205, lut=fake, out=fake, scratch=fake, prm=fake, bins=4096, cmax=8.0, dst=fake, vm=fake, io=240.0)

    def run(name, **bad):
        a = dict(good, **bad)
        f = getattr(lib, name)
        return {
            'wsi_stain_od_moments': lambda: f(a['img'], a['npix'], a['n'], a['v_max'], a['lut'], a['out'], a['scratch'], None),
            'wsi_stain_lab_moments': lambda: f(a['img'], a['npix'], a['n'], a['v_max'], a['out'], a['scratch'], None),
            'wsi_stain_angle_hist': lambda: f(a['img'], a['npix'], a['n'], a['v_max'], a['lut'], a['prm'], a['bins'], a['out'], None),
            'wsi_stain_conc_hist': lambda: f(a['img'], a['npix'], a['n'], a['v_max'], a['lut'], a['prm'], a['bins'], a['cmax'], a['out'], None),
            'wsi_stain_macenko_apply': lambda: f(a['img'], a['dst'], a['npix'], a['n'], a['vm'], a['lut'], a['prm'], a['io'], None),
            'wsi_stain_reinhard_apply': lambda: f(a['img'], a['dst'], a['npix'], a['n'], a['vm'], a['prm'], None),
        }[name]()
    shape = [dict(npix=0), dict(npix=-5), dict(npix=(1 << 40) + 1), dict(n=0), dict(n=-1), dict(n=65536)]
    vmax = [dict(v_max=-1), dict(v_max=256)]
    defects = {
        'wsi_stain_od_moments': [dict(img=None), dict(lut=None), dict(out=None), dict(scratch=None)] + shape + vmax,
        'wsi_stain_lab_moments': [dict(img=None), dict(out=None), dict(scratch=None)] + shape + vmax,
        'wsi_stain_angle_hist': [dict(img=None), dict(lut=None), dict(prm=None), dict(out=None), dict(bins=0), dict(bins=4097)] + shape + vmax,
        'wsi_stain_conc_hist': [dict(img=None), dict(lut=None), dict(prm=None), dict(out=None), dict(bins=0), dict(bins=4097), dict(cmax=0.0),
                                dict(cmax=-1.0), dict(cmax=float('nan'))] + shape + vmax,
        'wsi_stain_macenko_apply': [dict(img=None), dict(dst=None), dict(vm=None), dict(lut=None), dict(prm=None), dict(io=0.0),
                                    dict(io=float('nan')), dict(dst=C.c_void_p(4096 + 300))] + shape,
        'wsi_stain_reinhard_apply': [dict(img=None), dict(dst=None), dict(vm=None), dict(prm=None), dict(dst=C.c_void_p(4096 - 1))] + shape,
    }
    assert set(defects) == set(ENTRIES) - {'wsi_stain_moments_scratch_bytes'}
    for name, cases in defects.items():
        for bad in cases:
            assert run(name, **bad) == -22, (name, bad)
    # the scratch size: ten doubles per chunk of 32768 pixels and image, 0 for a bad shape
    f = lib.wsi_stain_moments_scratch_bytes
    assert f(1, 1) == 80 and f(32768, 3) == 240 and f(32769, 1) == 160 and f(40000 * 40000, 1) == 80 * ((40000 * 40000 + 32767) // 32768)
    assert f(0, 1) == 0 and f(10, 0) == 0 and f((1 << 40) + 1, 1) == 0 and f(10, 65536) == 0


def test_percentile_from_hist():
    p = stain.percentile_from_hist
    # hand-built: 4 bins over [0, 4); rank = max(1, ceil(p / 100 * n))
    assert p([0, 5, 0, 95], 99, 0.0, 4.0) == 3.5                # rank 99 of 100: the last bin
    assert p([0, 5, 0, 95], 5, 0.0, 4.0) == 1.5                 # rank 5: still the second bin
    assert p([0, 5, 0, 95], 6, 0.0, 4.0) == 3.5                 # rank 6 (exact arithmetic: 6 / 100 * 100 is 6, not 6.000000000000001)
    assert p([0, 5, 0, 95], 0, 0.0, 4.0) == 1.5                 # rank 1 = the smallest value
    assert p([0, 0, 7, 0], 1, 0.0, 4.0) == p([0, 0, 7, 0], 50, 0.0, 4.0) == p([0, 0, 7, 0], 100, 0.0, 4.0) == 2.5     # all in one bin
    assert p([1, 0, 0, 0], 99, -2.0, 2.0) == -1.5               # one value
    assert p([3, 0, 0, 1], 75, 0.0, 4.0) == 0.5 and p([3, 0, 0, 1], 76, 0.0, 4.0) == 3.5
    assert p([1] * 100, 99, 0.0, 100.0) == 98.5                 # 99 / 100 * 100 = 99.00000000000001 in floating point
    with pytest.raises(ValueError):
        p([0, 0, 0], 50, 0.0, 1.0)
    # seeded data: within one bin width of np.percentile
    rng = np.random.default_rng(5)
    for n, bins in ((1000, 4096), (37, 64), (100000, 4096)):
        x = rng.gamma(2.0, 0.6, n).clip(0, 7.999)
        h = np.bincount(np.floor(x / 8.0 * bins).astype(int), minlength=bins)
        for q in (1, 50, 99):
            assert abs(p(h, q, 0.0, 8.0) - np.percentile(x, q, method='inverted_cdf')) <= 8.0 / bins, (n, bins, q)


def test_v_max_rule_is_the_float_test():
    od = stain.od_table()
    assert od.dtype == np.float32 and np.array_equal(od, SO.OD) and np.all(np.diff(od) < 0)
    v_max = stain.tissue_v_max()
    assert v_max == SO.V_MAX == 205
    assert np.array_equal(od >= np.float32(stain.BETA), np.arange(256) <= v_max)
    assert np.array_equal(od.astype(np.float64) >= stain.BETA, np.arange(256) <= v_max)


def _known_stain_image(rng, he, n=200000):
    """u8 pixels of known stains, od = HE . c through rgb = Io exp(-od) - 1: 2 % pure haematoxylin, 2 % pure eosin, the rest mixtures with
    both concentrations > 0, which lie strictly between the two in angle.  All are tissue, so the 1st and 99th percentile of the angle are
    the medians of the two pure clusters, where the rounding of the pixels to bytes averages out."""
    k = n // 50
    c = np.stack((rng.uniform(0.6, 1.6, n), rng.uniform(0.6, 1.6, n)))
    c[0, :k], c[1, :k] = rng.uniform(1.0, 2.2, k), 0.0
    c[0, k:2 * k], c[1, k:2 * k] = 0.0, rng.uniform(1.0, 2.2, k)
    return np.clip(np.rint(stain.IO * np.exp(-(he @ c).T) - 1.0), 0, 255).astype(np.uint8).reshape(-1, 100, 3)


def test_oracle_recovers_known_stains():
    rng = np.random.default_rng(12)
    he = stain.MACENKO_REF.he / np.linalg.norm(stain.MACENKO_REF.he, axis=0)
    img = _known_stain_image(rng, he)
    got, max_c, n = SO.fit_macenko(img)
    assert n == img.shape[0] * img.shape[1]
    for k in range(2):
        angle = math.acos(min(1.0, float(got[:, k] @ he[:, k]) / float(np.linalg.norm(got[:, k]))))
        print('stain %d: %.2e rad from the truth, one bin = %.2e' % (k, angle, 2 * math.pi / stain.ANGLE_BINS))
        assert angle <= 2 * math.pi / stain.ANGLE_BINS
    assert got[0, 0] > got[0, 1] and np.all(np.abs(max_c - 1.6) < 0.03)          # the 99th percentile of uniform(0.6, 1.6) next to 2 % above it
    # a real-looking image with background: kept bytes, changed tissue, and a Reinhard target equal to the source changes next to nothing
    img = SO.shifted_he(3, 1, 128)[0]
    he2, mc2, _ = SO.fit_macenko(img)
    out = SO.apply_macenko(img, SO.macenko_matrix(he2, mc2))
    keep = ~SO.tissue(img)
    assert np.array_equal(out[keep], img[keep]) and (out[~keep] != img[~keep]).any()
    mean, std, _ = SO.fit_reinhard(img)
    same = SO.apply_reinhard(img, (mean, std), (mean, std))     # the paper's two matrices invert each other to four digits: a level at most
    assert np.abs(same.astype(int) - img.astype(int)).max() <= 1 and (same == img).mean() > 0.7
    for bad in (np.full((4, 4, 3), 255, np.uint8), np.full((4, 4, 3), 100, np.uint8)):
        with pytest.raises(ValueError):
            SO.fit_macenko(bad)
        with pytest.raises(ValueError):
            SO.fit_reinhard(bad)


def test_host_functions_match_the_spec():
    """stain.py's host steps against the oracle's, on the oracle's own moments and histograms (no device involved)."""
    img = SO.shifted_he(3, 1, 128)[0]
    n, s, ss = SO.od_moments(img)
    v = stain.macenko_plane(SO.moments_vector(n, s, ss))
    assert np.array_equal(v, SO.macenko_plane(img))
    he = stain.macenko_vectors(SO.angle_hist(img, v), v)
    assert np.array_equal(he, SO.stain_vectors(SO.angle_hist(img, v), v))
    he_o, mc_o, _ = SO.fit_macenko(img)
    p = stain.MacenkoParams(he_o, mc_o, n)
    assert np.allclose(stain.macenko_matrix(p), SO.macenko_matrix(he_o, mc_o), rtol=1e-13, atol=0)
    # the folded Reinhard map equals the three steps of the spec
    mean, std, _ = SO.fit_reinhard(img)
    tgt = (mean + np.array([0.1, -0.02, 0.01]), std * np.array([1.2, 0.8, 1.1]))
    g3, g = stain.reinhard_affine(stain.ReinhardParams(mean, std, n), stain.ReinhardParams(tgt[0], tgt[1], n))
    x = SO.lab_of(img)
    want = ((x - mean) * (tgt[1] / std) + tgt[0]) @ SO.LAB2LMS.T
    got = np.log10((img.reshape(-1, 3) + 1.0) / 256.0 @ SO.RGB2LMS.T) @ g3.T + g
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(stain.RGB2LMS, SO.RGB2LMS) and np.array_equal(stain.LMS2RGB, SO.LMS2RGB)
    assert np.allclose(stain.LMS2LAB, SO.LMS2LAB, rtol=1e-15) and np.allclose(stain.LAB2LMS, SO.LAB2LMS, rtol=1e-15)
    with pytest.raises(ValueError):
        stain.macenko_plane(SO.moments_vector(1, s, ss))
    with pytest.raises(ValueError):
        stain.macenko_plane(SO.moments_vector(3, np.array([3., 3., 3.]), np.full((3, 3), 3.0)))  # three identical pixels


def test_cpu_tensors_and_bad_arguments_are_refused():
    img = torch.zeros((4, 4, 3), dtype=torch.uint8)
    tgt = stain.ReinhardParams(np.zeros(3), np.ones(3), 10)
    for call in (lambda: stain.fit_macenko(img), lambda: stain.fit_reinhard(img), lambda: stain.normalize_macenko(img),
                 lambda: stain.normalize_reinhard(img, tgt), lambda: stain.Normalizer('macenko').apply(img)):
        with pytest.raises(RuntimeError, match='GPU'):
            call()
    with pytest.raises(ValueError):
        stain.Normalizer('vahadane')
    with pytest.raises(ValueError):
        stain.Normalizer('reinhard')                            # no built-in target


class _StubNormalizer:
    fit_level = None

    def __init__(self, fail=False):
        self.fits, self.applies, self.fail = [], [], fail

    def fit(self, img):
        self.fits.append(tuple(img.shape))
        if self.fail:
            raise ValueError('no tissue')
        return 'params'

    def apply(self, img, params=None, out=None):
        self.applies.append((tuple(img.shape), params))
        return 255 - img


def test_stained_slide_delegates_and_caches():
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    rng = np.random.default_rng(2)
    l0 = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    scan = ArraySlide([l0, l0[::4, ::4], l0[::16, ::16]], [1.0, 4.0, 16.0])
    scan.name = 'a.svs'
    norm = _StubNormalizer()
    s = stain.StainedSlide(scan, norm)
    assert s.level_dimensions == scan.level_dimensions and s.level_downsamples == scan.level_downsamples
    assert s.level_count == 3 and s.dimensions == scan.dimensions and s.name == 'a.svs'
    assert np.array_equal(np.asarray(s.read_region((8, 4), 0, (16, 8))), np.asarray(scan.read_region((8, 4), 0, (16, 8))))       # raw
    a = s.device_level(0, 'cpu')
    assert np.array_equal(a.numpy(), 255 - l0) and norm.fits == [(4, 6, 3)] and norm.applies == [((64, 96, 3), 'params')]
    assert s.device_level(0, 'cpu') is a and len(norm.applies) == 1                              # cached per (level, device)
    b = s.device_level(1, 'cpu')
    assert np.array_equal(b.numpy(), 255 - l0[::4, ::4]) and len(norm.fits) == 1 and len(norm.applies) == 2                      # fitted once
    assert np.array_equal(scan.device_level(0, 'cpu').numpy(), l0) and s.stain_error is None     # the scan's own level is untouched
    s.close()
    assert s._dev == {} and scan._dev == {} and np.array_equal(s.device_level(0, 'cpu').numpy(), 255 - l0) and len(norm.fits) == 1
    # an explicit fit level; a slide of one level fits on level 0
    norm = _StubNormalizer()
    norm.fit_level = 1
    stain.StainedSlide(scan, norm).device_level(0, 'cpu')
    assert norm.fits == [(16, 24, 3)]
    norm = _StubNormalizer()
    stain.StainedSlide(ArraySlide([l0]), norm).device_level(0, 'cpu')
    assert norm.fits == [(64, 96, 3)]
    # a failed fit: served raw, the reason recorded, not fitted again
    norm = _StubNormalizer(fail=True)
    s = stain.StainedSlide(scan, norm)
    assert np.array_equal(s.device_level(0, 'cpu').numpy(), l0) and s.stain_error == 'no tissue'
    s.device_level(1, 'cpu')
    assert len(norm.fits) == 1 and norm.applies == []


def test_dataset_wsis_without_stain_builds_what_it_built(tmp_path, monkeypatch):
    import myargs
    import utils.dataset as ds
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    a = myargs.args
    for k, v in (('scan_level', 0), ('scan_resize', 1), ('tile_w', 64), ('tile_h', 64), ('wsi_mask_pth', str(tmp_path / 'nomask'))):
        monkeypatch.setattr(a, k, v)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)          # the host tile grid: this test runs without a GPU
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)            # (the iterator only names its device)
    l0 = SO.shifted_he(4, 1, 256)[0]
    scan = ArraySlide([l0, l0[::4, ::4], l0[::16, ::16]], [1.0, 4.0, 16.0])
    params = {'ph': 64, 'pw': 64, 'sh': 48, 'sw': 48}
    before = ds.Dataset_wsis({'s.svs': scan}, params, bs=4)
    after = ds.Dataset_wsis({'s.svs': scan}, params, bs=4, stain=None)
    norm = _StubNormalizer()
    wrapped = ds.Dataset_wsis({'s.svs': scan}, params, bs=4, stain=norm)
    for d in (before, after, wrapped):
        assert list(d.wsis) == ['s.svs'] and len(d.wsis['s.svs']['iterator'].dataset) > 0
    w0, w1, w2 = before.wsis['s.svs'], after.wsis['s.svs'], wrapped.wsis['s.svs']
    assert w0['scan'] is scan and w1['scan'] is scan and set(w0) == set(w1) == set(w2)
    assert w0['iterator'].dataset.datalist == w1['iterator'].dataset.datalist == w2['iterator'].dataset.datalist      # the mask is raw
    assert np.array_equal(w0['mask'], w1['mask']) and np.array_equal(w0['mask'], w2['mask'])
    assert w0['iterator'].batch_size == w1['iterator'].batch_size == 4 and w0['maskpath'] == w1['maskpath']
    assert isinstance(w2['scan'], stain.StainedSlide) and w2['scan'].scan is scan and w2['scan'].normalizer is norm
    assert norm.fits == [] and norm.applies == []               # nothing is normalised before a level is asked for


# ------------------------------------------------------------------------------------- the inputs of tests/test_gpu_stain.py
def test_gpu_case_inputs_and_pairwise_moments():
    """What the GPU tests' fixture decides on its own: the head of an image by its address (the kernel's closed form), the tissue count
    of every step, the two constructions (a crop of the parent up to one step, the parent repeated periodically beyond), the condition
    that every step of every case holds tissue, and the pairwise moments against exactly rounded sums."""
    import test_gpu_stain as G
    for a in range(64):
        h = G.head_pixels(a)
        assert 0 <= h < 16 and (a + 3 * h) % 16 == 0 and h == (((16 - a % 16) & 15) * 11) & 15     # csrc/stain.hip, head_pixels
    img = np.full((3, 4096, 3), 255, np.uint8)                  # three steps of background ...
    img.reshape(-1, 3)[[0, 4, 4095, 4096, 4099, 8191, 12287]] = 100          # ... and seven tissue pixels
    assert G.step_tissue(img, 0) == ([3, 3, 1], None)
    assert G.step_tissue(img, 4) == ([4, 1], 1)                 # a head of four pixels: step 0 is pixels 4 .. 4099, two full steps, 12287 in a partial one
    assert G.step_tissue(img[:1, :4000], 0) == ([], None)       # under one step: nothing to count
    for h, w, n in G.CASES:
        case = G.Case(h, w, n)
        parents = SO.shifted_he(40 + h + w, n, G.PARENT)
        assert case.imgs.shape == (n, h, w, 3) and len(case.fits) == n
        for i in range(n):
            if n == 3 and i == 1:
                assert (case.imgs[i] == 255).all() and case.n[i] == 0
            elif h * w > G.STEP_PIXELS:
                yy, xx = np.mgrid[:h, :w]
                assert np.array_equal(case.imgs[i], parents[i][yy % G.PARENT, xx % G.PARENT])
            else:
                assert case.n[i] > 0 and any(np.array_equal(case.imgs[i], parents[i][y:y + h, x:x + w])
                                             for y in range(G.PARENT - h + 1) for x in range(G.PARENT - w + 1))
        if h * w >= G.STEP_PIXELS:
            assert len(case.step_tissue) == (1 if n == 1 else 2)
            for full, last in case.step_tissue:
                assert len(full) >= 1 and min(full) > 0 and (last is None or last > 0)
    v = SO.lab_of(SO.shifted_he(3, 1, 128)[0])
    n, s, ss = SO.moments_pairwise(v)
    assert n == 128 * 128
    for a in range(3):
        assert abs(s[a] - math.fsum(v[:, a])) <= 1e-14 * math.fsum(np.abs(v[:, a]))
        for b in range(3):
            p = v[:, a] * v[:, b]
            assert abs(ss[a, b] - math.fsum(p)) <= 1e-14 * math.fsum(np.abs(p)) and ss[a, b] == ss[b, a]
