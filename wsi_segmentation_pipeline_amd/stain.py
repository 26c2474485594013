"""Stain normalisation of u8 RGB pixels resident in HBM: Macenko (Macenko et al. 2009) and Reinhard (Reinhard et al. 2001).

The reference has no such code: parity unpinned, own spec (tests/stain_oracle.py).  Every step that touches pixels is a kernel of
csrc/stain.hip (one read of the image per fit step, one read and one write per apply); the host does the 3 x 3 linear algebra in
float64 between them.  Images are (H, W, 3) or (N, H, W, 3) uint8 CUDA tensors; a batch carries per-image parameters.

  fit_macenko / fit_reinhard            -> MacenkoParams / ReinhardParams (a list for a batch)
  normalize_macenko / normalize_reinhard   u8 in, u8 out (``out=img`` normalises in place)
  Normalizer, StainedSlide               the hooks of utils.dataset.Dataset_wsi(s) and utils.eval.predict_breastpathq
"""
import collections
import ctypes as C
import fractions
import math

import numpy as np
import torch

from . import native

IO = 240                                 # transmitted-light intensity of the optical-density table
BETA = 0.15                              # a pixel is tissue iff its optical density is >= BETA in every channel
ALPHA = 1.0                              # the angle percentiles are ALPHA and 100 - ALPHA
ANGLE_BINS = 4096                        # phi over [-pi, pi)
CONC_BINS = 4096                         # each concentration over [0, CONC_MAX)
CONC_MAX = 8.0

MacenkoParams = collections.namedtuple('MacenkoParams', 'he max_c n error', defaults=(None,))
ReinhardParams = collections.namedtuple('ReinhardParams', 'mean std n error', defaults=(None,))
MacenkoParams.__doc__ = 'he (3, 2) float64: haematoxylin, eosin; max_c (2,): 99th percentile of each concentration; n tissue pixels; error: why the fit failed, or None'
ReinhardParams.__doc__ = 'mean, std (3,) float64 of l, alpha, beta over the n tissue pixels (population std); error: why the fit failed, or None'

# the published target of Macenko's method (its authors' reference implementation)
MACENKO_REF = MacenkoParams(np.array([[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]]), np.array([1.9705, 1.0308]), 0)

# Reinhard et al. 2001, equations 4, 6 and 9: RGB -> LMS, LMS -> RGB, and log LMS <-> l-alpha-beta
RGB2LMS = np.array([[0.3811, 0.5783, 0.0402], [0.1967, 0.7244, 0.0782], [0.0241, 0.1288, 0.8444]])
LMS2RGB = np.array([[4.4679, -3.5873, 0.1193], [-1.2186, 2.3809, -0.1624], [0.0497, -0.2439, 1.2045]])
LMS2LAB = np.diag([1 / math.sqrt(3), 1 / math.sqrt(6), 1 / math.sqrt(2)]) @ np.array([[1., 1., 1.], [1., 1., -2.], [1., -1., 0.]])
LAB2LMS = np.array([[1., 1., 1.], [1., 1., -1.], [1., -2., 0.]]) @ np.diag([math.sqrt(3) / 3, math.sqrt(6) / 6, math.sqrt(2) / 2])


def od_table(io=IO):
    """od[v] = -ln((v + 1) / io), float64 rounded to fp32: the values the kernels and the spec share."""
    return (-np.log((np.arange(256, dtype=np.float64) + 1.0) / io)).astype(np.float32)


def tissue_v_max(io=IO, beta=BETA):
    """The largest byte whose optical density is >= beta: od_c >= beta in all channels iff max(r, g, b) <= v_max (205 at the defaults)."""
    return int(math.floor(io * math.exp(-beta))) - 1


def percentile_from_hist(hist, p, lo, hi):
    """The p-th percentile of a histogram over [lo, hi) in equal bins: the centre of the bin that holds rank max(1, ceil(p / 100 * n))
    of the n counted values (rank 1 = the smallest).  The rank is found in exact arithmetic."""
    hist = np.asarray(hist).astype(np.int64).reshape(-1)
    n = int(hist.sum())
    if n <= 0:
        raise ValueError('percentile of an empty histogram')
    rank = max(1, math.ceil(fractions.Fraction(p) * n / 100))
    k = int(np.searchsorted(np.cumsum(hist), rank, side='left'))
    return lo + (k + 0.5) * (hi - lo) / hist.size


# ---------------------------------------------------------------------------------------------------------------- device plumbing
def _images(img, what='img'):
    """(the tensor as (N, H, W, 3), batched?) of a u8 CUDA image or batch"""
    if not isinstance(img, torch.Tensor) or not img.is_cuda:
        raise RuntimeError('stain normalisation runs on the GPU (MI355X) only: %s must be a CUDA tensor' % what)
    if img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3 or not img.is_contiguous() or img.numel() == 0:
        raise ValueError('%s must be a contiguous uint8 (H, W, 3) or (N, H, W, 3) tensor' % what)
    return (img if img.dim() == 4 else img.unsqueeze(0)), img.dim() == 4


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _dev(arr, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=dtype)).to(dev)


_luts = {}


def _od_lut(dev, io):
    key = (str(dev), float(io))
    if key not in _luts:
        _luts[key] = _dev(od_table(io), np.float32, dev)
    return _luts[key]


def _moments(x, lab, io, beta):
    """(N, 10) float64 on the host: n, sum x, sum x (x) x over the tissue pixels of every image"""
    lib = native.load()
    n, npix, dev = x.shape[0], x.shape[1] * x.shape[2], x.device
    scratch = torch.empty(lib.wsi_stain_moments_scratch_bytes(npix, n), dtype=torch.uint8, device=dev)
    out = torch.empty((n, 10), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        if lab:
            rc = lib.wsi_stain_lab_moments(x.data_ptr(), npix, n, tissue_v_max(io, beta), out.data_ptr(), scratch.data_ptr(), _stream(dev))
        else:
            rc = lib.wsi_stain_od_moments(x.data_ptr(), npix, n, tissue_v_max(io, beta), _od_lut(dev, io).data_ptr(), out.data_ptr(),
                                          scratch.data_ptr(), _stream(dev))
    native.check(rc, 'wsi_stain_lab_moments' if lab else 'wsi_stain_od_moments')
    return out.cpu().numpy()


def _hist(x, conc, prm, io, beta):
    """angle (N, ANGLE_BINS) or concentration (N, 2, CONC_BINS) counts on the host; prm (N, 6) float64"""
    lib = native.load()
    n, npix, dev = x.shape[0], x.shape[1] * x.shape[2], x.device
    out = torch.empty((n, 2, CONC_BINS) if conc else (n, ANGLE_BINS), dtype=torch.int64, device=dev)
    p = _dev(prm, np.float32, dev)
    with torch.cuda.device(dev):
        if conc:
            rc = lib.wsi_stain_conc_hist(x.data_ptr(), npix, n, tissue_v_max(io, beta), _od_lut(dev, io).data_ptr(), p.data_ptr(), CONC_BINS,
                                         CONC_MAX, out.data_ptr(), _stream(dev))
        else:
            rc = lib.wsi_stain_angle_hist(x.data_ptr(), npix, n, tissue_v_max(io, beta), _od_lut(dev, io).data_ptr(), p.data_ptr(), ANGLE_BINS,
                                          out.data_ptr(), _stream(dev))
    native.check(rc, 'wsi_stain_conc_hist' if conc else 'wsi_stain_angle_hist')
    return out.cpu().numpy()


def _one_or_list(params, batched):
    if batched:
        return params
    if params[0].error:
        raise ValueError(params[0].error)
    return params[0]


# ---------------------------------------------------------------------------------------------------------------------------- fits
def macenko_plane(mom):
    """V (3, 2): the two leading eigenvectors of the optical-density covariance (divisor n - 1) of one image's moments, each flipped to
    a component sum >= 0.  ValueError: fewer than two tissue pixels, or a covariance of rank < 2."""
    n = int(mom[0])
    if n < 2:
        raise ValueError('%d tissue pixels: a stain fit needs at least two' % n)
    s = mom[1:4]
    ss = np.array([[mom[4], mom[5], mom[6]], [mom[5], mom[7], mom[8]], [mom[6], mom[8], mom[9]]])
    cov = (ss - np.outer(s, s) / n) / (n - 1)
    val, vec = np.linalg.eigh(cov)
    if not (val[2] > 0 and val[1] > 1e-9 * val[2]):
        raise ValueError('the optical densities of the tissue pixels do not span a plane (rank-deficient covariance)')
    v = vec[:, [2, 1]]
    return v * np.where(v.sum(0) >= 0, 1.0, -1.0)


def macenko_vectors(angle_hist, v, alpha=ALPHA):
    """HE (3, 2) from the angle histogram: V (cos phi, sin phi) at the alpha and 100 - alpha percentiles, haematoxylin (the larger first
    component) first."""
    lo = percentile_from_hist(angle_hist, alpha, -math.pi, math.pi)
    hi = percentile_from_hist(angle_hist, 100 - alpha, -math.pi, math.pi)
    a, b = v @ np.array([math.cos(lo), math.sin(lo)]), v @ np.array([math.cos(hi), math.sin(hi)])
    return np.stack((a, b), 1) if a[0] > b[0] else np.stack((b, a), 1)


def fit_macenko(img, io=IO, beta=BETA, alpha=ALPHA):
    """MacenkoParams of an image (ValueError where the fit fails) or the list of a batch's (a failed image: `.error` says why)."""
    x, batched = _images(img)
    n = x.shape[0]
    mom = _moments(x, False, io, beta)
    planes, errors = np.zeros((n, 3, 2)), [None] * n
    for i in range(n):
        try:
            planes[i] = macenko_plane(mom[i])
        except ValueError as e:
            errors[i] = str(e)
    ah = _hist(x, False, planes.reshape(n, 6), io, beta)
    he, pinv = np.zeros((n, 3, 2)), np.zeros((n, 2, 3))
    for i in range(n):
        if errors[i] is None:
            he[i] = macenko_vectors(ah[i], planes[i], alpha)
            pinv[i] = np.linalg.pinv(he[i])
    ch = _hist(x, True, pinv.reshape(n, 6), io, beta)
    out = []
    for i in range(n):
        if errors[i] is None:
            max_c = np.array([percentile_from_hist(ch[i, r], 99, 0.0, CONC_MAX) for r in range(2)])
            out.append(MacenkoParams(he[i], max_c, int(mom[i, 0])))
        else:
            out.append(MacenkoParams(None, None, int(mom[i, 0]), errors[i]))
    return _one_or_list(out, batched)


def fit_reinhard(img, io=IO, beta=BETA):
    """ReinhardParams of an image (ValueError where the fit fails) or the list of a batch's (a failed image: `.error` says why)."""
    x, batched = _images(img)
    mom = _moments(x, True, io, beta)
    out = []
    for m in mom:
        n = int(m[0])
        if n < 2:
            out.append(ReinhardParams(None, None, n, '%d tissue pixels: a stain fit needs at least two' % n))
            continue
        mean = m[1:4] / n
        var = m[[4, 7, 9]] / n - mean * mean
        if not np.all(var > 1e-12):
            out.append(ReinhardParams(None, None, n, 'a channel of the tissue pixels has zero variance'))
        else:
            out.append(ReinhardParams(mean, np.sqrt(var), n))
    return _one_or_list(out, batched)


# ------------------------------------------------------------------------------------------------------------------------- applies
def macenko_matrix(params, target=MACENKO_REF):
    """A (3, 3) float64 = HERef diag(maxCRef / maxC) pinv(HE): normalised optical density = A . od."""
    return np.asarray(target.he) @ np.diag(np.asarray(target.max_c) / np.asarray(params.max_c)) @ np.linalg.pinv(np.asarray(params.he))


def reinhard_affine(params, target):
    """(G (3, 3), g (3,)) float64 with log10 LMS' = G . log10 LMS + g: l-alpha-beta, (x - mean_src) std_tgt / std_src + mean_tgt, and back."""
    k = np.asarray(target.std) / np.asarray(params.std)
    return LAB2LMS @ np.diag(k) @ LMS2LAB, LAB2LMS @ (np.asarray(target.mean) - k * np.asarray(params.mean))


def _apply(x, out, macenko, prm, v_max, io):
    lib = native.load()
    n, npix, dev = x.shape[0], x.shape[1] * x.shape[2], x.device
    if out is None:
        out = torch.empty_like(x)
    else:
        o, _ = _images(out, 'out')
        if o.shape != x.shape or o.device != dev:
            raise ValueError('out must have the shape and device of img')
        out = o
    p, vm = _dev(prm, np.float32, dev), _dev(v_max, np.int32, dev)
    with torch.cuda.device(dev):
        if macenko:
            rc = lib.wsi_stain_macenko_apply(x.data_ptr(), out.data_ptr(), npix, n, vm.data_ptr(), _od_lut(dev, io).data_ptr(), p.data_ptr(),
                                             float(io), _stream(dev))
        else:
            rc = lib.wsi_stain_reinhard_apply(x.data_ptr(), out.data_ptr(), npix, n, vm.data_ptr(), p.data_ptr(), _stream(dev))
    native.check(rc, 'wsi_stain_macenko_apply' if macenko else 'wsi_stain_reinhard_apply')
    return out


def _normalize(img, params, fit, fold, nprm, out, background, io, beta):
    if background not in ('keep', 'all'):
        raise ValueError("background must be 'keep' or 'all'")
    x, batched = _images(img)
    if params is None:
        params = fit(img)
    plist = list(params) if batched else [params]
    if len(plist) != x.shape[0]:
        raise ValueError('%d parameter sets for %d images' % (len(plist), x.shape[0]))
    prm = np.zeros((x.shape[0], nprm))
    v_max = np.full(x.shape[0], tissue_v_max(io, beta) if background == 'keep' else 255, np.int32)
    for i, p in enumerate(plist):
        if p.error:
            v_max[i] = -1                                       # a failed fit: the image is served as it is
        else:
            prm[i] = fold(p)
    res = _apply(x, out, nprm == 9, prm, v_max, io)
    return res if batched else res[0]


def normalize_macenko(img, params=None, target=MACENKO_REF, out=None, background='keep', io=IO, beta=BETA):
    """`img` with its stain mapped onto `target` (MACENKO_REF, or another image's fitted MacenkoParams).  params=None: fitted on `img`
    (per image of a batch; an image whose fit fails is copied).  background='keep': non-tissue pixels are copied, 'all': every pixel is
    transformed.  out=img normalises in place."""
    return _normalize(img, params, lambda t: fit_macenko(t, io, beta), lambda p: (-math.log2(math.e) * macenko_matrix(p, target)).reshape(9),
                      9, out, background, io, beta)


def normalize_reinhard(img, target, params=None, out=None, background='keep', io=IO, beta=BETA):
    """`img` with the l-alpha-beta mean and standard deviation of its tissue mapped onto those of `target` (ReinhardParams fitted on an
    image of the caller's choice).  The other arguments as normalize_macenko."""
    def fold(p):
        g3, g = reinhard_affine(p, target)
        return np.concatenate((g3.reshape(9), g * math.log2(10.0)))
    return _normalize(img, params, lambda t: fit_reinhard(t, io, beta), fold, 12, out, background, io, beta)


# --------------------------------------------------------------------------------------------------------------------------- hooks
class Normalizer:
    """One method and one target: what Dataset_wsi(s)(stain=...) and predict_breastpathq(stain=...) take.  method 'macenko' (target: None
    = MACENKO_REF, or MacenkoParams) or 'reinhard' (target: ReinhardParams, required).  fit_level: the pyramid level a StainedSlide fits
    on (None: min(2, level_count - 1)).  Further keywords (background, io, beta) go to fit and normalize."""

    def __init__(self, method, target=None, fit_level=None, **kw):
        if method not in ('macenko', 'reinhard'):
            raise ValueError("method must be 'macenko' or 'reinhard'")
        if method == 'reinhard' and not isinstance(target, ReinhardParams):
            raise ValueError('Reinhard has no built-in target: pass ReinhardParams fitted on an image of your choice')
        self.method, self.fit_level, self.kw = method, fit_level, kw
        self.target = MACENKO_REF if target is None else target

    def fit(self, img):
        kw = {k: v for k, v in self.kw.items() if k in ('io', 'beta')}
        return fit_macenko(img, **kw) if self.method == 'macenko' else fit_reinhard(img, **kw)

    def apply(self, img, params=None, out=None):
        """`img` normalised with `params` (None: fitted on img itself, per image of a batch)"""
        if self.method == 'macenko':
            return normalize_macenko(img, params, self.target, out, **self.kw)
        return normalize_reinhard(img, self.target, params, out, **self.kw)


class StainedSlide:
    """A slide whose resident levels are stain-normalised.  The parameters are fitted once, on scan.device_level(fit_level), and applied
    to whichever level is asked for; the result is cached per (level, device).  read_region stays raw (nuclei masks and overlays keep
    the scanner's colours).  A slide whose fit fails is served un-normalised and `.stain_error` says why."""

    def __init__(self, scan, normalizer):
        self.scan, self.normalizer = scan, normalizer
        self.stain_params, self.stain_error = None, None
        self._dev = {}

    level_dimensions = property(lambda self: self.scan.level_dimensions)
    level_downsamples = property(lambda self: self.scan.level_downsamples)
    level_count = property(lambda self: self.scan.level_count)
    dimensions = property(lambda self: self.scan.dimensions)

    def read_region(self, location, level, size):
        return self.scan.read_region(location, level, size)

    def __getattr__(self, name):                                # whatever else the scan offers (name, level_array, ...)
        return getattr(self.__dict__['scan'], name)

    def close(self):
        self._dev.clear()
        if hasattr(self.scan, 'close'):
            self.scan.close()

    def _fit(self, device):
        if self.stain_params is None and self.stain_error is None:
            lvl = self.normalizer.fit_level
            lvl = min(2, self.scan.level_count - 1) if lvl is None else lvl
            try:
                self.stain_params = self.normalizer.fit(self.scan.device_level(lvl, device))
            except ValueError as e:
                self.stain_error = str(e)
        return self.stain_params

    def device_level(self, level, device):
        key = (level, str(device))
        if key not in self._dev:
            raw = self.scan.device_level(level, device)
            params = self._fit(device)
            self._dev[key] = raw if params is None else self.normalizer.apply(raw, params)
        return self._dev[key]
