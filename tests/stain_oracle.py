"""The specification of the stain normalisation (wsi_segmentation_pipeline_amd/stain.py, csrc/stain.hip), in float64 NumPy.

The reference has no such code, so this file IS the spec: Macenko et al. 2009 and Reinhard et al. 2001 restated so that a GPU can follow
them deterministically.  It shares with the package only the named constants and `percentile_from_hist`; everything numeric is written
out here.

Common: od[v] = -ln((v + 1) / Io), v = 0..255, float64 rounded to fp32 (the fp32 values are the spec); a pixel is tissue iff
od_c >= beta in all three channels, i.e. max(r, g, b) <= v_max = floor(Io exp(-beta)) - 1.

Macenko: (1) n, sum od, sum od (x) od over tissue pixels in float64 -> covariance (divisor n - 1) -> eigh -> the two leading eigenvectors
V (3 x 2), each flipped to a component sum >= 0; (2) phi = atan2(od . V2, od . V1), histogram over [-pi, pi) in ANGLE_BINS bins,
phi_lo / phi_hi = percentiles alpha and 100 - alpha (centre of the bin holding rank max(1, ceil(p / 100 n))), stain vectors
V (cos phi, sin phi), haematoxylin = the larger first component, HE = [H, E]; (3) C = pinv(HE) od, each row histogrammed over
[0, CONC_MAX) in CONC_BINS bins (values outside clamped into the end bins), maxC = 99th percentile of each row; (4) A = HERef
diag(maxCRef / maxC) pinv(HE), out_c = clamp(floor(Io exp(-(A od)_c) + 0.5), 0, 255).

Reinhard: rgb = (v + 1) / 256 -> LMS -> log10 -> l-alpha-beta (the paper's matrices); fit = n, mean and population standard deviation per
channel over tissue pixels; apply x' = (x - mean_src) std_tgt / std_src + mean_tgt, back through the inverse transform,
out_c = clamp(floor(256 rgb'_c - 1 + 0.5), 0, 255).

background 'keep' copies non-tissue pixels, 'all' transforms every pixel.  A fit raises ValueError for fewer than two tissue pixels, a
zero variance (Reinhard) or a rank-deficient covariance (Macenko)."""
import numpy as np

from wsi_segmentation_pipeline_amd.stain import ALPHA, ANGLE_BINS, BETA, CONC_BINS, CONC_MAX, IO, MACENKO_REF, percentile_from_hist

OD = (-np.log((np.arange(256, dtype=np.float64) + 1.0) / IO)).astype(np.float32)
V_MAX = int(np.floor(IO * np.exp(-BETA))) - 1

RGB2LMS = np.array([[0.3811, 0.5783, 0.0402], [0.1967, 0.7244, 0.0782], [0.0241, 0.1288, 0.8444]])
LMS2RGB = np.array([[4.4679, -3.5873, 0.1193], [-1.2186, 2.3809, -0.1624], [0.0497, -0.2439, 1.2045]])
_P = np.array([[1., 1., 1.], [1., 1., -2.], [1., -1., 0.]])
LMS2LAB = np.diag([1 / np.sqrt(3), 1 / np.sqrt(6), 1 / np.sqrt(2)]) @ _P
LAB2LMS = _P.T @ np.diag([np.sqrt(3) / 3, np.sqrt(6) / 6, np.sqrt(2) / 2])


def tissue(img):
    """bool (H, W): the tissue pixels of a u8 (H, W, 3) image"""
    return img.max(-1) <= V_MAX


def od_of(img):
    """(npix, 3) float64 optical densities (the fp32 table values) of the pixels `img` lists"""
    return OD[img.reshape(-1, 3)].astype(np.float64)


def od_moments(img):
    """(n, sum od (3,), sum od (x) od (3, 3)) over the tissue pixels"""
    x = od_of(img[tissue(img)])
    return x.shape[0], x.sum(0), x.T @ x


def moments_vector(n, s, ss):
    """the ten numbers in the order of wsi_stain_od_moments / wsi_stain_lab_moments"""
    return np.array([n, s[0], s[1], s[2], ss[0, 0], ss[0, 1], ss[0, 2], ss[1, 1], ss[1, 2], ss[2, 2]], np.float64)


def moments_pairwise(v):
    """(n, sum v (3,), sum v (x) v (3, 3)) over the rows of v (n, 3), every sum formed by np.sum over one contiguous vector, which adds
    pairwise: the rounding error grows with log2 n (about 32 units of 2^-53 of the sum of magnitudes at 8e6 rows), and no BLAS decides
    the order.  The reference for the kernels' moments at any size."""
    cols = [np.ascontiguousarray(v[:, k]) for k in range(3)]
    s = np.array([np.sum(c) for c in cols])
    ss = np.array([[np.sum(cols[a] * cols[b]) for b in range(3)] for a in range(3)])
    return v.shape[0], s, ss


def macenko_plane(img):
    n, s, ss = od_moments(img)
    if n < 2:
        raise ValueError('fewer than two tissue pixels')
    val, vec = np.linalg.eigh((ss - np.outer(s, s) / n) / (n - 1))
    if not (val[2] > 0 and val[1] > 1e-9 * val[2]):
        raise ValueError('rank-deficient covariance')
    v = vec[:, [2, 1]]
    return v * np.where(v.sum(0) >= 0, 1.0, -1.0)


def _bins(x, lo, hi, nbins):
    return np.clip(np.floor((x - lo) / (hi - lo) * nbins).astype(np.int64), 0, nbins - 1)


def angle_hist(img, v):
    x = od_of(img[tissue(img)])
    phi = np.arctan2(x @ v[:, 1], x @ v[:, 0])
    return np.bincount(_bins(phi, -np.pi, np.pi, ANGLE_BINS), minlength=ANGLE_BINS)


def stain_vectors(hist, v):
    lo, hi = percentile_from_hist(hist, ALPHA, -np.pi, np.pi), percentile_from_hist(hist, 100 - ALPHA, -np.pi, np.pi)
    a, b = v @ np.array([np.cos(lo), np.sin(lo)]), v @ np.array([np.cos(hi), np.sin(hi)])
    return np.stack((a, b), 1) if a[0] > b[0] else np.stack((b, a), 1)


def conc_hist(img, he):
    c = od_of(img[tissue(img)]) @ np.linalg.pinv(he).T
    return np.stack([np.bincount(_bins(c[:, r], 0.0, CONC_MAX, CONC_BINS), minlength=CONC_BINS) for r in range(2)])


def fit_macenko(img):
    """(HE (3, 2), maxC (2,), n)"""
    v = macenko_plane(img)
    he = stain_vectors(angle_hist(img, v), v)
    ch = conc_hist(img, he)
    return he, np.array([percentile_from_hist(ch[r], 99, 0.0, CONC_MAX) for r in range(2)]), int(tissue(img).sum())


def macenko_matrix(he, max_c, target=(MACENKO_REF.he, MACENKO_REF.max_c)):
    return np.asarray(target[0]) @ np.diag(np.asarray(target[1]) / max_c) @ np.linalg.pinv(he)


def _finish(img, new, background):
    out = np.clip(np.floor(new), 0, 255).astype(np.uint8).reshape(img.shape)
    if background == 'keep':
        out[~tissue(img)] = img[~tissue(img)]
    return out


def apply_macenko(img, a, background='keep'):
    return _finish(img, IO * np.exp(-(od_of(img) @ a.T)) + 0.5, background)


def lab_of(img):
    """(npix, 3) float64 l-alpha-beta of the pixels `img` lists"""
    rgb = (img.reshape(-1, 3).astype(np.float64) + 1.0) / 256.0
    return np.log10(rgb @ RGB2LMS.T) @ LMS2LAB.T


def lab_moments(img):
    x = lab_of(img[tissue(img)])
    return x.shape[0], x.sum(0), x.T @ x


def fit_reinhard(img):
    """(mean (3,), std (3,), n)"""
    x = lab_of(img[tissue(img)])
    if x.shape[0] < 2:
        raise ValueError('fewer than two tissue pixels')
    mean = x.sum(0) / x.shape[0]
    var = (x * x).sum(0) / x.shape[0] - mean * mean
    if not np.all(var > 1e-12):
        raise ValueError('zero variance')
    return mean, np.sqrt(var), x.shape[0]


def apply_reinhard(img, src, tgt, background='keep'):
    """src, tgt: (mean, std) pairs"""
    x = (lab_of(img) - src[0]) * (tgt[1] / src[1]) + tgt[0]
    rgb = (10.0 ** (x @ LAB2LMS.T)) @ LMS2RGB.T
    return _finish(img, 256.0 * rgb - 1.0 + 0.5, background)


def shifted_he(seed, n, size, gamma=(1.3, 0.8, 1.1)):
    """The tests' input family: synthetic.make_he_patches as (n, size, size, 3), stain-shifted by a per-channel gamma"""
    from wsi_segmentation_pipeline_amd import synthetic
    x = synthetic.make_he_patches(seed, n, size).transpose(0, 2, 3, 1).astype(np.float64) / 255.0
    return np.ascontiguousarray(np.rint(255.0 * x ** np.asarray(gamma)).astype(np.uint8))
