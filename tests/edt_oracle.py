"""The spec of the exact Euclidean distance transform (csrc/edt.hip, wsi_segmentation_pipeline_amd/distance.py) and of what is built on
it, in NumPy.  The rule is this project's own: a pixel is a feature iff its byte is non-zero (zero with invert),
out[y, x] = min over features (fy, fx) of (y - fy)^2 + (x - fx)^2 as int32, EDT_NONE everywhere on a map without a feature.  SciPy's
convention is the mirror image: distance_transform_edt(features == 0) ** 2 (tests/test_edt_cpu.py compares the two where SciPy is
installed)."""
import math

import numpy as np

EDT_NONE = 0x7FFFFFFF
G_NONE = 0xFFFF
LIMIT = 32768


def features(m, invert=False):
    m = np.asarray(m)
    assert m.ndim == 2 and 1 <= m.shape[0] <= LIMIT and 1 <= m.shape[1] <= LIMIT
    return (m == 0) if invert else (m != 0)


def brute(m, invert=False):
    """the definition itself: an int64 minimum over every feature, for maps up to about 40 x 40"""
    f = features(m, invert)
    h, w = f.shape
    out = np.full((h, w), EDT_NONE, np.int64)
    fy, fx = np.nonzero(f)
    if len(fy):
        y, x = np.mgrid[0:h, 0:w]
        d = (y[..., None] - fy.astype(np.int64)) ** 2 + (x[..., None] - fx.astype(np.int64)) ** 2
        out = d.min(-1)
    return out.astype(np.int32)


def column_distances(m, invert=False):
    """g[y, x]: the distance in rows to the nearest feature of column x as uint16, G_NONE where the column has none"""
    f = features(m, invert)
    h, w = f.shape
    rows = np.arange(h, dtype=np.int64)[:, None]
    far = np.int64(1) << 40
    above = np.maximum.accumulate(np.where(f, rows, -far), 0)                  # the last feature row at or above y
    below = np.minimum.accumulate(np.where(f, rows, far)[::-1], 0)[::-1]       # the first at or below y
    g = np.minimum(rows - above, below - rows)
    return np.where(g >= h, G_NONE, g).astype(np.uint16)


def rows_from_g(g):
    """out[y, x] = min over x' of (x - x')^2 + g[y, x']^2 with G_NONE skipped: per output column one minimum over the candidate
    columns, whole rows at a time"""
    g = np.asarray(g, np.uint16)
    h, w = g.shape
    big = np.int64(1) << 40
    g2 = np.where(g == G_NONE, big, g.astype(np.int64) ** 2)
    xs = np.arange(w, dtype=np.int64)
    out = np.empty((h, w), np.int64)
    chunk = max(1, (1 << 22) // max(1, h * w))                   # output columns per step: about 4M int64 candidates at a time
    for x0 in range(0, w, chunk):
        x = xs[x0:x0 + chunk]
        out[:, x0:x0 + chunk] = (g2[:, None, :] + ((x[:, None] - xs[None, :]) ** 2)[None]).min(-1)
    return np.where(out >= big, EDT_NONE, out).astype(np.int32)


def rows_single(g_row):
    """rows_from_g of one long row, column candidates limited to the finite entries (the 32768-wide hand-made plane)"""
    g_row = np.asarray(g_row, np.uint16)
    w = len(g_row)
    cols = np.nonzero(g_row != G_NONE)[0].astype(np.int64)
    if not len(cols):
        return np.full(w, EDT_NONE, np.int32)
    g2 = g_row[cols].astype(np.int64) ** 2
    xs = np.arange(w, dtype=np.int64)
    return ((xs[:, None] - cols[None, :]) ** 2 + g2[None, :]).min(-1).astype(np.int32)


def distance_sq(m, invert=False):
    """the two-pass spec: column_distances, then rows_from_g"""
    return rows_from_g(column_distances(m, invert))


def distance(m, invert=False):
    d2 = distance_sq(m, invert)
    return np.where(d2 == EDT_NONE, np.inf, np.sqrt(d2.astype(np.float64)))


def morph_disc(mask, r, op):
    """dilate: d2(mask) <= r^2; erode: d2(mask, invert) > r^2 (outside the map is neither feature nor background); open = dilate of
    erode; close = erode of dilate"""
    r2 = int(r) * int(r)
    dilate = lambda m: (distance_sq(m) <= r2).astype(np.uint8)
    erode = lambda m: (distance_sq(m, True) > r2).astype(np.uint8)
    return {'dilate': dilate, 'erode': erode, 'open': lambda m: dilate(erode(m)), 'close': lambda m: erode(dilate(m))}[op](np.asarray(mask))


def margin_band(mask, inner, outer):
    mask = np.asarray(mask)
    inside = mask != 0
    return ((inside & (distance_sq(mask, True) <= int(inner) ** 2)) | (~inside & (distance_sq(mask) <= int(outer) ** 2))).astype(np.uint8)


def bwperim(m):
    """mahotas.labeled.bwperim(n=4), outside counting as unset: a set pixel with an unset or missing 4-neighbour"""
    f = np.pad(np.asarray(m) != 0, 1)
    inner = f[1:-1, 1:-1]
    return (inner & ~(f[:-2, 1:-1] & f[2:, 1:-1] & f[1:-1, :-2] & f[1:-1, 2:])).astype(np.uint8)


def pooled_scores(values, counts, n_a, n_b, spacing=1.0):
    """hd, hd95, assd from the pooled multiset of squared distances, given as ascending unique values and their counts"""
    n = n_a + n_b
    if n_a == 0 and n_b == 0:
        return {'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'n_a': 0, 'n_b': 0}
    if n_a == 0 or n_b == 0:
        return {'hd': math.inf, 'hd95': math.inf, 'assd': math.inf, 'n_a': n_a, 'n_b': n_b}
    values, counts = [int(v) for v in values], [int(c) for c in counts]
    assert sum(counts) == n and values == sorted(set(values))
    k = (95 * n + 99) // 100                                    # ceil(0.95 n): nearest rank
    seen, kth, total = 0, values[-1], 0.0
    for v, c in zip(values, counts):
        if seen < k <= seen + c:
            kth = v
        seen += c
        total += c * math.sqrt(v)                               # ascending order, float64: the same bits every run
    s = float(spacing)
    return {'hd': s * math.sqrt(values[-1]), 'hd95': s * math.sqrt(kth), 'assd': s * total / n, 'n_a': n_a, 'n_b': n_b}


def surface_distances(a, b, spacing=1.0):
    sa, sb = bwperim(a) > 0, bwperim(b) > 0
    n_a, n_b = int(sa.sum()), int(sb.sum())
    if n_a == 0 or n_b == 0:
        return pooled_scores([], [], n_a, n_b, spacing)
    pooled = np.concatenate([distance_sq(sb)[sa], distance_sq(sa)[sb]]).astype(np.int64)
    values, counts = np.unique(pooled, return_counts=True)
    return pooled_scores(values, counts, n_a, n_b, spacing)
