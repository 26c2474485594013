"""The coverage rule of the annotation rasteriser (wsi_segmentation_pipeline_amd/annotations.py, csrc/poly_dev.h), written once in
NumPy int64: the spec the host program and the device kernel are compared with, byte for byte.

A polygon is n >= 1 integer vertices, closed implicitly; a lattice point p = (px, py) is in full-resolution coordinates.
  edge      its ends sorted by y into lo and hi.  With lo.y == hi.y it never crosses; otherwise it crosses iff lo.y <= py < hi.y and
            (hi.x - lo.x) (py - lo.y) - (px - lo.x) (hi.y - lo.y) > 0: the edge is strictly to the right of p on p's scanline.
  coverage  p is covered if it lies on any closed edge (that cross product 0 and p inside the edge's box; a zero-length edge is its own
            point), or if the number of crossings is odd (even-odd rule).
  output    pixel (x, y) of the W x H u8 map samples p = (ox + x sx, oy + y sy); polygons are painted in list order, a covered pixel takes
            the label of the last polygon covering it (label 0 erases), an uncovered one keeps what `out` held (0 for a fresh map).
  limits    every coordinate and every sampled point lies in [-2^29, 2^29]: a difference fits 31 bits, a cross product int64."""
import math

import numpy as np

LIMIT = 1 << 29


def covered(poly, px, py):
    """bool array (the broadcast shape of px and py): the points the polygon covers"""
    v = np.asarray(poly, np.int64).reshape(-1, 2)
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    shape = np.broadcast(px, py).shape
    odd, on = np.zeros(shape, bool), np.zeros(shape, bool)
    for i in range(len(v)):
        a, b = v[i], v[(i + 1) % len(v)]
        lo, hi = (a, b) if a[1] <= b[1] else (b, a)
        cross = (hi[0] - lo[0]) * (py - lo[1]) - (px - lo[0]) * (hi[1] - lo[1])
        if lo[1] != hi[1]:
            odd ^= (lo[1] <= py) & (py < hi[1]) & (cross > 0)
        on |= (cross == 0) & (px >= min(a[0], b[0])) & (px <= max(a[0], b[0])) & (py >= lo[1]) & (py <= hi[1])
    return on | odd


def boundary(poly, px, py):
    """the on-an-edge half of the rule alone"""
    v = np.asarray(poly, np.int64).reshape(-1, 2)
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    on = np.zeros(np.broadcast(px, py).shape, bool)
    for i in range(len(v)):
        a, b = v[i], v[(i + 1) % len(v)]
        cross = (b[0] - a[0]) * (py - a[1]) - (px - a[0]) * (b[1] - a[1])
        on |= (cross == 0) & (px >= min(a[0], b[0])) & (px <= max(a[0], b[0])) & (py >= min(a[1], b[1])) & (py <= max(a[1], b[1]))
    return on


def edge_lattice_points(poly):
    """the lattice points on the closed edges, enumerated by gcd stepping: {(x, y)}"""
    v = [(int(x), int(y)) for x, y in np.asarray(poly, np.int64).reshape(-1, 2)]
    pts = set()
    for i, (ax, ay) in enumerate(v):
        bx, by = v[(i + 1) % len(v)]
        g = math.gcd(abs(bx - ax), abs(by - ay))
        if g == 0:
            pts.add((ax, ay))
            continue
        sx, sy = (bx - ax) // g, (by - ay) // g
        pts.update((ax + k * sx, ay + k * sy) for k in range(g + 1))
    return pts


def rasterize(coords, labels, size, step=1, origin=(0, 0), out=None):
    """the (H, W) u8 map; `out` (H, W) u8 is painted over in place of a fresh map of zeros and is left unchanged itself"""
    w, h = int(size[0]), int(size[1])
    sx, sy = (int(step), int(step)) if np.isscalar(step) else (int(step[0]), int(step[1]))
    res = np.zeros((h, w), np.uint8) if out is None else np.array(out, np.uint8)
    assert res.shape == (h, w) and sx >= 1 and sy >= 1
    px = (int(origin[0]) + np.arange(w, dtype=np.int64) * sx)[None, :]
    py = (int(origin[1]) + np.arange(h, dtype=np.int64) * sy)[:, None]
    for poly, label in zip(coords, labels):
        res[covered(poly, px, py)] = int(label)
    return res
