"""The hull rule of wsi_segmentation_pipeline_amd/regions.py (csrc/region_hulls_dev.h, csrc/region_hulls.hip), written once in Python
integers (NumPy scalars overflow at these sizes): the spec the device is pinned to byte for byte.  The rule is this project's own (parity
unpinned).

A pixel (x, y) is the unit square (x, y) .. (x + 1, y + 1) in map corner coordinates.  A region of regions_oracle.label is the union of
its pixels' squares; its hull is the convex hull of that union.  Only the corners (x0, y), (x0, y + 1), (x1, y), (x1, y + 1) of its runs
[x0, x1) can be vertices, and of those only the leftmost and the rightmost of every corner row.  Vertices are strictly convex, start at
the smallest (y, x) and go clockwise as seen with y pointing down.  A hull's record is sixteen int64, FIELDS below."""
import math

import numpy as np

import regions_oracle as RO

FIELDS = ('hull_first', 'hull_n', 'hull_area2', 'feret_sq', 'feret_a', 'feret_b', 'width_num', 'width_den', 'width_edge', 'width_vertex', 'orth_num',
          'zero0', 'zero1', 'zero2', 'zero3', 'zero4')
F = {name: k for k, name in enumerate(FIELDS)}
PIECE = 64                               # csrc/region_hulls_dev.h PIECE: corner rows one lane chains at the first level
GROUP_ROWS = 64 * PIECE                  # corner rows one first-level workgroup stages


def cross(ux, uy, vx, vy):
    return ux * vy - uy * vx


def chain(points, side):
    """Andrew's monotone chain over points sorted by y: side 0 keeps the right chain (turn > 0 at every kept point), side 1 the left"""
    st = []
    for c in points:
        while len(st) >= 2:
            a, b = st[-2], st[-1]
            t = cross(b[0] - a[0], b[1] - a[1], c[0] - b[0], c[1] - b[1])
            if (t <= 0) if side == 0 else (t >= 0):
                st.pop()
            else:
                break
        st.append(c)
    return st


def hull_of_rows(y0, lo, hi):
    """the vertex list [(x, y)] from the leftmost and rightmost corner of the corner rows y0, y0 + 1, ..; and the two chains as rows j"""
    right = chain([(int(x), y0 + j) for j, x in enumerate(hi)], 0)
    left = chain([(int(x), y0 + j) for j, x in enumerate(lo)], 1)
    return [left[0]] + right + left[:0:-1], [p[1] - y0 for p in right], [p[1] - y0 for p in left]


def measure(v):
    """(hull_area2, feret_sq, feret_a, feret_b, width_num, width_den, width_edge, width_vertex, orth_num) of a vertex list, all int"""
    n = len(v)
    area2 = sum(cross(v[i][0], v[i][1], v[(i + 1) % n][0], v[(i + 1) % n][1]) for i in range(n))
    best, fa, fb = 0, 0, 0
    for i in range(n):
        for j in range(i + 1, n):
            d = (v[j][0] - v[i][0]) ** 2 + (v[j][1] - v[i][1]) ** 2
            if d > best:
                best, fa, fb = d, i, j
    width = None
    for i in range(n):
        ex, ey = v[(i + 1) % n][0] - v[i][0], v[(i + 1) % n][1] - v[i][1]
        c, far = 0, 0
        for t in range(n):
            a = abs(cross(ex, ey, v[t][0] - v[i][0], v[t][1] - v[i][1]))
            if a > c:
                c, far = a, t
        num, den = c * c, ex * ex + ey * ey
        if width is None or num * width[1] < width[0] * den:      # exact: Python integers
            width = (num, den, i, far)
    dx, dy = v[fb][0] - v[fa][0], v[fb][1] - v[fa][1]
    cs = [cross(dx, dy, p[0] - v[fa][0], p[1] - v[fa][1]) for p in v]
    return (area2, best, fa, fb) + width + (max(cs) - min(cs),)


class Hulls:
    """n hulls: table (n, 16) int64, vertices (V, 2) int32, polys (the vertex lists), and the device workspace's arrays (height, row_off,
    lo, hi, st_r, st_l, n_r, n_l, count, first; the chains are the final ones)"""

    def __init__(self, **k):
        self.__dict__.update(k)

    def __getattr__(self, name):
        if name in F:
            return self.table[:, F[name]]
        raise AttributeError(name)


def corner_rows(r):
    """per region (y0, lo list, hi list) from the runs and ids of a regions_oracle.Regions"""
    t = r.table
    rows = [(int(t[k, RO.F['y0']]), [RO.LIMIT + 1] * int(t[k, RO.F['y1']] - t[k, RO.F['y0']] + 1), [-1] * int(t[k, RO.F['y1']] - t[k, RO.F['y0']] + 1))
            for k in range(r.n)]
    for (y, x0, x1, _), ident in zip(r.runs.tolist(), r.id.tolist()):
        y0, lo, hi = rows[ident - 1]
        for j in (y - y0, y - y0 + 1):
            lo[j], hi[j] = min(lo[j], x0), max(hi[j], x1)
    return rows


def hulls(r):
    """the hulls of every region of a regions_oracle.Regions"""
    rows = corner_rows(r)
    table = np.zeros((r.n, 16), np.int64)
    polys, first = [], 0
    ws = dict(height=[], lo=[], hi=[], st_r=[], st_l=[], n_r=[], n_l=[])
    for k, (y0, lo, hi) in enumerate(rows):
        v, right, left = hull_of_rows(y0, lo, hi)
        table[k, :11] = (first, len(v)) + measure(v)
        polys.append(v)
        first += len(v)
        ws['height'].append(len(lo))
        ws['lo'] += lo
        ws['hi'] += hi
        ws['st_r'] += right + [0] * (len(lo) - len(right))
        ws['st_l'] += left + [0] * (len(lo) - len(left))
        ws['n_r'].append(len(right))
        ws['n_l'].append(len(left))
    vertices = np.asarray([p for v in polys for p in v], np.int32).reshape(-1, 2)
    height = np.asarray(ws['height'] + [0], np.uint32)
    count = np.asarray([len(v) for v in polys] + [0], np.uint32)
    return Hulls(n=r.n, table=table, vertices=vertices, polys=polys, height=height, row_off=np.concatenate([[0], np.cumsum(height[:-1])]).astype(np.uint32),
                 lo=np.asarray(ws['lo'], np.int32), hi=np.asarray(ws['hi'], np.int32), st_r=np.asarray(ws['st_r'], np.uint32),
                 st_l=np.asarray(ws['st_l'], np.uint32), n_r=np.asarray(ws['n_r'], np.uint32), n_l=np.asarray(ws['n_l'], np.uint32), count=count,
                 first=np.concatenate([[0], np.cumsum(count[:-1])]).astype(np.uint32))


def label(m, classes=None, connectivity=8, weight=None):
    """-> (regions_oracle.Regions, Hulls)"""
    r = RO.label(m, classes, connectivity, weight)
    return r, hulls(r)


# ------------------------------------------------------------------------------------------------------ the definitions, by brute force
def corners_of(r):
    """per region, every corner of its runs, sorted"""
    out = [set() for _ in range(r.n)]
    for (y, x0, x1, _), ident in zip(r.runs.tolist(), r.id.tolist()):
        out[ident - 1] |= {(x0, y), (x0, y + 1), (x1, y), (x1, y + 1)}
    return [sorted(s) for s in out]


def plain_hull(points):
    """the strictly convex hull of any point set as a set of points (Andrew's chain over the x-sorted points): the textbook form the row
    form above is checked against"""
    pts = sorted(set(points))
    def half(seq):
        st = []
        for c in seq:
            while len(st) >= 2 and cross(st[-1][0] - st[-2][0], st[-1][1] - st[-2][1], c[0] - st[-1][0], c[1] - st[-1][1]) <= 0:
                st.pop()
            st.append(c)
        return st
    return set(half(pts)) | set(half(pts[::-1]))


def brute_feret_sq(points):
    return max((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 for a in points for b in points)


def brute_width(points, v):
    """the least squared extent of all `points` along an edge normal of the polygon v, as (num, den) of the first edge that attains it"""
    best = None
    for i in range(len(v)):
        ex, ey = v[(i + 1) % len(v)][0] - v[i][0], v[(i + 1) % len(v)][1] - v[i][1]
        proj = [cross(ex, ey, p[0] - v[i][0], p[1] - v[i][1]) for p in points]
        num, den = (max(proj) - min(proj)) ** 2, ex * ex + ey * ey
        if best is None or num * best[1] < best[0] * den:
            best = (num, den)
    return best


# ------------------------------------------------------------------------------------------------------------------- what follows
def feret_max(t):
    return [math.sqrt(int(x)) for x in t[:, F['feret_sq']]]


def feret_min(t):
    return [math.sqrt(int(n) / int(d)) for n, d in zip(t[:, F['width_num']], t[:, F['width_den']])]


def feret_orth(t):
    return [int(o) / math.sqrt(int(f)) for o, f in zip(t[:, F['orth_num']], t[:, F['feret_sq']])]


def bed_size(mask, step=1, mpp=None):
    """the host rule of regions.bed_size on the spec: the largest region (ties: the smallest id) of a u8 mask at connectivity 8"""
    r, h = label(np.asarray(mask, np.uint8), None, 8)
    if r.n == 0:
        return None
    k = int(np.argmax(r.table[:, RO.F['area']]))
    area, hull_area = int(r.table[k, RO.F['area']]), int(h.table[k, F['hull_area2']]) / 2
    out = dict(d1=feret_max(h.table)[k], d2=feret_orth(h.table)[k], area=area, hull_area=hull_area, solidity=area / hull_area)
    if mpp is not None:
        mm = step * float(mpp) / 1000.0
        out.update(d1_mm=out['d1'] * mm, d2_mm=out['d2'] * mm, area_mm2=area * mm * mm)
    return out
