"""The boundary tracing rule of wsi_segmentation_pipeline_amd/contours.py (csrc/contour_dev.h, csrc/contour.hip), written once in NumPy
and Python ints: the spec the host program and the device kernels are compared with, byte for byte.  It is this project's own rule
(the reference has no such code; cv2 and skimage are absent), pinned by an exact round trip through tests/annotations_oracle.py.

  input     a u8 label map m of H rows x W columns and a 256-entry table of traced labels.  A pixel outside the map has no label and
            differs from every label.
  edges     pixel (x, y) is the corner square (x, y) - (x + 1, y + 1), x right, y down.  Side d of a pixel: 0 top (heading east), 1
            right (south), 2 bottom (west), 3 left (north).  Side d of P is a boundary edge iff m[P] is traced and the pixel across that
            side has another label: a crack between two traced labels is an edge of both, in opposite directions.
  successor for edge (P, d) let F be the pixel ahead of P in the heading of d and A the pixel across side d of F.  F differs from P: turn
            right, (P, d + 1).  Else A differs: straight, (F, d).  Else turn left, (A, d - 1).  F is tested first (4-connected
            foreground), so at a saddle the walk stays on its own pixel and the loops of all labels are a laminar family.
  order     an edge's key is (ty (W + 1) + tx) 4 + d with (tx, ty) its tail corner; a loop starts at the tail of its smallest-key edge
            (always a turn) and loops are listed by that key, ascending.
  vertices  the tails of the edges whose predecessor has another heading, in traversal order from the start.
  per loop  label of P; area2 = sum x_i y_(i+1) - x_(i+1) y_i over the vertices in map-corner coordinates (positive: outer loop,
            negative: hole); edge count; vertex count.
  level 0   corner (cx, cy) -> (ox + cx sx - sx // 2, oy + cy sy - sy // 2), then with bounds = (W0, H0) clamped to [0, W0 - 1] x [0, H0 - 1].
  painter   loops by |area2| descending, on a tie holes before outer loops, then list order; an outer loop paints its label, a hole 0.
  guarantee for steps >= 2 each way, annotations_oracle.rasterize(paint-order coordinates, labels, (W, H), step, origin) equals
            where(traced[m], m, 0); with bounds whenever (W - 1) sx < W0 <= W sx, and likewise for y.  Not at step 1.
  limits    1 <= W, H; H W <= 2^28; every produced coordinate in [-2^29, 2^29]; steps >= 1."""
import numpy as np

LIMIT = 1 << 29
MAX_PIXELS = 1 << 28
DX, DY = (1, 0, -1, 0), (0, 1, 0, -1)                           # heading of side d


def traced_table(classes=None):
    """the 256-entry bool table: labels 1..255 by default, else the given labels (0 allowed; outside 0..255: ValueError)"""
    t = np.zeros(256, bool)
    if classes is None:
        t[1:] = True
        return t
    for c in classes:
        if int(c) != c or not 0 <= int(c) <= 255:
            raise ValueError('class %r is not a label in 0..255' % (c,))
        t[int(c)] = True
    return t


def _step2(step):
    sx, sy = (int(step), int(step)) if np.isscalar(step) else (int(step[0]), int(step[1]))
    if sx < 1 or sy < 1:
        raise ValueError('step %r must be >= 1' % (step,))
    return sx, sy


def quads(m):
    """(H + 1, W + 1, 4) int16: the labels round every corner in the order NW, SW, SE, NE (-1 outside the map)"""
    h, w = m.shape
    p = np.full((h + 2, w + 2), -1, np.int16)
    p[1:-1, 1:-1] = m
    return np.stack((p[:-1, :-1], p[1:, :-1], p[1:, 1:], p[:-1, 1:]), -1)


def edges_and_successors(m, traced):
    """(keys ascending, succ as indices into keys, vertex flags): the boundary edges of the map as one permutation"""
    h, w = m.shape
    q = quads(m)
    out = np.zeros((h + 1, w + 1, 4), bool)
    for d in range(4):
        px, ac = q[..., (2 - d) & 3], q[..., (3 - d) & 3]       # the edge's pixel and the pixel across, seen from the tail corner
        out[..., d] = (px >= 0) & traced[np.maximum(px, 0)] & (ac != px)
    keys = np.flatnonzero(out.ravel()).astype(np.int64)
    ci, d = keys >> 2, keys & 3
    head = ci + np.array([1, w + 1, -1, -(w + 1)], np.int64)[d]
    qt, qh = q.reshape(-1, 4)[ci], q.reshape(-1, 4)[head]
    rows = np.arange(len(keys))
    P, F, A = qh[rows, (1 - d) & 3], qh[rows, (2 - d) & 3], qh[rows, (3 - d) & 3]
    d2 = np.where(F != P, (d + 1) & 3, np.where(A != P, d, (d + 3) & 3))
    succ = np.searchsorted(keys, head * 4 + d2)
    assert np.array_equal(keys[succ], head * 4 + d2)             # a successor is a boundary edge,
    assert np.array_equal(np.sort(succ), rows)                   # and the successor map a permutation
    own = qt[rows, (2 - d) & 3]
    vertex = ~((qt[rows, (1 - d) & 3] == own) & (qt[rows, (0 - d) & 3] != own))      # the straight predecessor is missing
    return keys, succ, vertex


class Traced:
    """what trace returns: vertices (V, 2) int32 in level-0 coordinates; per loop first, count (vertices), edges, label (int32) and area2 (int64)"""

    def __init__(self, vertices, first, count, edges, label, area2, size, step, origin, bounds):
        self.vertices, self.first, self.count, self.edges, self.label, self.area2 = vertices, first, count, edges, label, area2
        self.size, self.step, self.origin, self.bounds = size, step, origin, bounds

    def loops(self):
        return [self.vertices[f:f + c].astype(np.int64) for f, c in zip(self.first, self.count)]

    def records(self):
        """the 32-byte loop records of the device: first vertex, vertex count, edge count, label, 0, 0, 0, 0"""
        r = np.zeros((len(self.first), 8), np.int32)
        r[:, 0], r[:, 1], r[:, 2], r[:, 3] = self.first, self.count, self.edges, self.label
        return r

    def paint_list(self):
        return paint_list(self.loops(), self.label, self.area2)


def to_level0(corners, step, origin, bounds=None):
    sx, sy = _step2(step)
    c = np.asarray(corners, np.int64).reshape(-1, 2)
    out = np.stack((int(origin[0]) + c[:, 0] * sx - sx // 2, int(origin[1]) + c[:, 1] * sy - sy // 2), 1)
    if bounds is not None:
        out[:, 0] = np.clip(out[:, 0], 0, int(bounds[0]) - 1)
        out[:, 1] = np.clip(out[:, 1], 0, int(bounds[1]) - 1)
    return out


def trace(m, classes=None, step=16, origin=(0, 0), bounds=None, min_area=0):
    m = np.asarray(m)
    if m.ndim != 2 or m.dtype != np.uint8:
        raise ValueError('the label map must be a 2-D uint8 array')
    h, w = m.shape
    if h < 1 or w < 1 or h * w > MAX_PIXELS:
        raise ValueError('a map of %d x %d pixels is outside 1 .. 2^28 pixels' % (w, h))
    sx, sy = _step2(step)
    traced = traced_table(classes)
    if bounds is not None and (int(bounds[0]) < 1 or int(bounds[1]) < 1):
        raise ValueError('bounds %r must be positive' % (bounds,))
    for v in [int(origin[0]), int(origin[1])] + to_level0([(0, 0), (w, h)], step, origin, bounds).ravel().tolist():
        if not -LIMIT <= int(v) <= LIMIT:
            raise ValueError('the coordinate %d is outside [-2^29, 2^29]' % int(v))
    keys, succ, vertex = edges_and_successors(m, traced)
    keys_l, succ_l, vertex_l = keys.tolist(), succ.tolist(), vertex.tolist()
    seen = np.zeros(len(keys), bool)
    verts, first, count, edges, label, area2 = [], [], [], [], [], []
    for e0 in range(len(keys_l)):                               # ascending keys: the first unseen edge of a loop is its smallest
        if seen[e0]:
            continue
        assert vertex_l[e0]                                     # the start is a turn
        loop, e, n = [], e0, 0
        while True:
            seen[e] = True
            n += 1
            if vertex_l[e]:
                c = keys_l[e] >> 2
                loop.append((c % (w + 1), c // (w + 1)))
            e = succ_l[e]
            if e == e0:
                break
        a2 = sum(loop[i][0] * loop[(i + 1) % len(loop)][1] - loop[(i + 1) % len(loop)][0] * loop[i][1] for i in range(len(loop)))
        if abs(a2) < 2 * min_area:
            continue
        c, d = keys_l[e0] >> 2, keys_l[e0] & 3
        tx, ty = c % (w + 1), c // (w + 1)
        first.append(len(verts))
        count.append(len(loop))
        edges.append(n)
        label.append(int(m[ty - (d >= 2), tx - (d in (1, 2))]))
        area2.append(a2)
        verts.extend(loop)
    v0 = to_level0(verts, step, origin, bounds).astype(np.int32)
    i32 = lambda a: np.asarray(a, np.int32).reshape(-1)
    return Traced(v0, i32(first), i32(count), i32(edges), i32(label), np.asarray(area2, np.int64).reshape(-1), (w, h), (sx, sy),
                  (int(origin[0]), int(origin[1])), bounds)


def paint_order(area2):
    """indices of the loops in painter's order: |area2| descending, holes before outer loops on a tie, then list order"""
    a = [int(v) for v in area2]
    return sorted(range(len(a)), key=lambda k: (-abs(a[k]), a[k] > 0, k))


def paint_list(loops, label, area2):
    order = paint_order(area2)
    return [loops[k] for k in order], [int(label[k]) if int(area2[k]) > 0 else 0 for k in order]
