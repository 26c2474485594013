"""Class maps traced into annotation polygons on the device: the way back from a u8 label map (predict_wsis' classes, a tumour bed) to
what ImageScope shows beside the pathologist's own annotations and what `Dataset_wsis(annotations=...)` reads.

The tracing rule is this project's own (spec: tests/contours_oracle.py; the reference has no such code and cv2 / skimage are absent, so
parity is unpinned): the boundary between a traced label and anything else is walked with the label's pixels as 4-connected foreground,
which makes the loops of all labels nested or disjoint, never crossing.  It is pinned by an exact round trip: for steps >= 2,
`annotations.rasterize(*c.paint_list(), (W, H), step, origin)` is `where(traced[m], m, 0)` byte for byte (at step 1 it is not: the
rasteriser covers closed edges, so crack polygons gain a column and a row).  The kernels (wsi_contour_*, csrc/contour.hip) find and
order the loops by pointer doubling over the edges' successor permutation; all of it is integer and bit-reproducible.  There is no CPU
fallback."""
from xml.sax.saxutils import quoteattr

import numpy as np
import torch

from . import native
from .engine import _ptr, _require_gpu
from .maps import check_map, stage_marker, step2

LIMIT = 1 << 29                          # csrc/contour_dev.h wsi_contour::LIMIT
MAX_PIXELS = 1 << 28                     # wsi_contour::MAX_PIXELS: the 4 H W edge slots fit 30 bits
DEFAULT_NAMES = {1: 'Benign', 2: 'In situ', 3: 'Invasive'}     # what annotations.read_imagescope maps back to 1 / 2 / 3


def traced_table(classes=None):
    """the 256-entry u8 table of traced labels: 1..255 by default, else the labels given (0 is allowed)"""
    t = np.zeros(256, np.uint8)
    if classes is None:
        t[1:] = 1
        return t
    for c in classes:
        if isinstance(c, (float, np.floating)) and int(c) != c or not 0 <= int(c) <= 255:
            raise ValueError('class %r is not a label in 0..255' % (c,))
        t[int(c)] = 1
    return t


def level0_corner(c, origin, step, bound=None):
    """map corner -> level-0 coordinate along one axis (Python ints)"""
    v = int(origin) + int(c) * int(step) - int(step) // 2
    return v if bound is None else min(max(v, 0), int(bound) - 1)


class Contours:
    """The loops of a traced map.  vertices (V, 2) int32 in level-0 coordinates, loop after loop; per loop `first` vertex, vertex `count`,
    `edges` (unit edges of the map), `label` (int32) and `area2` (int64, twice the signed area in map pixels: positive for an outer
    loop, negative for a hole).  Loops are listed by their smallest edge key (top-most, then left-most start corner)."""

    def __init__(self, vertices, first, count, edges, label, area2, size, step, origin=(0, 0), bounds=None):
        self.vertices, self.first, self.count, self.edges, self.label, self.area2 = vertices, first, count, edges, label, area2
        self.size, self.step, self.origin, self.bounds = (int(size[0]), int(size[1])), step2(step), (int(origin[0]), int(origin[1])), bounds
        self._cache = None

    def __len__(self):
        return int(self.first.shape[0])

    def _host(self):
        """vertices, first, count, label, area2 as host arrays, copied once"""
        if self._cache is None:
            self._cache = [np.asarray(torch.as_tensor(t).cpu().numpy()) for t in (self.vertices, self.first, self.count, self.label, self.area2)]
        return self._cache

    def loops(self):
        """host: [(k, 2) int64 arrays], in list order"""
        v, first, count = self._host()[:3]
        v = v.astype(np.int64).reshape(-1, 2)
        return [v[f:f + c] for f, c in zip(first.tolist(), count.tolist())]

    def paint_order(self):
        """loop indices by |area2| descending, holes before outer loops on a tie, then list order: every loop comes after its container"""
        a = self._host()[4].tolist()
        return sorted(range(len(a)), key=lambda k: (-abs(a[k]), a[k] > 0, k))

    def paint_list(self):
        """host: (coords, labels) in painter's order with holes as label 0: annotations.rasterize(coords, labels, size, step, origin)
        gives the traced labels of the map back (steps >= 2)"""
        loops, (label, area2) = self.loops(), self._host()[3:]
        order = self.paint_order()
        return [loops[k] for k in order], [int(label[k]) if int(area2[k]) > 0 else 0 for k in order]


def _check_geometry(w, h, sx, sy, ox, oy, bounds):
    if w < 1 or h < 1 or w * h > MAX_PIXELS:
        raise ValueError('a map of %d x %d pixels is outside 1 .. 2^28 pixels' % (w, h))
    if bounds is not None and (int(bounds[0]) < 1 or int(bounds[1]) < 1):
        raise ValueError('bounds %r must be positive' % (bounds,))
    bw, bh = (None, None) if bounds is None else (int(bounds[0]), int(bounds[1]))
    for what, v in (('the origin x', ox), ('the origin y', oy), ('the first x', level0_corner(0, ox, sx, bw)), ('the last x', level0_corner(w, ox, sx, bw)),
                    ('the first y', level0_corner(0, oy, sy, bh)), ('the last y', level0_corner(h, oy, sy, bh))):
        if not -LIMIT <= v <= LIMIT:
            raise ValueError('%s %d is outside [-2^29, 2^29]' % (what, v))


def trace_raw(label_map, table, step, origin=(0, 0), bounds=None, alloc=None, stages=None):
    """The five device stages on a u8 (H, W) GPU tensor -> (vertices (V, 2) int32, loop records (L, 8) int32, area2 (L,) int64, n_edges).
    alloc(n_vertices, n_loops) -> (vertices, records, area2) buffers at least that large (default: exact fresh tensors); the leading
    rows are returned.  stages: a dict that receives, per stage name ('count', 'build', 'ranks', 'order', 'emit'), the [begin, end]
    torch.cuda.Event pair recorded round the stage's entry (tools/contour_times.py)."""
    lib = native.load()
    sx, sy = step2(step)
    ox, oy = int(origin[0]), int(origin[1])
    h, w, pitch = check_map(label_map, 'the label map')
    _check_geometry(w, h, sx, sy, ox, oy, bounds)
    _require_gpu(label_map, 'the label map')
    table = np.ascontiguousarray(table, np.uint8)
    assert table.shape == (256,)
    dev = label_map.device
    bw, bh = (0, 0) if bounds is None else (int(bounds[0]), int(bounds[1]))
    tp = table.ctypes.data_as(native.C.c_void_p)

    mark = stage_marker(stages)

    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        count_ws = torch.empty(lib.wsi_contour_count_workspace_bytes(w, h), dtype=torch.uint8, device=dev)
        n_edges_t = torch.zeros(1, dtype=torch.int32, device=dev)
        mark('count')
        native.check(lib.wsi_contour_count(_ptr(label_map), w, h, pitch, tp, _ptr(count_ws), _ptr(n_edges_t), st), 'wsi_contour_count')
        mark('count')
        n_edges = int(n_edges_t.item())                             # the one number the workspace is sized by
        if n_edges == 0:
            nv = nl = 0
        else:
            ws_bytes = lib.wsi_contour_workspace_bytes(n_edges)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            counts = torch.zeros(2, dtype=torch.int32, device=dev)
            mark('build')
            native.check(lib.wsi_contour_build(_ptr(label_map), w, h, pitch, tp, _ptr(count_ws), n_edges, _ptr(ws), ws_bytes, st), 'wsi_contour_build')
            mark('build')
            mark('ranks')
            native.check(lib.wsi_contour_ranks(_ptr(ws), ws_bytes, n_edges, st), 'wsi_contour_ranks')
            mark('ranks')
            mark('order')
            native.check(lib.wsi_contour_order(_ptr(ws), ws_bytes, n_edges, w, _ptr(counts), st), 'wsi_contour_order')
            mark('order')
            nl, nv = (int(v) for v in counts.tolist())
        if alloc is None:
            vertices = torch.empty((nv, 2), dtype=torch.int32, device=dev)
            records = torch.empty((nl, 8), dtype=torch.int32, device=dev)
            area2 = torch.empty((nl,), dtype=torch.int64, device=dev)
        else:
            vertices, records, area2 = alloc(nv, nl)
            if vertices.shape[0] < nv or records.shape[0] < nl or area2.shape[0] < nl or not (vertices.is_contiguous() and records.is_contiguous()):
                raise ValueError('alloc returned buffers smaller than %d vertices / %d loops' % (nv, nl))
        if n_edges:
            mark('emit')
            native.check(lib.wsi_contour_emit(_ptr(label_map), w, h, pitch, _ptr(ws), ws_bytes, n_edges, ox, oy, sx, sy, bw, bh, _ptr(vertices), nv,
                                              _ptr(records), _ptr(area2), nl, st), 'wsi_contour_emit')
            mark('emit')
    return vertices[:nv], records[:nl], area2[:nl], n_edges


def trace(label_map, classes=None, step=16, origin=(0, 0), bounds=None, min_area=0):
    """Trace a u8 (H, W) CUDA label map (unit column stride, any row stride and alignment) into a `Contours`.
    classes: None traces labels 1..255, an iterable of ints those labels (0 allowed; outside 0..255: ValueError).
    step, origin: map pixel (x, y) samples level-0 point origin + (x, y) * step, so map corner (cx, cy) becomes
    origin + (cx, cy) * step - step // 2; bounds = (W0, H0) clamps to the slide.  The round trip through annotations.rasterize needs
    step >= 2 each way (and, with bounds, (W - 1) sx < W0 <= W sx, likewise y); step 1 traces but does not round-trip.
    min_area=a drops the loops with |area2| < 2 a map pixels; what a dropped loop contains is smaller and goes with it.
    An empty map gives empty tensors and launches nothing after the count."""
    table = traced_table(classes)
    vertices, rec, area2, _ = trace_raw(label_map, table, step, origin, bounds)
    if min_area > 0 and len(area2):
        keep = area2.abs() >= 2 * min_area
        idx = torch.nonzero(keep)[:, 0]
        cnt = rec[idx, 1].to(torch.int64)
        new_first = torch.cumsum(cnt, 0) - cnt
        src = torch.repeat_interleave(rec[idx, 0].to(torch.int64) - new_first, cnt) + torch.arange(int(cnt.sum()), device=rec.device)
        vertices, rec, area2 = vertices[src], rec[idx].clone(), area2[idx]
        rec[:, 0] = new_first.to(torch.int32)
    h, w = label_map.shape
    return Contours(vertices, rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], area2, (w, h), step, origin, bounds)


# ---------------------------------------------------------------------------------------------------------------------- the writer
def _regions(c, mpp, names, holes, first_id):
    """the Region elements of one layer as text, in painter's order: one format per region, no Python per vertex"""
    v, first, count, label, area2 = c._host()
    v = v.astype(np.int64).reshape(-1, 2)
    sx, sy = c.step
    # the rectilinear perimeter of every loop at once: |v - next(v)| summed per loop, next wrapping to the loop's first vertex
    if len(first):
        nxt = np.arange(1, len(v) + 1)
        nxt[first + count - 1] = first
        length = np.add.reduceat(np.abs(v - v[nxt]).sum(1), first)
    quoted = {l: quoteattr(str(n)) for l, n in names.items()}
    out, rid = [], first_id
    for k in c.paint_order():
        hole = int(area2[k]) < 0
        if hole and holes == 'drop':
            continue
        f, n, name = int(first[k]), int(count[k]), quoted[int(label[k])]
        out.append('<Region Id="%d" Type="1" Text=%s NegativeROA="%d" AreaMicrons="%.4f" LengthMicrons="%.4f"><Attributes><Attribute Id="0" Name="" Value=%s />'
                   '</Attributes><Vertices>' % (rid, name, hole, abs(int(area2[k])) / 2.0 * sx * sy * mpp * mpp, float(length[k]) * mpp, name)
                   + '<Vertex X="%d" Y="%d" Z="0" />' * n % tuple(v[f:f + n].ravel().tolist()) + '</Vertices></Region>\n')
        rid += 1
    return ''.join(out), rid


def write_imagescope(path, c, mpp=1.0, names=None, holes='negative', layers=()):
    """Write the loops of `c` as Aperio ImageScope XML, the structure annotations.read_imagescope and the reference's reader walk:
    Annotations(MicronsPerPixel) / Annotation / [Attributes, Regions] / Region(Id, Text, NegativeROA, AreaMicrons, LengthMicrons) /
    [Attributes / Attribute(Value=name), Vertices / Vertex(X, Y, Z="0")].  Regions go in painter's order (largest first), so a reader
    that paints in file order restores the map.  AreaMicrons = |area2| / 2 * sx * sy * mpp^2; LengthMicrons = the rectilinear perimeter
    of the level-0 vertices * mpp.  names: {label: name} (default 1 Benign, 2 In situ, 3 Invasive); a label of `c` without a name raises
    ValueError before anything is written.  holes: 'negative' writes a hole as a region with NegativeROA="1" and the enclosing label's
    name (ImageScope subtracts it; read_imagescope(negative='erase') gives it label 0), 'drop' leaves holes out.
    layers: further (contours, names) pairs, each an Annotation element of its own after the first (readers take root[0] only)."""
    if holes not in ('negative', 'drop'):
        raise ValueError("holes must be 'negative' or 'drop', not %r" % (holes,))
    mpp = float(mpp)
    if not mpp > 0:
        raise ValueError('mpp %r must be positive' % (mpp,))
    all_layers = [(c, DEFAULT_NAMES if names is None else names)] + [(lc, DEFAULT_NAMES if ln is None else ln) for lc, ln in layers]
    for lc, ln in all_layers:
        for l in sorted(set(lc._host()[3].tolist())):
            if l not in ln:
                raise ValueError('label %d is traced but has no name' % l)
    parts = ['<?xml version="1.0" encoding="utf-8"?>\n<Annotations MicronsPerPixel="%.6f">\n' % mpp]
    rid = 1
    for k, (lc, ln) in enumerate(all_layers):
        text, rid = _regions(lc, mpp, ln, holes, rid)
        parts.append('<Annotation Id="%d" Name="" ReadOnly="0" Type="4" Visible="1" LineColor="65280"><Attributes />\n<Regions>\n%s</Regions></Annotation>\n'
                     % (k + 1, text))
    parts.append('</Annotations>\n')
    with open(path, 'w', encoding='utf-8') as f:
        f.write(''.join(parts))
    return path


def stated_mpp(scan):
    """microns per pixel of level 0 where the slide states it (`scan.mpp`, or openslide's `properties['openslide.mpp-x']`), else None"""
    v = getattr(scan, 'mpp', None)
    if v is None:
        v = (getattr(scan, 'properties', None) or {}).get('openslide.mpp-x')
    try:
        v = float(v)
    except (TypeError, ValueError):
        return None
    return v if v > 0 else None


def slide_mpp(scan):
    """stated_mpp, or 1.0 where the slide states none"""
    v = stated_mpp(scan)
    return 1.0 if v is None else v
