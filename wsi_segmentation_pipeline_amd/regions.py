"""Region tables on the device: a u8 class map labelled into connected regions and every region measured in one pass - how many lesions
a slide holds, how large each is, of which class, and where.

The rule is this project's own (spec: tests/regions_oracle.py; parity unpinned).  A run is a maximal stretch of equal bytes in one row
whose class is traced; two runs of one class in neighbouring rows are joined iff they touch (connectivity 4: share a pixel side; 8: a
side or a corner); a region is a class of the closure, numbered 1 .. n in raster order of its first pixel.  The kernels (wsi_region_*,
csrc/regions.hip) work on runs, not pixels, and every sum is a closed form per run in integers, so the table is the same bytes every
run.  There is no CPU fallback."""
import csv
import math
from fractions import Fraction

import numpy as np
import torch

from . import native
from .contours import traced_table
from .engine import _ptr, _require_gpu
from .maps import as_u8, check_map, check_out_i32, stage_marker, step2, take_workspace

LIMIT = 32768                            # csrc/regions_dev.h wsi_region::LIMIT
FIELDS = ('area', 'x0', 'y0', 'x1', 'y1', 'sx', 'sy', 'sxx', 'sxy', 'syy', 'perim', 'wsum', 'first', 'cls', 'border', 'reserved')
_F = {name: k for k, name in enumerate(FIELDS)}
STAGES = ('count', 'runs', 'link', 'rank', 'table', 'paint')


class Regions:
    """n regions; table (n, 16) int64 on the map's device, one row per region in FIELDS order; labels (H, W) int32 or None."""

    def __init__(self, table, labels, size, n_runs=0, hulls=None):
        self.table, self.labels, self.size, self.n_runs = table, labels, (int(size[0]), int(size[1])), int(n_runs)
        self.n = int(table.shape[0])
        self.hulls = hulls                                      # a `Hulls` where label(..., hulls=True) made them
        self._host_table = None

    def __len__(self):
        return self.n

    area = property(lambda self: self.table[:, _F['area']])
    cls = property(lambda self: self.table[:, _F['cls']])
    box = property(lambda self: self.table[:, _F['x0']:_F['y1'] + 1])
    perim = property(lambda self: self.table[:, _F['perim']])
    wsum = property(lambda self: self.table[:, _F['wsum']])
    border = property(lambda self: self.table[:, _F['border']])
    first = property(lambda self: self.table[:, _F['first']])

    def host(self):
        """the table as a host int64 array, copied once"""
        if self._host_table is None:
            self._host_table = np.asarray(torch.as_tensor(self.table).cpu().numpy(), np.int64).reshape(-1, 16)
        return self._host_table

    def centroid(self):
        """(n, 2) float64 (cx, cy) = (sx / area, sy / area), on the host"""
        t = self.host()
        a = t[:, _F['area']].astype(np.float64)
        return np.stack([t[:, _F['sx']] / a, t[:, _F['sy']] / a], 1)

    def axes(self):
        """major, minor, orientation (radians, the major axis against x) from the central second moments per pixel, 1 / 12 added for the
        pixel's own extent: the eigenvalues l of the inertia tensor give axis lengths 4 sqrt(l).  float64 on the host."""
        t = self.host()
        a = t[:, _F['area']].astype(np.float64)
        cx, cy = t[:, _F['sx']] / a, t[:, _F['sy']] / a
        mxx = t[:, _F['sxx']] / a - cx * cx + 1.0 / 12
        myy = t[:, _F['syy']] / a - cy * cy + 1.0 / 12
        mxy = t[:, _F['sxy']] / a - cx * cy
        half, diff = (mxx + myy) / 2, np.sqrt(((mxx - myy) / 2) ** 2 + mxy * mxy)
        return 4 * np.sqrt(np.maximum(half + diff, 0)), 4 * np.sqrt(np.maximum(half - diff, 0)), 0.5 * np.arctan2(2 * mxy, mxx - myy)

    def rows(self, step=1, origin=(0, 0), mpp=None, hulls=False):
        """one dict per region: id, class, area_px (map pixels), area_um2 (None without mpp; a map pixel is step x step level-0 pixels
        of mpp microns), the box and the centroid in level-0 coordinates (map pixel x covers origin + x step .. origin + (x + 1) step,
        its centre is origin + (x + 0.5) step), perim (pixel sides), major, minor (map pixels), mean_weight (wsum / area).
        hulls: also HULL_COLUMNS from self.hulls - feret_max, feret_min, feret_orth (map pixels), their *_um (length x step x mpp; None
        without mpp or where the step differs between x and y), solidity, hull_area_px"""
        sx, sy = step2(step)
        ox, oy = int(origin[0]), int(origin[1])
        t, c = self.host(), self.centroid()
        major, minor, _ = self.axes()
        out = []
        for k in range(self.n):
            area = int(t[k, _F['area']])
            out.append({
                'id': k + 1, 'class': int(t[k, _F['cls']]), 'area_px': area,
                'area_um2': None if mpp is None else area * sx * sy * float(mpp) * float(mpp),
                'x0': ox + int(t[k, _F['x0']]) * sx, 'y0': oy + int(t[k, _F['y0']]) * sy,
                'x1': ox + int(t[k, _F['x1']]) * sx, 'y1': oy + int(t[k, _F['y1']]) * sy,
                'cx': ox + (float(c[k, 0]) + 0.5) * sx, 'cy': oy + (float(c[k, 1]) + 0.5) * sy,
                'perim': int(t[k, _F['perim']]), 'major': float(major[k]), 'minor': float(minor[k]),
                'mean_weight': int(t[k, _F['wsum']]) / area,
            })
        if hulls:
            if self.hulls is None:
                raise ValueError('these regions were labelled without hulls=True')
            h = self.hulls
            um = None if mpp is None or sx != sy else sx * float(mpp)
            fmax, fmin, forth, harea = h.feret_max(), h.feret_min(), h.feret_orth(), h.hull_area()
            solidity = h.solidity(t[:, _F['area']])
            for k, row in enumerate(out):
                row.update(feret_max=float(fmax[k]), feret_min=float(fmin[k]), feret_orth=float(forth[k]),
                           feret_max_um=None if um is None else float(fmax[k]) * um, feret_min_um=None if um is None else float(fmin[k]) * um,
                           feret_orth_um=None if um is None else float(forth[k]) * um, solidity=float(solidity[k]), hull_area_px=float(harea[k]))
        return out


CSV_COLUMNS = ('id', 'class', 'name', 'area_px', 'area_um2', 'x0', 'y0', 'x1', 'y1', 'cx', 'cy', 'perim', 'major', 'minor', 'mean_weight')


HULL_COLUMNS = ('feret_max', 'feret_min', 'feret_orth', 'feret_max_um', 'feret_min_um', 'feret_orth_um', 'solidity', 'hull_area_px')


def write_csv(path, r, step=1, origin=(0, 0), mpp=None, names=None, hulls=False):
    """the rows of `r` as CSV, one line per region under CSV_COLUMNS; names: {class: name} (a class without one gets ''); area_um2 is
    empty where mpp is None.  hulls: HULL_COLUMNS follow CSV_COLUMNS."""
    names = names or {}
    columns = CSV_COLUMNS + HULL_COLUMNS if hulls else CSV_COLUMNS
    with open(path, 'w', newline='', encoding='utf-8') as f:
        w = csv.writer(f)
        w.writerow(columns)
        for row in (r.rows(step, origin, mpp, hulls=True) if hulls else r.rows(step, origin, mpp)):
            row['name'] = names.get(row['class'], '')
            w.writerow(['' if row[c] is None else ('%.4f' % row[c] if isinstance(row[c], float) else row[c]) for c in columns])
    return path


# ------------------------------------------------------------------------------------------------------------------------- hulls
HULL_FIELDS = ('hull_first', 'hull_n', 'hull_area2', 'feret_sq', 'feret_a', 'feret_b', 'width_num', 'width_den', 'width_edge', 'width_vertex', 'orth_num')
_H = {name: k for k, name in enumerate(HULL_FIELDS)}
HULL_STAGES = ('hull_rows', 'hull_chains', 'hull_emit', 'hull_measure')


class Hulls:
    """The convex hull of every region (spec: tests/region_hulls_oracle.py; kernels: wsi_regionhull_*, csrc/region_hulls.hip).  table
    (n, 16) int64 on the map's device, one row per region in HULL_FIELDS order and five zero words; vertices (V, 2) int32 (x, y) in map
    corner coordinates - pixel (x, y) is the square (x, y) .. (x + 1, y + 1) - region k's at hull_first[k] : hull_first[k] + hull_n[k],
    strictly convex, from the smallest (y, x), clockwise as seen with y pointing down."""

    def __init__(self, table, vertices):
        self.table, self.vertices = table, vertices
        self.n = int(table.shape[0])
        self._host_table = self._host_vertices = None

    def __len__(self):
        return self.n

    hull_first = property(lambda self: self.table[:, _H['hull_first']])
    hull_n = property(lambda self: self.table[:, _H['hull_n']])
    hull_area2 = property(lambda self: self.table[:, _H['hull_area2']])
    feret_sq = property(lambda self: self.table[:, _H['feret_sq']])
    feret_pair = property(lambda self: self.table[:, _H['feret_a']:_H['feret_b'] + 1])
    width = property(lambda self: self.table[:, _H['width_num']:_H['width_den'] + 1])
    orth_num = property(lambda self: self.table[:, _H['orth_num']])

    def host(self):
        """the table as a host int64 array, copied once"""
        if self._host_table is None:
            self._host_table = np.asarray(torch.as_tensor(self.table).cpu().numpy(), np.int64).reshape(-1, 16)
        return self._host_table

    def host_vertices(self):
        if self._host_vertices is None:
            self._host_vertices = np.asarray(torch.as_tensor(self.vertices).cpu().numpy(), np.int32).reshape(-1, 2)
        return self._host_vertices

    def polygons(self, step=1, origin=(0, 0)):
        """[(hull_n, 2) int64 arrays] in level-0 coordinates: corner (cx, cy) becomes origin + (cx sx, cy sy), the true corner of the
        pixel's footprint, as `Regions.rows` places the box (contours.trace shifts its vertices by half a step; these are not shifted)"""
        sx, sy = step2(step)
        t, v = self.host(), self.host_vertices().astype(np.int64)
        v = v * np.asarray([sx, sy], np.int64) + np.asarray([int(origin[0]), int(origin[1])], np.int64)
        return [v[int(f):int(f) + int(n)] for f, n in zip(t[:, _H['hull_first']], t[:, _H['hull_n']])]

    def _col(self, name):
        return self.host()[:, _H[name]].astype(np.float64)       # every word is below 2^61; float64 is only the last step

    def feret_max(self):
        """the largest distance between two points of the region, sqrt(feret_sq), map pixels"""
        return np.sqrt(self._col('feret_sq'))

    def feret_min(self):
        """the least caliper width, sqrt(width_num / width_den)"""
        return np.sqrt(self._col('width_num') / self._col('width_den'))

    def feret_orth(self):
        """the extent at right angles to the longest diameter, orth_num / sqrt(feret_sq)"""
        return self._col('orth_num') / np.sqrt(self._col('feret_sq'))

    def feret_angle(self):
        """radians of the longest diameter a -> b against x"""
        t, v = self.host(), self.host_vertices().astype(np.int64)
        d = v[t[:, _H['hull_first']] + t[:, _H['feret_b']]] - v[t[:, _H['hull_first']] + t[:, _H['feret_a']]]
        return np.arctan2(d[:, 1].astype(np.float64), d[:, 0].astype(np.float64)).reshape(-1)

    def hull_area(self):
        return self._col('hull_area2') / 2

    def solidity(self, area):
        """area / hull_area, at most 1; area: the regions' areas (Regions.area or its host copy)"""
        a = np.asarray(torch.as_tensor(area).cpu().numpy() if isinstance(area, torch.Tensor) else area, np.float64).reshape(-1)
        return a / self.hull_area()

    def hull_perimeter(self):
        """the edge lengths summed in vertex order, float64"""
        out = np.zeros(self.n, np.float64)
        for k, p in enumerate(self.polygons()):
            total = 0.0
            for e in (np.roll(p, -1, 0) - p).tolist():
                total += math.sqrt(e[0] * e[0] + e[1] * e[1])
            out[k] = total
        return out


def _hulls(lib, region_ws, region_ws_bytes, tab, w, h, n_runs, n, dev, st, mark):
    """the hull stages on a workspace of their own; one synchronisation: the vertex count sizes `vertices`"""
    need = lib.wsi_regionhull_workspace_bytes(w, h, n_runs, n)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    mark('hull_rows')
    native.check(lib.wsi_regionhull_rows(_ptr(region_ws), region_ws_bytes, _ptr(tab), w, h, n_runs, n, _ptr(ws), need, st), 'wsi_regionhull_rows')
    mark('hull_rows')
    mark('hull_chains')
    native.check(lib.wsi_regionhull_chains(_ptr(ws), need, w, h, n_runs, n, _ptr(counts), st), 'wsi_regionhull_chains')
    mark('hull_chains')
    total, status = (int(v) for v in counts.tolist())             # the one synchronisation the hulls add
    if status != 0 or not 4 * n <= total <= 2 * (n_runs + n):
        raise RuntimeError('wsi_regionhull_chains: status %d, %d vertices for %d regions of %d runs' % (status, total, n, n_runs))
    vertices = torch.empty((total, 2), dtype=torch.int32, device=dev)
    table = torch.empty((n, 16), dtype=torch.int64, device=dev)
    mark('hull_emit')
    native.check(lib.wsi_regionhull_emit(_ptr(ws), need, _ptr(tab), w, h, n_runs, n, total, _ptr(vertices), st), 'wsi_regionhull_emit')
    mark('hull_emit')
    mark('hull_measure')
    native.check(lib.wsi_regionhull_measure(_ptr(ws), need, w, h, n_runs, n, _ptr(vertices), total, _ptr(table), st), 'wsi_regionhull_measure')
    mark('hull_measure')
    return Hulls(table, vertices)


def label(m, classes=None, connectivity=8, labels=True, weight=None, out=None, workspace=None, stages=None, hulls=False):
    """Label a u8 (H, W) CUDA class map (unit column stride, any row stride and alignment) -> `Regions`.
    classes: None takes labels 1..255, an iterable of ints those labels (0 allowed).  connectivity: 4 or 8.  labels: also paint the
    (H, W) int32 label map (into `out` where given: int32, unit column stride, any row stride).  weight: a u8 map of the same shape
    whose sum per region goes into `wsum`.  workspace: a u8 tensor at least wsi_region_workspace_bytes large to work in.
    Two synchronisations: the run count sizes the workspace, the region count sizes the table.  A map without a traced pixel launches
    nothing after the count.  stages: a dict that receives, per name of STAGES, the [begin, end] torch.cuda.Event pair of the stage.
    hulls: also the convex hull and the Feret diameters of every region, as `Regions.hulls` (a `Hulls`); one more synchronisation - the
    vertex count sizes the vertex list - and the stages HULL_STAGES."""
    lib = native.load()
    if connectivity not in (4, 8):
        raise ValueError('connectivity %r is neither 4 nor 8' % (connectivity,))
    table = np.ascontiguousarray(traced_table(classes), np.uint8)
    h, w, pitch = check_map(m, 'the class map', LIMIT)
    _require_gpu(m, 'the class map')
    if weight is not None:
        if tuple(weight.shape) != (h, w):
            raise ValueError('the weight map must have the shape of the class map')
        wpitch = check_map(weight, 'the weight map', LIMIT)[2]
        _require_gpu(weight, 'the weight map')
    dev = m.device
    if out is not None:
        check_out_i32(out, h, w, dev)
    tp = table.ctypes.data_as(native.C.c_void_p)
    mark = stage_marker(stages)

    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        count_ws = torch.empty(lib.wsi_region_count_workspace_bytes(w, h), dtype=torch.uint8, device=dev)
        n_runs_t = torch.zeros(1, dtype=torch.int32, device=dev)
        mark('count')
        native.check(lib.wsi_region_count(_ptr(m), w, h, pitch, tp, _ptr(count_ws), _ptr(n_runs_t), st), 'wsi_region_count')
        mark('count')
        n_runs = int(n_runs_t.item())                               # the first synchronisation: the workspace is sized by it
        if n_runs == 0:
            lab = None
            if labels:
                lab = torch.zeros((h, w), dtype=torch.int32, device=dev) if out is None else out.zero_()
            empty = Hulls(torch.zeros((0, 16), dtype=torch.int64, device=dev), torch.zeros((0, 2), dtype=torch.int32, device=dev)) if hulls else None
            return Regions(torch.zeros((0, 16), dtype=torch.int64, device=dev), lab, (w, h), hulls=empty)
        workspace = take_workspace(workspace, lib.wsi_region_workspace_bytes(w, h, n_runs), dev)
        ws_bytes = int(workspace.numel())
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        mark('runs')
        native.check(lib.wsi_region_runs(_ptr(m), w, h, pitch, tp, _ptr(count_ws), n_runs, _ptr(workspace), ws_bytes, st), 'wsi_region_runs')
        mark('runs')
        mark('link')
        native.check(lib.wsi_region_link(_ptr(workspace), ws_bytes, w, h, n_runs, connectivity, st), 'wsi_region_link')
        mark('link')
        mark('rank')
        native.check(lib.wsi_region_rank(_ptr(workspace), ws_bytes, w, h, n_runs, connectivity, _ptr(counts), st), 'wsi_region_rank')
        mark('rank')
        n, status = (int(v) for v in counts.tolist())               # the second and last synchronisation
        if status != 0 or not 1 <= n <= n_runs:
            raise RuntimeError('wsi_region_rank: %d joined pairs of runs ended in different regions (%d regions of %d runs)' % (status, n, n_runs))
        tab = torch.empty((n, 16), dtype=torch.int64, device=dev)
        mark('table')
        native.check(lib.wsi_region_table(_ptr(workspace), ws_bytes, w, h, n_runs, n, _ptr(weight) if weight is not None else None,
                                          wpitch if weight is not None else 0, _ptr(tab), st), 'wsi_region_table')
        mark('table')
        lab = None
        if labels:
            lab = torch.empty((h, w), dtype=torch.int32, device=dev) if out is None else out
            mark('paint')
            native.check(lib.wsi_region_paint(_ptr(workspace), ws_bytes, w, h, n_runs, _ptr(lab), 4 * (lab.stride(0) if h > 1 else w), st),
                         'wsi_region_paint')
            mark('paint')
        made = _hulls(lib, workspace, ws_bytes, tab, w, h, n_runs, n, dev, st, mark) if hulls else None
    return Regions(tab, lab, (w, h), n_runs, made)


# ------------------------------------------------------------------------------------------------------------- what follows from it
def remove_small(m, min_area, connectivity=8, classes=None, fill=0):
    """area opening of a class map: the regions of fewer than min_area pixels become `fill`; everything else is kept"""
    m = as_u8(m, 'the class map')
    r = label(m, classes, connectivity, labels=True)
    if r.n == 0:
        return m.clone()
    small = torch.cat([torch.zeros(1, dtype=torch.bool, device=m.device), r.area.to(m.device) < int(min_area)])
    return torch.where(small[r.labels.long()], torch.full_like(m, int(fill)), m)


def overlaps(a, b):
    """(K, 3) int64 (id_a, id_b, pixels) of two label maps (or `Regions` with labels) of one shape, over the pixels where both are set,
    sorted by id_a, then id_b"""
    la, lb = (x.labels if isinstance(x, Regions) else x for x in (a, b))
    if la is None or lb is None or tuple(la.shape) != tuple(lb.shape):
        raise ValueError('overlaps needs two label maps of one shape')
    both = (la > 0) & (lb > 0)
    key = la[both].to(torch.int64) << 32 | lb[both].to(torch.int64)
    pairs, counts = torch.unique(key, return_counts=True)
    return torch.stack([pairs >> 32, pairs & 0xffffffff, counts.to(torch.int64)], 1).reshape(-1, 3)


def foreground(m, classes=None):
    """u8 mask: isin(map, classes), non-zero where classes is None"""
    if classes is None:
        return (m != 0).to(torch.uint8)
    lut = torch.from_numpy(traced_table(classes)).to(m.device)
    return lut[m.long()]


def score_dict(n_pred, n_gt, tp_pred, tp_gt):
    precision = tp_pred / n_pred if n_pred else (1.0 if n_gt == 0 else 0.0)
    recall = tp_gt / n_gt if n_gt else (1.0 if n_pred == 0 else 0.0)
    f1 = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
    return dict(n_pred=n_pred, n_gt=n_gt, tp_pred=tp_pred, tp_gt=tp_gt, fp=n_pred - tp_pred, fn=n_gt - tp_gt, precision=precision, recall=recall, f1=f1)


def lesion_scores(pred, gt, classes=None, connectivity=8, iou=0.5, min_area=0):
    """Lesions as objects.  The foreground of each map is isin(map, classes) (None: non-zero); regions of fewer than min_area pixels are
    left out of both.  A ground-truth region is found iff some predicted region p has inter den >= num (area_p + area_g - inter) in
    integers, num / den = Fraction(iou).limit_denominator(2^20); a predicted region is true by the same test; iou = 0 means any shared
    pixel.  -> n_pred, n_gt, tp_pred, tp_gt, fp, fn, precision (tp_pred / n_pred; without predictions 1.0 if there is no ground truth
    either, else 0.0), recall (the mirror image), f1 (0.0 where precision + recall is 0).  The default 0.5 is the usual object-level
    convention, not a measurement."""
    fr = Fraction(iou).limit_denominator(1 << 20)
    if not 0 <= fr <= 1:
        raise ValueError('iou %r is outside [0, 1]' % (iou,))
    num, den = fr.numerator, fr.denominator
    pred, gt = as_u8(pred, 'the prediction'), as_u8(gt, 'the ground truth')
    rp, rg = label(foreground(pred, classes), None, connectivity), label(foreground(gt, classes), None, connectivity)
    ap, ag = rp.host()[:, _F['area']], rg.host()[:, _F['area']]
    keep_p, keep_g = ap >= min_area, ag >= min_area
    found_p, found_g = np.zeros(rp.n, bool), np.zeros(rg.n, bool)
    if rp.n and rg.n:
        o = overlaps(rp, rg).cpu().numpy()
        p, g, inter = o[:, 0] - 1, o[:, 1] - 1, o[:, 2]          # areas are below 2^30 and den at most 2^20: the products stay in int64
        hit = keep_p[p] & keep_g[g] & (inter * den >= num * (ap[p] + ag[g] - inter))
        found_p[p[hit]] = True
        found_g[g[hit]] = True
    return score_dict(int(keep_p.sum()), int(keep_g.sum()), int((found_p & keep_p).sum()), int((found_g & keep_g).sum()))


def bed_size(mask, step=1, mpp=None):
    """The two dimensions a pathologist reports for the tumour bed, from a u8 (or bool) CUDA mask: of its largest region at connectivity 8
    (ties: the smallest id) d1 = the largest diameter and d2 = the extent at right angles to it, in map pixels, with area, hull_area and
    solidity; with mpp (microns per level-0 pixel; a map pixel is `step` of them) also d1_mm, d2_mm, area_mm2.  None on an empty mask."""
    r = label(as_u8(mask, 'the mask'), None, 8, labels=False, hulls=True)
    if r.n == 0:
        return None
    areas = r.host()[:, _F['area']]
    k = int(np.argmax(areas))                                   # the first of the largest
    h = r.hulls
    area, hull_area = int(areas[k]), float(h.hull_area()[k])
    out = dict(d1=float(h.feret_max()[k]), d2=float(h.feret_orth()[k]), area=area, hull_area=hull_area, solidity=area / hull_area)
    if mpp is not None:
        mm = int(step) * float(mpp) / 1000.0
        out.update(d1_mm=out['d1'] * mm, d2_mm=out['d2'] * mm, area_mm2=area * mm * mm)
    return out


def heat_threshold(thresh):
    """heat / 255 >= thresh on u8 codes: heat >= ceil(thresh 255) (253 for 0.99)"""
    return int(math.ceil(255.0 * float(thresh) - 1e-9))


def slide_positive(heat_u8, thresh=0.99, open_k=50, min_fraction=0.0):
    """Does this slide hold tumour at all?  The reference's rule (paper_tools/check_for_false_positives.py:61-69) on the device:
    uint8(heat >= thresh 255) -> open open_k x open_k -> count_nonzero / size > min_fraction.  -> {'positive', 'fraction', 'n_regions',
    'largest_area'}, the last two from the regions of the opened mask (connectivity 8)."""
    return _slide_positive(heat_u8, thresh, open_k, min_fraction)[0]


def _slide_positive(heat_u8, thresh, open_k, min_fraction, hulls=False):
    from . import postprocess as PP
    heat = as_u8(heat_u8, 'the heat map').contiguous()
    opened = PP.morph_rect((heat >= heat_threshold(thresh)).to(torch.uint8), open_k, 'open')
    r = label(opened, None, 8, labels=False, weight=heat, **({'hulls': True} if hulls else {}))
    fraction = int(torch.count_nonzero(opened)) / opened.numel()
    return dict(positive=bool(fraction > min_fraction), fraction=float(fraction), n_regions=r.n,
                largest_area=int(r.area.max()) if r.n else 0), r
