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

    def __init__(self, table, labels, size, n_runs=0):
        self.table, self.labels, self.size, self.n_runs = table, labels, (int(size[0]), int(size[1])), int(n_runs)
        self.n = int(table.shape[0])
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

    def rows(self, step=1, origin=(0, 0), mpp=None):
        """one dict per region: id, class, area_px (map pixels), area_um2 (None without mpp; a map pixel is step x step level-0 pixels
        of mpp microns), the box and the centroid in level-0 coordinates (map pixel x covers origin + x step .. origin + (x + 1) step,
        its centre is origin + (x + 0.5) step), perim (pixel sides), major, minor (map pixels), mean_weight (wsum / area)"""
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
        return out


CSV_COLUMNS = ('id', 'class', 'name', 'area_px', 'area_um2', 'x0', 'y0', 'x1', 'y1', 'cx', 'cy', 'perim', 'major', 'minor', 'mean_weight')


def write_csv(path, r, step=1, origin=(0, 0), mpp=None, names=None):
    """the rows of `r` as CSV, one line per region under CSV_COLUMNS; names: {class: name} (a class without one gets ''); area_um2 is
    empty where mpp is None"""
    names = names or {}
    with open(path, 'w', newline='', encoding='utf-8') as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for row in r.rows(step, origin, mpp):
            row['name'] = names.get(row['class'], '')
            w.writerow(['' if row[c] is None else ('%.4f' % row[c] if isinstance(row[c], float) else row[c]) for c in CSV_COLUMNS])
    return path


def label(m, classes=None, connectivity=8, labels=True, weight=None, out=None, workspace=None, stages=None):
    """Label a u8 (H, W) CUDA class map (unit column stride, any row stride and alignment) -> `Regions`.
    classes: None takes labels 1..255, an iterable of ints those labels (0 allowed).  connectivity: 4 or 8.  labels: also paint the
    (H, W) int32 label map (into `out` where given: int32, unit column stride, any row stride).  weight: a u8 map of the same shape
    whose sum per region goes into `wsum`.  workspace: a u8 tensor at least wsi_region_workspace_bytes large to work in.
    Two synchronisations: the run count sizes the workspace, the region count sizes the table.  A map without a traced pixel launches
    nothing after the count.  stages: a dict that receives, per name of STAGES, the [begin, end] torch.cuda.Event pair of the stage."""
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
            return Regions(torch.zeros((0, 16), dtype=torch.int64, device=dev), lab, (w, h))
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
    return Regions(tab, lab, (w, h), n_runs)


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


def heat_threshold(thresh):
    """heat / 255 >= thresh on u8 codes: heat >= ceil(thresh 255) (253 for 0.99)"""
    return int(math.ceil(255.0 * float(thresh) - 1e-9))


def slide_positive(heat_u8, thresh=0.99, open_k=50, min_fraction=0.0):
    """Does this slide hold tumour at all?  The reference's rule (paper_tools/check_for_false_positives.py:61-69) on the device:
    uint8(heat >= thresh 255) -> open open_k x open_k -> count_nonzero / size > min_fraction.  -> {'positive', 'fraction', 'n_regions',
    'largest_area'}, the last two from the regions of the opened mask (connectivity 8)."""
    return _slide_positive(heat_u8, thresh, open_k, min_fraction)[0]


def _slide_positive(heat_u8, thresh, open_k, min_fraction):
    from . import postprocess as PP
    heat = as_u8(heat_u8, 'the heat map').contiguous()
    opened = PP.morph_rect((heat >= heat_threshold(thresh)).to(torch.uint8), open_k, 'open')
    r = label(opened, None, 8, labels=False, weight=heat)
    fraction = int(torch.count_nonzero(opened)) / opened.numel()
    return dict(positive=bool(fraction > min_fraction), fraction=float(fraction), n_regions=r.n,
                largest_area=int(r.area.max()) if r.n else 0), r
