"""Ground-truth class maps from the pathologists' XML annotations, rasterised on the device.

The reference makes `<slide>_mask.png` / `<slide>_tumor_bed.png` on the host (preprocess/mk_gt.py:20-39, utils/read_xml.py:24-106 for
Aperio ImageScope files, utils/read_xml_sunnybrook.py:25-194 for Sedeen files): cv2.fillPoly on a full-resolution (H0, W0, 3) canvas,
of which every `4 ** level`-th pixel is kept.  Only the lattice points (x s, y s) are ever read, so this module evaluates polygon
coverage at those points directly, in exact integer arithmetic, on the GPU (wsi_poly_raster, csrc/poly.hip); the map appears where its
consumers are (wsi_score_counts, wsi_mask_iou_counts, the convex hull).

The coverage rule is this project's own (spec: tests/annotations_oracle.py; it is not pinned against cv2, whose rounding of edges
cannot be reproduced here): a polygon of n >= 1 integer vertices, closed implicitly, covers a lattice point p if p lies on one of its
closed edges, or if an odd number of edges cross p's scanline strictly to the right of p (even-odd rule; an edge with ends lo, hi
sorted by y crosses iff lo.y <= py < hi.y and (hi.x - lo.x)(py - lo.y) - (px - lo.x)(hi.y - lo.y) > 0).  Polygons are painted in list
order; label 0 erases.  Every coordinate and every sampled point lies in [-2^29, 2^29].  There is no CPU fallback."""
import xml.etree.ElementTree as ET

import numpy as np
import torch

from . import native
from .engine import _ptr, _require_gpu

LIMIT = 1 << 29                          # csrc/poly_dev.h wsi_poly::LIMIT
TILE_W, TILE_H = 128, 32                 # the kernel's tile (TILE_W, TILE_H), the edges it stages per pass (EDGE_CHUNK) and the LDS
EDGE_CHUNK, EDGE_CAP = 256, 512          # slots they are compacted into (EDGE_CAP): tests/test_annotations_cpu.py compares with the header

IMAGESCOPE_CLASSES = (('benign', 1), ('in situ', 2), ('invasive', 3))
SEDEEN_SKIPPED_TYPES = ('point', 'ellipse', 'text')


# ------------------------------------------------------------------------------------------------------------------------ parsers
def read_imagescope(path, negative=None):
    """Aperio ImageScope / BACH XML (reference utils/read_xml.py:29-66) -> (coords, labels, lengths, areas, microns per pixel): the
    regions under root[0][1]; a region's label is its first attribute's `Value`, or its own `Text`, mapped by substring
    (case-insensitive) benign / in situ / invasive -> 1 / 2 / 3.  A label that matches none raises ValueError naming the region (the
    reference fails later, with a TypeError, when it indexes its colour list).
    negative: None reads a region with NegativeROA="1" like any other (the reference's behaviour); 'erase' gives it the label 0, so
    that painting in file order subtracts it (what contours.write_imagescope(holes='negative') writes for a hole)."""
    if negative not in (None, 'erase'):
        raise ValueError("negative must be None or 'erase', not %r" % (negative,))
    root = ET.parse(path).getroot()
    coords, labels, lengths, areas = [], [], [], []
    for k, r in enumerate(root[0][1].findall('Region')):
        try:
            text = r[0][0].get('Value')
        except IndexError:
            text = None
        if text is None:
            text = r.get('Text')
        label = next((c for name, c in IMAGESCOPE_CLASSES if name in (text or '').lower()), None)
        if label is None:
            raise ValueError('%s: region %s has the label %r, which is none of benign / in situ / invasive' % (path, r.get('Id', k), text))
        areas.append(float(r.get('AreaMicrons')))
        lengths.append(float(r.get('LengthMicrons')))
        labels.append(0 if negative == 'erase' and r.get('NegativeROA') == '1' else label)
        coords.append([[int(v.get('X')), int(v.get('Y'))] for v in r[1]])
    return coords, labels, lengths, areas, float(root.get('MicronsPerPixel'))


def class_dictionary(label):
    """the class of a Sedeen description (reference utils/read_xml_sunnybrook.py:47-70), restated rule by rule"""
    label = label.lower().replace(' ', '')
    if 'cellularity' in label:
        out = 0
    elif label == 'i' or 'invasive' in label or 'idc' in label or 'ilc' in label:
        out = 3
    elif 'dcis' in label:
        out = 2
    elif 'benign' in label or 'udh' in label:
        out = 1
    else:
        out = 0                                                 # normal, tb and everything else
    if 'no dcis' in label and out == 2:                         # (spaces are gone by now: the reference's rule never fires; kept as it stands)
        out = 0
    return out


def _sedeen_graphics(path, keep):
    root = ET.parse(path).getroot()
    coords, labels = [], []
    for g in root[0][3].findall('graphic'):
        description = g.get('description')
        if not keep(g, description):
            continue
        coords.append([tuple(int(float(i)) for i in p.text.split(',')) for p in g[2].findall('point')])
        labels.append(description)
    return coords, labels


def read_sedeen(path):
    """Sunnybrook / Sedeen session XML (reference :112-141) -> (coords, descriptions): the graphics under root[0][3] whose class is not
    0 and whose type is none of point / ellipse / text; a vertex is int(float(.)) of each half of its `x,y` text."""
    return _sedeen_graphics(path, lambda g, d: class_dictionary(d) != 0 and g.get('type') not in SEDEEN_SKIPPED_TYPES)


def read_sedeen_tb(path):
    """the tumour-bed graphics (reference :197-223): descriptions that contain `tb` (lower case, spaces removed; returned in that form)"""
    coords, labels = _sedeen_graphics(path, lambda g, d: 'tb' in d.lower().replace(' ', ''))
    return coords, [l.lower().replace(' ', '') for l in labels]


def sedeen_polygons(coords, classes, size):
    """fillImage's two rules (reference :25-43) on Sedeen polygons: a coordinate above the image size (W0, H0) becomes size - 1, and a
    polygon is kept only if its box is more than 100 in both directions.  -> (coords, classes) of the kept polygons."""
    w0, h0 = int(size[0]), int(size[1])
    out_c, out_l = [], []
    for c, l in zip(coords, classes):
        v = np.asarray(c, np.int64).reshape(-1, 2).copy()
        if len(v) == 0:
            continue
        v[v[:, 0] > w0, 0] = w0 - 1
        v[v[:, 1] > h0, 1] = h0 - 1
        if v[:, 0].max() - v[:, 0].min() > 100 and v[:, 1].max() - v[:, 1].min() > 100:
            out_c.append(v)
            out_l.append(l)
    return out_c, out_l


# --------------------------------------------------------------------------------------------------------------------- rasteriser
def _in_limit(v, what):
    if not -LIMIT <= int(v) <= LIMIT:
        raise ValueError('%s %d is outside [-2^29, 2^29], the range the exact 64-bit coverage test is stated for' % (what, int(v)))
    return int(v)


def pack_polygons(coords, labels):
    """-> (edges int32 (E, 4): x0, y0, x1, y1 per edge, 16 bytes; polys int32 (P, 8): first edge, edge count, box xmin, ymin, xmax,
    ymax, label, 0).  A polygon of n vertices has n edges, the last one closing it (n = 1: one zero-length edge)."""
    coords, labels = list(coords), list(labels)
    if len(coords) != len(labels):
        raise ValueError('%d polygons but %d labels' % (len(coords), len(labels)))
    if not coords:
        return np.zeros((0, 4), np.int32), np.zeros((0, 8), np.int32)
    verts = [np.asarray(c).reshape(-1, 2) for c in coords]
    count = np.array([len(v) for v in verts], np.int64)
    for k in np.flatnonzero(count == 0):
        raise ValueError('polygon %d has no vertex' % k)
    for k, v in enumerate(verts):
        if not np.issubdtype(v.dtype, np.integer):
            raise ValueError('polygon %d: vertices must be integers' % k)
    lab = np.array([int(l) for l in labels], np.int64)
    for k in np.flatnonzero((lab < 0) | (lab > 255)):
        raise ValueError('polygon %d: label %d is not a byte' % (k, lab[k]))
    v = np.concatenate(verts)                                    # every polygon's vertices, one after the other
    first = np.concatenate(([0], np.cumsum(count)[:-1]))
    if len(v) > 0x7fffffff:
        raise ValueError('%d edges do not fit the 32-bit edge index' % len(v))
    if int(v.min()) < -LIMIT or int(v.max()) > LIMIT:
        bad = np.flatnonzero(((v < -LIMIT) | (v > LIMIT)).any(1))[0]
        k = int(np.searchsorted(first, bad, 'right')) - 1
        _in_limit([int(c) for c in v[bad] if not -LIMIT <= int(c) <= LIMIT][0], 'polygon %d: the coordinate' % k)
    edges = np.empty((len(v), 4), np.int32)
    edges[:, :2] = v
    edges[:-1, 2:] = v[1:]                                       # an edge ends at the next vertex,
    edges[first + count - 1, 2:] = v[first]                      # the polygon's last one at its first
    polys = np.zeros((len(verts), 8), np.int32)
    polys[:, 0], polys[:, 1], polys[:, 6] = first, count, lab
    polys[:, 2:4], polys[:, 4:6] = np.minimum.reduceat(v, first), np.maximum.reduceat(v, first)
    return edges, polys


def rasterize(coords, labels, size, step=1, origin=(0, 0), out=None, device='cuda'):
    """The u8 (H, W) map of size = (W, H) on the GPU: pixel (x, y) samples (origin + (x, y) * step) of the polygons, painted in list
    order.  step: an integer or (sx, sy), >= 1; origin: integers, may be negative.  out: a 2-D u8 GPU tensor (H, W) with unit column
    stride (any row stride, any alignment) that is painted over and returned; uncovered pixels keep its bytes."""
    lib = native.load()
    w, h = int(size[0]), int(size[1])
    sx, sy = (int(step), int(step)) if np.isscalar(step) else (int(step[0]), int(step[1]))
    ox, oy = int(origin[0]), int(origin[1])
    if w <= 0 or h <= 0 or sx < 1 or sy < 1:
        raise ValueError('size %r and step %r must be positive' % (size, step))
    for what, v in (('the origin x', ox), ('the origin y', oy), ('the last sampled x', ox + (w - 1) * sx if w > 1 else ox),
                    ('the last sampled y', oy + (h - 1) * sy if h > 1 else oy)):
        _in_limit(v, what)
    edges, polys = pack_polygons(coords, labels)
    if out is None:
        out = torch.zeros((h, w), dtype=torch.uint8, device=device)
    _require_gpu(out, 'the map to paint over')
    if out.dtype != torch.uint8 or out.dim() != 2 or tuple(out.shape) != (h, w) or (w > 1 and out.stride(1) != 1) or (h > 1 and out.stride(0) < w):
        raise ValueError('out must be a (%d, %d) uint8 tensor with contiguous rows' % (h, w))
    if len(polys) == 0:
        return out
    dev = out.device
    e_dev, p_dev = torch.from_numpy(edges).to(dev), torch.from_numpy(polys).to(dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        native.check(lib.wsi_poly_raster(_ptr(e_dev), len(edges), _ptr(p_dev), len(polys), _ptr(out), w, h, out.stride(0) if h > 1 else w,
                                         ox, oy, sx, sy, st), 'wsi_poly_raster')
    return out


def level_step(scan, level):
    """the integer nearest scan.level_downsamples[level]; ValueError where that is more than 1 % off (pass an explicit step then)"""
    ds = float(scan.level_downsamples[level])
    step = max(1, int(round(ds)))
    if abs(step - ds) > 0.01 * ds:
        raise ValueError('level %d has the downsample %.4f, which is no integer to 1 %%: pass an explicit step' % (level, ds))
    return step


def level_map(coords, labels, scan, level, device='cuda', step=None):
    """The class map at pyramid level `level`, u8 (h, w) = level_dimensions[level] on the GPU.  The reference keeps every step-th pixel
    of the full-resolution canvas, ceil(W0 / step) x ceil(H0 / step) of them; that map is cropped or zero-padded to the level's size,
    which may differ by at most one pixel each way (ValueError otherwise).  There is no resize."""
    step = level_step(scan, level) if step is None else int(step)
    w0, h0 = scan.level_dimensions[0]
    lw, lh = scan.level_dimensions[level]
    sw, sh = -(-int(w0) // step), -(-int(h0) // step)
    if abs(sw - lw) > 1 or abs(sh - lh) > 1:
        raise ValueError('level %d is %d x %d but every %d-th pixel of %d x %d gives %d x %d: pass the step this level was made with'
                         % (level, lw, lh, step, w0, h0, sw, sh))
    out = torch.zeros((int(lh), int(lw)), dtype=torch.uint8, device=device)
    w, h = min(sw, int(lw)), min(sh, int(lh))
    rasterize(coords, labels, (w, h), step, out=out[:h, :w])
    return out


def tumor_bed_map(gt):
    """The ground-truth tumour bed of a class map (reference utils/read_xml.py:96-106): the convex hull image of (gt >= 2), the
    malignant classes, u8 0 / 1 on the GPU - the hull step of postprocess.tumor_bed with its open and dilate at 1 x 1."""
    from . import postprocess
    _require_gpu(gt, 'class map')
    return postprocess.tumor_bed(gt.contiguous(), 2, 1, 1).tb_pred


def slide_ground_truth(xml_path, scan, fmt, device='cuda'):
    """(gt, tb_gt) u8 GPU maps of a slide at the level utils.eval.predict_wsis scores at, min(2, level_count - 1).
    fmt: 'imagescope', 'sedeen' or callable(path, scan) -> (coords, integer labels).  Sedeen: fillImage's clamp and 100-pixel rule
    apply, and tb_gt is the union of the `tb` graphics when the file has any (the hull of the malignant classes otherwise)."""
    level = min(2, len(scan.level_dimensions) - 1)
    tb = None
    if fmt == 'imagescope':
        coords, labels = read_imagescope(xml_path)[:2]
    elif fmt == 'sedeen':
        coords, desc = read_sedeen(xml_path)
        coords, labels = sedeen_polygons(coords, [class_dictionary(d) for d in desc], scan.level_dimensions[0])
        tb_coords = sedeen_polygons(*read_sedeen_tb(xml_path), scan.level_dimensions[0])[0]
        if tb_coords:
            tb = level_map(tb_coords, [1] * len(tb_coords), scan, level, device)
    elif callable(fmt):
        coords, labels = fmt(xml_path, scan)
    else:
        raise ValueError("annotations must be None, 'imagescope', 'sedeen' or a callable, not %r" % (fmt,))
    gt = level_map(coords, labels, scan, level, device)
    return gt, (tumor_bed_map(gt) if tb is None else tb)
