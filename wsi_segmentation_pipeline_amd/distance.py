"""Distances on resident u8 maps: the exact Euclidean distance transform on the device (wsi_edt_*, csrc/edt.hip), and what follows from
it - round structuring elements, margin bands round a mask, and the surface scores between two outlines (Hausdorff, HD95, mean surface
distance) that an area ratio cannot give.

The rule is this project's own (spec: tests/edt_oracle.py; the reference has no such code): a pixel is a feature iff its byte is
non-zero (zero with invert), out[y, x] = min over features of (y - fy)^2 + (x - fx)^2 as int32, EDT_NONE everywhere on a map without a
feature.  SciPy's convention is the mirror image: distance_transform_edt(features == 0) ** 2.  Pixels are isotropic, and no
nearest-feature index is produced.  All of it is integer and bit-reproducible.  There is no CPU fallback."""
import math

import torch

from . import native
from .engine import _ptr, _require_gpu
from .maps import as_u8, check_map, check_out_i32, stage_marker, take_workspace

EDT_NONE = 0x7FFFFFFF                    # csrc/edt_dev.h wsi_edt::EDT_NONE
G_NONE = 0xFFFF                          # wsi_edt::G_NONE
LIMIT = 32768                            # wsi_edt::LIMIT: W, H <= LIMIT
BAND = 64                                # wsi_edt::BAND: rows of one band of the column pass


def g_pitch(w):
    """u16 values between two rows of the workspace's g plane (the plane starts the workspace)"""
    return (int(w) + 127) // 128 * 128


def distance_sq(features, invert=False, out=None, workspace=None, stages=None):
    """Squared Euclidean distance to the nearest feature of a u8 (H, W) CUDA map (unit column stride, any row stride and alignment)
    -> int32 (H, W); EDT_NONE everywhere where the map has no feature.  out: an int32 (H, W) tensor to fill (unit column stride);
    workspace: a u8 tensor of at least wsi_edt_workspace_bytes(W, H) to reuse; stages: a dict that receives, per pass ('columns',
    'rows'), the [begin, end] torch.cuda.Event pair recorded round its entry (tools/edt_times.py)."""
    lib = native.load()
    h, w, pitch = check_map(features, 'the map', LIMIT)
    _require_gpu(features, 'the map')
    dev = features.device
    if out is None:
        out = torch.empty((h, w), dtype=torch.int32, device=dev)
    else:
        check_out_i32(out, h, w, dev)
    workspace = take_workspace(workspace, lib.wsi_edt_workspace_bytes(w, h), dev)
    out_pitch = 4 * (out.stride(0) if h > 1 else w)
    mark = stage_marker(stages)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        mark('columns')
        native.check(lib.wsi_edt_columns(_ptr(features), w, h, pitch, int(bool(invert)), _ptr(workspace), workspace.numel(), st), 'wsi_edt_columns')
        mark('columns')
        mark('rows')
        native.check(lib.wsi_edt_rows(_ptr(workspace), workspace.numel(), w, h, _ptr(out), out_pitch, st), 'wsi_edt_rows')
        mark('rows')
    return out


def distance(features, invert=False):
    """the float64 square root of distance_sq; inf where the map has no feature"""
    d2 = distance_sq(features, invert)
    return torch.where(d2 == EDT_NONE, torch.full((), math.inf, dtype=torch.float64, device=d2.device), d2.to(torch.float64).sqrt())


def _mask(mask):
    mask = as_u8(mask, 'the map')
    check_map(mask, 'the map', LIMIT)
    return mask


def _radius(r, what):
    if isinstance(r, bool) or int(r) != r or int(r) < 0 or int(r) >= LIMIT:
        raise ValueError('%s %r must be an integer in 0 .. %d' % (what, r, LIMIT - 1))
    return int(r)


def morph_disc(mask, r, op):
    """Dilate / erode / open / close a u8 (H, W) CUDA mask by the disc of radius r (an int >= 0, compared on squares) -> u8 0 / 1.
    dilate: d2(mask) <= r^2; erode: d2(mask, invert=True) > r^2; open = dilate of erode, close = erode of dilate.  Outside the map is
    neither feature nor background, so erosion does not eat from the border (cv2's convention, which postprocess.morph_rect follows)."""
    mask, r2 = _mask(mask), _radius(r, 'the radius') ** 2
    if op not in ('dilate', 'erode', 'open', 'close'):
        raise ValueError("op must be 'dilate', 'erode', 'open' or 'close', not %r" % (op,))
    dilate = lambda m: (distance_sq(m) <= r2).to(torch.uint8)
    erode = lambda m: (distance_sq(m, invert=True) > r2).to(torch.uint8)
    return {'dilate': dilate, 'erode': erode, 'open': lambda m: dilate(erode(m)), 'close': lambda m: erode(dilate(m))}[op](mask)


def margin_band(mask, inner, outer):
    """The ring round a mask's border -> u8 0 / 1: a pixel inside the mask within `inner` of the nearest pixel outside it, or outside
    the mask within `outer` of it (integers, compared on squares)."""
    mask = _mask(mask)
    i2, o2 = _radius(inner, 'inner') ** 2, _radius(outer, 'outer') ** 2
    inside = mask != 0
    return ((inside & (distance_sq(mask, invert=True) <= i2)) | (~inside & (distance_sq(mask) <= o2))).to(torch.uint8)


def pooled_scores(values, counts, n_a, n_b, spacing=1.0):
    """hd, hd95, assd from the pooled multiset of squared surface distances, given as ascending unique values and their counts (host
    integers).  hd = spacing * sqrt(max); hd95 = spacing * sqrt(the k-th smallest), k = ceil(0.95 n) (nearest rank: an exact integer
    until the root); assd = spacing * (sum over ascending values of count * sqrt(value)) / n in float64, the order fixed, so the same
    bits every run.  Both surfaces empty: 0.0 each; exactly one empty: inf each."""
    n = n_a + n_b
    if n == 0:
        return {'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'n_a': 0, 'n_b': 0}
    if n_a == 0 or n_b == 0:
        return {'hd': math.inf, 'hd95': math.inf, 'assd': math.inf, 'n_a': n_a, 'n_b': n_b}
    k = (95 * n + 99) // 100
    seen, kth, total = 0, values[-1], 0.0
    for v, c in zip(values, counts):
        if seen < k <= seen + c:
            kth = v
        seen += c
        total += c * math.sqrt(v)
    s = float(spacing)
    return {'hd': s * math.sqrt(values[-1]), 'hd95': s * math.sqrt(kth), 'assd': s * total / n, 'n_a': n_a, 'n_b': n_b}


def surface_distances(a, b, spacing=1.0):
    """Hausdorff, HD95 and average symmetric surface distance between two u8 (H, W) CUDA masks of one size ->
    {'hd', 'hd95', 'assd', 'n_a', 'n_b'}, in pixels times `spacing`.  The surfaces are postprocess.bwperim(a) and bwperim(b) (4-connected,
    outside counting as unset); the directed squared distances are distance_sq of the other surface gathered at this surface's
    pixels; both directions are pooled into one multiset of n = n_a + n_b integers (pooled_scores)."""
    from . import postprocess as PP
    a, b = _mask(a), _mask(b)
    if a.shape != b.shape or a.device != b.device:
        raise ValueError('the two masks must have one size and one device')
    sa, sb = PP.bwperim(a) > 0, PP.bwperim(b) > 0
    n_a, n_b = int(sa.sum().item()), int(sb.sum().item())
    if n_a == 0 or n_b == 0:
        return pooled_scores([], [], n_a, n_b, spacing)
    pooled = torch.cat([distance_sq(sb.to(torch.uint8))[sa], distance_sq(sa.to(torch.uint8))[sb]])
    values, counts = torch.unique(pooled, sorted=True, return_counts=True)
    return pooled_scores(values.tolist(), counts.tolist(), n_a, n_b, spacing)
