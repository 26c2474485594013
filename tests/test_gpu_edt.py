"""GPU side of the distance transform (csrc/edt.hip through wsi_segmentation_pipeline_amd.distance): every case byte for byte equal to the
spec (tests/edt_oracle.py) - the int32 distances and the workspace inside 0xA5 guards, the map inside guards at four base alignments and
three pitches and never written - the two entries driven alone, then morph_disc, margin_band, surface_distances and the
boundary_scores hook of predict_wsis."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contour_fixture as CF                                   # noqa: E402
import edt_fixture as F                                        # noqa: E402
import edt_oracle as O                                         # noqa: E402
from wsi_segmentation_pipeline_amd import distance as D, native      # noqa: E402
from wsi_segmentation_pipeline_amd.slide import ArraySlide     # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0xA5
PLACES = ((0, 0), (1, 5), (3, 16), (8, 5))                      # (bytes before the map's first byte mod 16, pitch - W)
FRONT = 256                                                     # guard bytes before the workspace and the output (keeps their alignment)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def place(dev, m, offset, extra):
    """the map inside a guarded allocation: first byte `offset` bytes in, rows W + extra apart -> (the strided view, the whole buffer)"""
    h, w = m.shape
    pitch = w + extra
    host = np.full(offset + h * pitch + 64, GUARD, np.uint8)
    np.lib.stride_tricks.as_strided(host[offset:], (h, w), (pitch, 1))[:] = m
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 16 == 0
    return torch.as_strided(buf, (h, w), (pitch, 1), offset), buf, host


def guarded(dev, nbytes):
    """nbytes of 0xA5 between FRONT bytes of guard before and 64 behind -> (the whole buffer, the inner u8 view)"""
    buf = torch.full((FRONT + nbytes + 64,), GUARD, dtype=torch.uint8, device=dev)
    return buf, buf[FRONT:FRONT + nbytes]


def spec(m, invert):
    g = O.column_distances(m, invert)
    return g, O.rows_from_g(g)


def check(dev, m, invert=False, places=PLACES[1:2], out_extra=3, want=None):
    """the transform of `m` at every placement into a guarded output of pitch W + out_extra and a guarded workspace: the spec's bytes,
    the spec's g plane, no byte written outside either, the map's allocation untouched"""
    lib = native.load()
    m = np.ascontiguousarray(m, np.uint8)
    h, w = m.shape
    want_g, want = spec(m, invert) if want is None else want
    for offset, extra in places:
        view, buf, host = place(dev, m, offset, extra)
        need = lib.wsi_edt_workspace_bytes(w, h)
        ws_buf, ws = guarded(dev, need)
        out_pitch = w + out_extra
        out_buf, out_bytes = guarded(dev, 4 * h * out_pitch)
        out = torch.as_strided(out_bytes.view(torch.int32), (h, w), (out_pitch, 1))
        got = D.distance_sq(view, invert, out=out, workspace=ws)
        assert got.data_ptr() == out.data_ptr()
        assert np.array_equal(got.cpu().numpy(), want), (offset, extra, invert)
        whole = out_buf.cpu().numpy()
        inner = whole[FRONT:FRONT + 4 * h * out_pitch].reshape(h, 4 * out_pitch)
        assert (whole[:FRONT] == GUARD).all() and (whole[FRONT + 4 * h * out_pitch:] == GUARD).all() and (inner[:, 4 * w:] == GUARD).all()
        whole = ws_buf.cpu().numpy()
        assert (whole[:FRONT] == GUARD).all() and (whole[FRONT + need:] == GUARD).all()
        plane = whole[FRONT:FRONT + 2 * h * D.g_pitch(w)].view(np.uint16).reshape(h, D.g_pitch(w))
        assert np.array_equal(plane[:, :w], want_g), (offset, extra, invert)
        assert np.array_equal(buf.cpu().numpy(), host)           # the map is never written, nor a byte round it
    return want


# ------------------------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize('w', (1, 15, 16, 17, 255, 256, 257, F.ROW_ROUND + 1))
def test_widths_round_the_16_byte_piece_the_column_tile_and_the_row_round(dev, w):
    """2049: one value past what the row pass's lanes fetch per round (256 lanes x 8 values), and a ninth column tile of one column"""
    for h in ((2,) if w > 2000 else (1, 3, 65)):
        for invert in (False, True):
            check(dev, F.random_map(h, w, 0.02, 100 * w + h), invert)


@pytest.mark.parametrize('h', (F.BAND - 1, F.BAND, F.BAND + 1, 2 * F.BAND + 1))
def test_heights_round_the_band(dev, h):
    for w in (37, 300):
        check(dev, F.random_map(h, w, 0.004, 7 * h + w), False)
        check(dev, F.random_map(h, w, 0.97, 9 * h + w), True)


@pytest.mark.parametrize('offset', (0, 1, 3, 8))
def test_base_alignments_and_pitches(dev, offset):
    m = F.random_map(70, 83, 0.01, 77)
    want = spec(m, False)
    check(dev, m, places=[(offset, extra) for extra in (0, 5, 16)], want=want)
    check(dev, m[:, :33], places=[(offset, 0), (offset, 5)], out_extra=0)


# ----------------------------------------------------------------------------------------------------------------------- contents
def test_empty_and_all_feature_maps(dev):
    for h, w in ((1, 1), (70, 300)):
        for fill, invert in ((0, False), (9, True)):
            want = check(dev, np.full((h, w), fill, np.uint8), invert)
            assert (want == O.EDT_NONE).all()
        for fill, invert in ((200, False), (0, True)):
            assert (check(dev, np.full((h, w), fill, np.uint8), invert) == 0).all()
    d = D.distance(torch.zeros((5, 9), dtype=torch.uint8, device=dev))
    assert d.dtype == torch.float64 and torch.isinf(d).all()


def test_one_feature_in_each_corner(dev):
    h, w = 2 * F.BAND + 9, 270
    yy, xx = np.mgrid[0:h, 0:w]
    singles = []
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 1
        singles.append(check(dev, m))
        assert np.array_equal(singles[-1], (yy - y) ** 2 + (xx - x) ** 2)
    want = check(dev, F.corners(h, w), places=PLACES[2:3])
    assert np.array_equal(want, np.minimum.reduce(singles)) and want.max() > 20000


def test_feature_only_in_the_last_band(dev):
    """the lower carry crosses four whole bands upward (and, inverted, every band has features but for single rows)"""
    h, w = 4 * F.BAND + 3, 45
    m = np.zeros((h, w), np.uint8)
    m[h - 2, ::3] = 1
    want = check(dev, m)
    assert want[0, 0] == (h - 2) ** 2 and want[0, 1] == (h - 2) ** 2 + 1
    check(dev, m[::-1], places=PLACES[3:])                       # and the upper carry downward
    check(dev, m, True)


def test_columns_without_a_feature(dev):
    m = F.random_map(130, 40, 0.3, 3)
    m[:, 5] = m[:, 39] = m[:, 0] = 0
    g = O.column_distances(m)
    assert (g[:, [0, 5, 39]] == O.G_NONE).all() and (g[:, 1] != O.G_NONE).all()
    check(dev, m)
    check(dev, np.where(m > 0, 0, 1).astype(np.uint8), True)


def test_blob_map_512_x_384(dev):
    m = CF.blob_map(384, 512, 3, 5)
    want = check(dev, m, places=PLACES[1:2])
    assert want.max() > 1 and (want == 0).sum() == (m > 0).sum() and (want[m == 0] > 0).all()
    inv = check(dev, m, True, places=PLACES[3:])
    assert ((want == 0) ^ (inv == 0)).all()
    a, b = D.distance_sq(torch.from_numpy(m).to(dev)), D.distance_sq(torch.from_numpy(m).to(dev))
    assert torch.equal(a, b) and a.is_cuda and a.dtype == torch.int32


# ---------------------------------------------------------------------------------------------------------- the entries driven alone
def test_rows_alone_on_the_hand_made_plane_of_the_largest_sum(dev):
    lib = native.load()
    w = 32768
    g = F.largest_sum_row(w)
    need = lib.wsi_edt_workspace_bytes(w, 1)
    assert D.g_pitch(w) == w and need >= 2 * w
    ws_buf, ws = guarded(dev, need)
    ws[:2 * w] = torch.from_numpy(g.view(np.uint8)).to(dev)      # the documented layout: the plane at offset 0
    before = ws_buf.cpu().numpy().copy()
    out_buf, out_bytes = guarded(dev, 4 * w)
    st = torch.cuda.current_stream(dev).cuda_stream
    assert lib.wsi_edt_rows(native.C.c_void_p(ws.data_ptr()), need, w, 1, native.C.c_void_p(out_bytes.data_ptr()), 4 * w, st) == 0
    got = out_bytes.view(torch.int32).cpu().numpy()
    assert got[w - 1] == 2147352578 == 2 * 32767 ** 2 and got[0] == 32767 ** 2
    assert np.array_equal(got, O.rows_single(g))
    whole = out_buf.cpu().numpy()
    assert (whole[:FRONT] == GUARD).all() and (whole[FRONT + 4 * w:] == GUARD).all()
    assert np.array_equal(ws_buf.cpu().numpy(), before)         # the row entry only reads the workspace
    # a plane of three rows, the middle one without a finite value
    plane = np.full((3, D.g_pitch(40)), 0x1234, np.uint16)       # the values past W of a row are never used
    plane[:, :40] = O.G_NONE
    plane[0, 7], plane[2, 39], plane[2, 0] = 5, 0, 3
    ws3 = torch.from_numpy(plane.view(np.uint8).reshape(-1)).to(dev)
    pad = torch.zeros(lib.wsi_edt_workspace_bytes(40, 3) - ws3.numel(), dtype=torch.uint8, device=dev)
    ws3 = torch.cat([ws3, pad])
    out = torch.full((3, 40), -1, dtype=torch.int32, device=dev)
    assert lib.wsi_edt_rows(native.C.c_void_p(ws3.data_ptr()), ws3.numel(), 40, 3, native.C.c_void_p(out.data_ptr()), 160, st) == 0
    assert np.array_equal(out.cpu().numpy(), O.rows_from_g(plane[:, :40]))
    assert (out[1] == O.EDT_NONE).all()


def test_columns_alone_equal_the_specs_g(dev):
    lib = native.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    for (h, w), density, invert in (((3 * F.BAND + 7, 300), 0.003, False), ((F.BAND + 1, 17), 0.05, True), ((1, 70), 0.2, False)):
        m = F.random_map(h, w, density, h + w)
        view, buf, host = place(dev, m, 3, 5)
        need = lib.wsi_edt_workspace_bytes(w, h)
        ws_buf, ws = guarded(dev, need)
        assert lib.wsi_edt_columns(native.C.c_void_p(view.data_ptr()), w, h, w + 5, int(invert), native.C.c_void_p(ws.data_ptr()), need, st) == 0
        whole = ws_buf.cpu().numpy()
        plane = whole[FRONT:FRONT + 2 * h * D.g_pitch(w)].view(np.uint16).reshape(h, D.g_pitch(w))
        assert np.array_equal(plane[:, :w], O.column_distances(m, invert))
        assert (whole[:FRONT] == GUARD).all() and (whole[FRONT + need:] == GUARD).all() and np.array_equal(buf.cpu().numpy(), host)


# ------------------------------------------------------------------------------------------------------------- the Python layer
def two_masks():
    a = (F.disc(90, 120, 40, 50, 22) | F.disc(90, 120, 55, 80, 12)).astype(np.uint8)
    a[40, 50] = 0
    b = (F.disc(90, 120, 44, 56, 20) | F.disc(90, 120, 12, 100, 4)).astype(np.uint8)
    return a, b


def test_morph_disc_and_margin_band_equal_the_spec(dev):
    a, _ = two_masks()
    a[0:6, 0:9] = 1                                             # a piece on the border: erosion does not eat it from outside
    t = torch.from_numpy(a).to(dev)
    for r in (0, 1, 5):
        for op in ('dilate', 'erode', 'open', 'close'):
            got = D.morph_disc(t, r, op)
            assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), O.morph_disc(a, r, op)), (r, op)
    assert D.morph_disc(t, 5, 'erode')[0, 0] == 1 and D.morph_disc(torch.ones((20, 30), dtype=torch.uint8, device=dev), 7, 'erode').all()
    for inner, outer in ((0, 0), (2, 0), (0, 3), (4, 9)):
        got = D.margin_band(t, inner, outer)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), O.margin_band(a, inner, outer)), (inner, outer)
    assert int(D.margin_band(t, 4, 9).sum()) > 500
    assert np.array_equal(D.margin_band(t > 0, 4, 9).cpu().numpy(), O.margin_band(a, 4, 9))


def test_surface_distances_equal_the_spec(dev):
    a, b = two_masks()
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    want = O.surface_distances(a, b)
    assert want['n_a'] > 100 and want['n_b'] > 100 and want['hd'] > want['hd95'] > want['assd'] > 0
    assert D.surface_distances(ta, tb) == want and D.surface_distances(tb, ta)['hd'] == want['hd']
    assert D.surface_distances(ta, tb, spacing=0.25) == O.surface_distances(a, b, spacing=0.25)
    same = D.surface_distances(ta, ta)
    assert (same['hd'], same['hd95'], same['assd']) == (0.0, 0.0, 0.0) and same['n_a'] == same['n_b'] == want['n_a']
    z = torch.zeros_like(ta)
    assert D.surface_distances(z, z) == {'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'n_a': 0, 'n_b': 0} == O.surface_distances(a * 0, a * 0)
    one = D.surface_distances(ta, z)
    assert one['hd'] == one['hd95'] == one['assd'] == math.inf and (one['n_a'], one['n_b']) == (want['n_a'], 0) and one == O.surface_distances(a, a * 0)
    assert D.surface_distances(z, tb)['assd'] == math.inf


# ------------------------------------------------------------------------------------------------------------------------ the hook
GREYS = (225, 165, 105, 45)                                      # the slide's grey of class 0 .. 3


def test_predict_wsis_boundary_scores(dev, tmp_path, monkeypatch):
    """an ArraySlide whose 16 x 16 blocks carry the grey of a class and a one-layer dense model that reads the grey, as
    tests/test_gpu_annotations.py drives predict_wsis: the three scores are the spec's on the returned bed and the ground-truth bed,
    0.0 where the ground truth is the returned bed, and absent - the keys of before - with the flag unset"""
    import myargs
    import utils.dataset as ds
    import utils.eval as val
    from PIL import Image
    for k, v in (('scan_level', 0), ('scan_resize', 1), ('num_classes', 4), ('class_probs', [0., 0., 0., 0.]), ('tile_w', 64), ('tile_h', 64),
                 ('tile_stride_w', 64), ('tile_stride_h', 64), ('val_save_pth', str(tmp_path / 'out')), ('wsi_mask_pth', str(tmp_path / 'nomask'))):
        monkeypatch.setattr(myargs.args, k, v)
    args = myargs.args
    os.makedirs(str(tmp_path / 'nomask'))
    Image.fromarray(np.full((48, 64), 255, np.uint8)).save(str(tmp_path / 'nomask' / 'case.svs.png'))     # every tile is foreground
    gt = CF.blob_map(48, 64, 3, 33, radius=3)
    gt[20:40, 20:50] = 3                                        # a tumour large enough to survive the 20 x 20 opening
    l2 = np.repeat(np.asarray(GREYS, np.uint8)[gt][..., None], 3, -1)
    slide = ArraySlide([np.repeat(np.repeat(l2, 16, 0), 16, 1), np.repeat(np.repeat(l2, 4, 0), 4, 1), l2], [1.0, 4.0, 16.0])
    slide.name = 'case.svs'
    centres = torch.tensor([(g / 255.0 - args.dataset_mean[0]) / args.dataset_std[0] for g in GREYS], device=dev)

    class ReadsTheGrey(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):                                     # (B, 3, h, w) -> (B, 4, h, w): minus the distance to each class's grey
            return -(x[:, :1] - centres.view(1, 4, 1, 1)).abs()

    model = ReadsTheGrey().to(dev)
    params = {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}
    tb_gt = np.zeros((48, 64), np.uint8)
    tb_gt[14:38, 24:58] = 255                                   # a bed the pathologist drew elsewhere

    def run(tb, **kw):
        dataset = ds.Dataset_wsis({'case.svs': slide}, params, bs=64)
        dataset.wsis['case.svs']['gt'] = torch.from_numpy(gt).to(dev)
        dataset.wsis['case.svs']['tb_gt'] = tb
        return val.predict_wsis(model, dataset, 1, save=False, **kw)['case.svs']

    plain = run(torch.from_numpy(tb_gt).to(dev))
    parent_keys = {'acc', 's', 'acc_masked', 's_masked', 'iou_fg', 'iou_tb'}
    assert set(plain['scores']) == parent_keys
    res = run(torch.from_numpy(tb_gt).to(dev), boundary_scores=True)
    bed = res['tumor_bed'].cpu().numpy()
    assert bed.any() and torch.equal(res['tumor_bed'], plain['tumor_bed'])
    sc = res['scores']
    assert set(sc) == parent_keys | {'hd_tb', 'hd95_tb', 'assd_tb'}            # the slide states no mpp: no '_um' keys
    assert {k: sc[k] for k in parent_keys} == plain['scores']
    want = O.surface_distances(bed, tb_gt)
    assert want['hd'] >= want['hd95'] >= want['assd'] > 0
    assert (sc['hd_tb'], sc['hd95_tb'], sc['assd_tb']) == (want['hd'], want['hd95'], want['assd'])
    slide.mpp = 0.25                                            # stated: microns = pixels * mpp * the level's step
    um = run(tb_gt, boundary_scores=True)['scores']             # (a host array as tb_gt goes the same way)
    assert set(um) == parent_keys | {'hd_tb', 'hd95_tb', 'assd_tb', 'hd_tb_um', 'hd95_tb_um', 'assd_tb_um'}
    assert (um['hd_tb'], um['hd95_tb_um'], um['assd_tb_um']) == (want['hd'], want['hd95'] * 4.0, want['assd'] * 4.0) and um['hd_tb_um'] == want['hd'] * 4.0
    del slide.mpp
    exact = run(res['tumor_bed'], boundary_scores=True)['scores']
    assert (exact['hd_tb'], exact['hd95_tb'], exact['assd_tb']) == (0.0, 0.0, 0.0) and abs(exact['iou_tb'] - 1) <= 1e-6
    # without tb_gt the flag adds nothing
    dataset = ds.Dataset_wsis({'case.svs': slide}, params, bs=64)
    dataset.wsis['case.svs']['gt'] = torch.from_numpy(gt).to(dev)
    assert set(val.predict_wsis(model, dataset, 1, save=False, boundary_scores=True)['case.svs']['scores']) == parent_keys
