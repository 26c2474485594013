"""CPU side of the region tables: the run rule (tests/regions_oracle.py) against a brute-force flood fill, against SciPy and against
the boundary tracer's spec, hand-written tables, the host layer of wsi_segmentation_pipeline_amd.regions with the spec standing in for
the device, the C-ABI entries, their argument checks and the documented workspace layout, and the shared per-run arithmetic
(csrc/regions_dev.h) as a stand-alone program under the host sanitizers, equal to the spec on the whole corpus."""
import ctypes as C
import csv
import math
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contour_fixture as CF                                   # noqa: E402
import contours_oracle as CO                                   # noqa: E402
import region_fixture as RF                                    # noqa: E402
import regions_oracle as O                                     # noqa: E402
from wsi_segmentation_pipeline_amd import native, regions as R      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = O.F


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


# ---------------------------------------------------------------------------------------------------------------------- the spec
def test_run_rule_equals_the_flood_fill():
    cases = RF.random_cases(220) + RF.shape_cases()
    assert sum(c.get('classes') is not None and 0 in c['classes'] for c in cases) >= 30
    regions = 0
    for c in cases:
        for conn in (4, 8):
            r = O.label(c['m'], c.get('classes'), conn, c.get('weight'))
            lab, stats = O.flood(c['m'], c.get('classes'), conn)
            assert np.array_equal(r.labels, lab), (c['name'], conn)
            assert np.array_equal(r.table, O.table_from_labels(c['m'], lab, c.get('weight'))), (c['name'], conn)
            assert [(int(a), int(p)) for a, p in zip(r.area, r.perim)] == stats
            assert (r.table[:, F['reserved']] == 0).all() and r.table.dtype == np.int64 and r.labels.dtype == np.int32
            regions += r.n
    assert regions > 5000


def test_run_rule_equals_scipy():
    ndi = pytest.importorskip('scipy.ndimage')
    for c in RF.random_cases(60, seed=5) + RF.shape_cases() + [dict(name='blobs', m=CF.blob_map(60, 90, 3, 2))]:
        m = c['m']
        for conn in (4, 8):
            r = O.label(m, None, conn)
            structure = np.ones((3, 3), int) if conn == 8 else None
            total = 0
            for cls in sorted(set(np.unique(m).tolist()) - {0}):
                lab, n = ndi.label(m == cls, structure)
                ours = np.where(m == cls, r.labels, 0)
                pairs = np.unique(np.stack([lab[lab > 0], ours[lab > 0]], 1), axis=0)
                assert len(pairs) == n == len(np.unique(pairs[:, 1])), (c['name'], conn, cls)       # the same partition
                ids = pairs[np.argsort(pairs[:, 0]), 1] - 1
                idx = np.arange(1, n + 1)
                yy, xx = np.mgrid[0:m.shape[0], 0:m.shape[1]]
                assert np.array_equal(r.area[ids], ndi.sum(np.ones_like(lab), lab, idx).astype(np.int64))
                assert np.array_equal(r.sx[ids], ndi.sum(xx, lab, idx).astype(np.int64)) and np.array_equal(r.sy[ids], ndi.sum(yy, lab, idx).astype(np.int64))
                for k, sl in enumerate(ndi.find_objects(lab)):
                    assert r.table[ids[k], F['x0']:F['y1'] + 1].tolist() == [sl[1].start, sl[0].start, sl[1].stop, sl[0].stop]
                total += n
            assert total == r.n


def test_connectivity_4_regions_are_what_the_tracer_outlines():
    checks = 0
    for c in CF.random_cases(120):
        r = O.label(c['m'], c['classes'], 4)
        t = CO.trace(c['m'], c['classes'], c['step'], c['origin'], c['bounds'])
        for cls in np.nonzero(O.traced_table(c['classes']))[0].tolist():
            mine, loops = r.cls == cls, np.asarray(t.label) == cls
            a2, edges = np.asarray(t.area2)[loops], np.asarray(t.edges)[loops]
            assert int(mine.sum()) == int((a2 > 0).sum())
            assert 2 * int(r.area[mine].sum()) == int(a2.sum())
            assert int(r.perim[mine].sum()) == int(edges.sum())
            checks += 1
    assert checks >= 200


# ------------------------------------------------------------------------------------------------------------------ tables by hand
def rec(**k):
    return [k.get(f, 0) for f in O.FIELDS]


def test_hand_written_tables():
    one = np.zeros((3, 4), np.uint8)
    one[1, 2] = 7
    assert O.label(one).table.tolist() == [rec(area=1, x0=2, y0=1, x1=3, y1=2, sx=2, sy=1, sxx=4, sxy=2, syy=1, perim=4, first=6, cls=7)]
    block = np.zeros((4, 5), np.uint8)
    block[1:3, 1:4] = 2
    assert O.label(block, weight=np.full((4, 5), 10, np.uint8)).table.tolist() == [
        rec(area=6, x0=1, y0=1, x1=4, y1=3, sx=12, sy=9, sxx=28, sxy=18, syy=15, perim=10, wsum=60, first=6, cls=2)]
    ring = np.ones((3, 3), np.uint8)
    ring[1, 1] = 0
    assert O.label(ring).table.tolist() == [rec(area=8, x1=3, y1=3, sx=8, sy=8, sxx=14, sxy=8, syy=14, perim=16, cls=1, border=1)]     # 12 outside + 4 round the hole
    both = O.label(ring, [0, 1])
    assert both.n == 2 and both.table[1].tolist() == rec(area=1, x0=1, y0=1, x1=2, y1=2, sx=1, sy=1, sxx=1, sxy=1, syy=1, perim=4, first=4)
    diag = np.zeros((4, 4), np.uint8)
    diag[1, 1] = diag[2, 2] = 1
    assert O.label(diag, connectivity=8).table.tolist() == [rec(area=2, x0=1, y0=1, x1=3, y1=3, sx=3, sy=3, sxx=5, sxy=5, syy=5, perim=8, first=5, cls=1)]
    four = O.label(diag, connectivity=4)
    assert four.n == 2 and four.first.tolist() == [5, 10] and four.labels[2, 2] == 2 and four.perim.tolist() == [4, 4]
    anti = np.zeros((2, 2), np.uint8)
    anti[0, 1] = anti[1, 0] = 1
    assert O.label(anti, connectivity=8).n == 1 and O.label(anti, connectivity=4).n == 2
    two = np.zeros((2, 2), np.uint8)
    two[0, 0], two[1, 1] = 1, 2                                  # a corner is shared, the class is not
    assert O.label(two, connectivity=8).n == 2
    for y, x in ((0, 2), (2, 0), (4, 2), (2, 4)):                # a pixel on each border, and one inside
        m = np.zeros((5, 5), np.uint8)
        m[y, x] = m[2, 2] = 1
        assert O.label(m).border.tolist() == ([1, 0] if (y, x) < (2, 2) else [0, 1])
    empty = O.label(np.zeros((3, 3), np.uint8))
    assert empty.n == 0 and empty.table.shape == (0, 16) and not empty.labels.any()


def test_axes_of_a_rectangle():
    m = np.zeros((30, 40), np.uint8)
    m[5:11, 7:31] = 1                                           # 24 wide, 6 high: the moments of a uniform a x b rectangle are a^2 / 12, b^2 / 12
    m[20:28, 3:5] = 2                                           # 2 wide, 8 high: the major axis is vertical
    r = R.Regions(torch.from_numpy(O.label(m).table), None, (40, 30))
    major, minor, angle = r.axes()
    assert np.allclose(major, [4 * math.sqrt(24 * 24 / 12), 4 * math.sqrt(8 * 8 / 12)], rtol=1e-12)
    assert np.allclose(minor, [4 * math.sqrt(6 * 6 / 12), 4 * math.sqrt(2 * 2 / 12)], rtol=1e-12)
    assert abs(angle[0]) < 1e-12 and abs(abs(angle[1]) - math.pi / 2) < 1e-12
    assert np.allclose(r.centroid(), [[18.5, 7.5], [3.5, 23.5]])
    assert all(np.allclose(a, b) for a, b in zip(r.axes(), O.axes(O.label(m).table)))


# ------------------------------------------------------------------------------------- the host layer, the spec in the device's place
@pytest.fixture
def spec_device(monkeypatch):
    def label(m, classes=None, connectivity=8, labels=True, weight=None, **kw):
        assert m.dtype == torch.uint8 and not kw
        r = O.label(m.numpy(), classes, connectivity, None if weight is None else weight.numpy())
        return R.Regions(torch.from_numpy(r.table), torch.from_numpy(r.labels) if labels else None, m.shape[::-1], len(r.runs))
    monkeypatch.setattr(R, 'label', label)


def test_lesion_scores_by_hand(spec_device):
    gt = np.zeros((12, 30), np.uint8)
    gt[1:5, 1:5] = 2                                            # g1: 16 px
    gt[1:5, 10:14] = 3                                          # g2: 16 px
    gt[8:10, 20:24] = 2                                         # g3: 8 px
    pred = np.zeros((12, 30), np.uint8)
    pred[1:5, 1:5] = 3                                          # p1 = g1 exactly (the class within the foreground does not matter): IoU 1
    pred[1:5, 12:20] = 2                                        # p2: 32 px, shares 8 with g2: IoU 8 / 40
    pred[8:10, 22:26] = 2                                       # p3: 8 px, shares 4 with g3: IoU 4 / 12 = 1 / 3
    pred[11, 0:3] = 1                                           # class 1 is no lesion under classes=(2, 3)
    t = lambda a: torch.from_numpy(a)
    got = R.lesion_scores(t(pred), t(gt), classes=(2, 3))
    assert got == dict(n_pred=3, n_gt=3, tp_pred=1, tp_gt=1, fp=2, fn=2, precision=1 / 3, recall=1 / 3, f1=1 / 3) == O.lesion_scores(pred, gt, (2, 3))
    assert R.lesion_scores(t(pred), t(gt), classes=(2, 3), iou=1 / 3)['tp_gt'] == 2           # 4 * 3 >= 1 * 12: the integers decide
    assert R.lesion_scores(t(pred), t(gt), classes=(2, 3), iou=0.334)['tp_gt'] == 1
    assert R.lesion_scores(t(pred), t(gt), classes=(2, 3), iou=0)['tp_pred'] == 3
    assert R.lesion_scores(t(pred), t(gt), iou=0)['n_pred'] == 4                             # every non-zero class
    assert R.lesion_scores(t(pred), t(gt), classes=(2, 3), iou=0, min_area=9) == O.lesion_scores(pred, gt, (2, 3), iou=0, min_area=9)
    assert R.lesion_scores(t(pred), t(gt), classes=(2, 3), iou=0, min_area=9)['n_gt'] == 2
    # an IoU of exactly 1 / 2: 8 shared of 8 + 16 - 8
    a, b = np.zeros((4, 8), np.uint8), np.zeros((4, 8), np.uint8)
    a[0:2, 0:4], b[0:4, 0:4] = 1, 1
    assert R.lesion_scores(t(a), t(b))['tp_gt'] == 1 and R.lesion_scores(t(a), t(b), iou=0.501)['tp_gt'] == 0
    # the empty rules
    z = np.zeros((4, 8), np.uint8)
    assert R.lesion_scores(t(z), t(z)) == dict(n_pred=0, n_gt=0, tp_pred=0, tp_gt=0, fp=0, fn=0, precision=1.0, recall=1.0, f1=1.0)
    none = R.lesion_scores(t(z), t(b))
    assert (none['precision'], none['recall'], none['f1'], none['fn']) == (0.0, 0.0, 0.0, 1)
    extra = R.lesion_scores(t(a), t(z))
    assert (extra['precision'], extra['recall'], extra['f1'], extra['fp']) == (0.0, 0.0, 0.0, 1)
    with pytest.raises(ValueError):
        R.lesion_scores(t(a), t(b), iou=1.5)


def test_slide_positive_threshold(spec_device, monkeypatch):
    from oracle import postprocess_oracle as PO
    from wsi_segmentation_pipeline_amd import postprocess as PP
    assert R.heat_threshold(0.99) == 253 == math.ceil(0.99 * 255) and R.heat_threshold(0.9) == 230 and R.heat_threshold(1.0) == 255
    monkeypatch.setattr(PP, 'morph_rect', lambda img, k, op: torch.from_numpy(PO.morph_open(img.numpy(), k)) if op == 'open' else 1 / 0)
    heat = np.zeros((80, 90), np.uint8)
    heat[10:65, 20:75] = 252                                    # 55 x 55 of 252: just under 0.99 * 255 = 252.45
    out = R.slide_positive(torch.from_numpy(heat))
    assert out == dict(positive=False, fraction=0.0, n_regions=0, largest_area=0)
    heat[10:65, 20:75] = 253
    heat[70:75, 0:5] = 255                                      # a speck the 50 x 50 opening removes
    out = R.slide_positive(torch.from_numpy(heat))
    assert out == dict(positive=True, fraction=55 * 55 / (80 * 90), n_regions=1, largest_area=55 * 55) == O.slide_positive(heat)[0]
    assert R.slide_positive(torch.from_numpy(heat), min_fraction=0.5)['positive'] is False
    assert R.slide_positive(torch.from_numpy(heat), open_k=3)['n_regions'] == 2
    for v in range(256):                                        # the integer comparison is the reference's float one
        assert (v >= R.heat_threshold(0.99)) == bool(np.uint8(v) >= 0.99 * 255)


def test_remove_small_overlaps_rows_and_csv(spec_device, tmp_path):
    m = CF.blob_map(40, 50, 3, 8, radius=2)
    t = torch.from_numpy(m)
    for conn, classes, fill in ((8, None, 0), (4, (2, 3), 9)):
        got = R.remove_small(t, 12, conn, classes, fill).numpy()
        assert np.array_equal(got, O.remove_small(m, 12, conn, classes, fill)) and (got != m).any()
        r = O.label(got, classes, conn)
        assert (r.area >= 12).all() or fill != 0
    assert torch.equal(R.remove_small(torch.zeros((3, 3), dtype=torch.uint8), 5), torch.zeros((3, 3), dtype=torch.uint8))
    other = CF.blob_map(40, 50, 3, 9, radius=2)
    ra, rb = R.label(t), R.label(torch.from_numpy(other), connectivity=4)
    got = R.overlaps(ra, rb).numpy()
    assert got.dtype == np.int64 and np.array_equal(got, O.overlaps(ra.labels.numpy(), rb.labels.numpy())) and len(got) > 5
    assert got[:, 2].sum() == ((m > 0) & (other > 0)).sum() and np.array_equal(got, got[np.lexsort((got[:, 1], got[:, 0]))])
    assert R.overlaps(ra.labels, torch.zeros_like(ra.labels)).shape == (0, 3)
    # rows and the CSV: level-0 coordinates and square microns
    two = np.zeros((6, 8), np.uint8)
    two[1:3, 2:6] = 3
    two[4, 0] = 1
    w = np.full((6, 8), 100, np.uint8)
    r = R.label(torch.from_numpy(two), weight=torch.from_numpy(w))
    rows = r.rows(step=16, origin=(5, -3), mpp=0.25)
    assert rows[0] == {'id': 1, 'class': 3, 'area_px': 8, 'area_um2': 8 * 16 * 16 * 0.0625, 'x0': 5 + 32, 'y0': -3 + 16, 'x1': 5 + 96, 'y1': -3 + 48,
                       'cx': 5 + 4.0 * 16, 'cy': -3 + 2.0 * 16, 'perim': 12, 'major': rows[0]['major'], 'minor': rows[0]['minor'], 'mean_weight': 100.0}
    assert abs(rows[0]['major'] - 4 * math.sqrt(16 / 12)) < 1e-12 and abs(rows[0]['minor'] - 4 * math.sqrt(4 / 12)) < 1e-12
    assert rows[1]['class'] == 1 and rows[1]['x0'] == 5 and rows[1]['cx'] == 5 + 8.0 and r.rows()[1]['area_um2'] is None
    path = R.write_csv(str(tmp_path / 'r.csv'), r, 16, (5, -3), 0.25, {3: 'Invasive'})
    back = list(csv.DictReader(open(path)))
    assert list(back[0]) == list(R.CSV_COLUMNS) and len(back) == 2
    assert (back[0]['name'], back[0]['area_um2'], back[0]['x1'], back[0]['cx'], back[1]['name']) == ('Invasive', '128.0000', '101', '69.0000', '')
    assert list(csv.DictReader(open(R.write_csv(str(tmp_path / 'n.csv'), r))))[0]['area_um2'] == ''
    assert r.box.tolist() == [[2, 1, 6, 3], [0, 4, 1, 5]] and r.cls.tolist() == [3, 1] and r.border.tolist() == [0, 1] and r.wsum.tolist() == [800, 100]


def test_label_refuses_what_it_cannot_take():
    with pytest.raises(RuntimeError):
        R.label(torch.zeros((4, 5), dtype=torch.uint8))           # no device, no fallback
    for bad in (torch.zeros((4, 5), dtype=torch.int32), torch.zeros((2, 4, 5), dtype=torch.uint8), torch.zeros((4, 10), dtype=torch.uint8)[:, ::2],
                np.zeros((4, 5), np.uint8)):
        with pytest.raises(ValueError):
            R.label(bad)
    with pytest.raises(ValueError):
        R.label(torch.zeros((4, 5), dtype=torch.uint8), connectivity=6)
    with pytest.raises(ValueError):
        R.label(torch.zeros((4, 5), dtype=torch.uint8), classes=[256])


# ------------------------------------------------------------------------------------------------------------------ the C entries
NAMES = {'wsi_region_count_workspace_bytes', 'wsi_region_workspace_bytes', 'wsi_region_count', 'wsi_region_runs', 'wsi_region_link', 'wsi_region_rank',
         'wsi_region_table', 'wsi_region_paint'}


def test_entries_declared_mirrored_and_checked(lib):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read(), flags=re.S)
    assert set(re.findall(r'\b(wsi_region_[a-z0-9_]+)\s*\(', hdr)) == {n for n in native.SIGNATURES if n.startswith('wsi_region_')} == NAMES
    assert all(hasattr(lib, n) for n in NAMES)
    for n in NAMES:                                             # argument counts of the header and of the ctypes mirror agree
        args = re.search(r'\b%s\s*\(([^)]*)\)' % n, hdr).group(1)
        assert len(args.split(',')) == len(native.SIGNATURES[n][1]), n
    assert int(re.search(r'#define WSI_HIP_ABI_VERSION (\d+)', hdr).group(1)) == native.ABI_VERSION == 9       # additive: the version stays
    mk = open(os.path.join(native.CSRC, 'Makefile')).read()
    assert re.search(r'^SRCS\s*=.*\bregions\.hip\b', mk, re.M) and re.search(r'^build/%\.o:.*\bregions_dev\.h\b', mk, re.M)
    assert "'regions'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    # every check comes before any device work, so the entries answer without a GPU.  Fake, aligned addresses.
    P = lambda a: C.c_void_p(a)
    table = (C.c_uint8 * 256)(*([0] + [1] * 255))
    M, WS, CWS, N, OUT = P((1 << 21) + 3), P(1 << 22), P(1 << 20), P(1 << 19), P(1 << 23)
    need = lib.wsi_region_workspace_bytes(64, 48, 100)
    big = dict(bytes=1 << 40)

    def count(**k):
        return lib.wsi_region_count(k.get('map', M), k.get('W', 64), k.get('H', 48), k.get('pitch', 69), k.get('table', table), k.get('cws', CWS),
                                    k.get('n', N), None)
    for k in (dict(map=None), dict(table=None), dict(cws=None), dict(n=None), dict(W=0), dict(H=0), dict(W=-2), dict(W=32769, pitch=40000), dict(H=32769),
              dict(pitch=63), dict(cws=P((1 << 20) + 2)), dict(n=P((1 << 19) + 1))):
        assert count(**k) == -22, k

    def runs(**k):
        return lib.wsi_region_runs(k.get('map', M), k.get('W', 64), k.get('H', 48), k.get('pitch', 69), k.get('table', table), k.get('cws', CWS),
                                   k.get('n', 100), k.get('ws', WS), k.get('bytes', need), None)
    for k in (dict(map=None), dict(table=None), dict(cws=None), dict(ws=None), dict(W=0), dict(H=32769, **big), dict(pitch=63), dict(n=0), dict(n=64 * 48 + 1, **big),
              dict(bytes=need - 1), dict(ws=P((1 << 22) + 8))):
        assert runs(**k) == -22, k
    for fn in (lib.wsi_region_link, lambda *a: lib.wsi_region_rank(*a[:-1], N, a[-1])):
        def call(**k):
            return fn(k.get('ws', WS), k.get('bytes', need), k.get('W', 64), k.get('H', 48), k.get('n', 100), k.get('conn', 8), None)
        for k in (dict(ws=None), dict(bytes=need - 1), dict(W=0), dict(H=0), dict(W=32769, **big), dict(n=0), dict(conn=6), dict(conn=0), dict(conn=-4),
                  dict(ws=P((1 << 22) + 4))):
            assert call(**k) == -22, k
    assert lib.wsi_region_rank(WS, need, 64, 48, 100, 8, None, None) == -22

    def tab(**k):
        return lib.wsi_region_table(k.get('ws', WS), k.get('bytes', need), k.get('W', 64), k.get('H', 48), k.get('n', 100), k.get('regions', 7),
                                    k.get('weight', None), k.get('wpitch', 0), k.get('table', OUT), None)
    for k in (dict(ws=None), dict(table=None), dict(bytes=need - 1), dict(W=0), dict(n=0), dict(regions=0), dict(regions=101), dict(table=P((1 << 23) + 4)),
              dict(weight=M, wpitch=63)):
        assert tab(**k) == -22, k

    def paint(**k):
        return lib.wsi_region_paint(k.get('ws', WS), k.get('bytes', need), k.get('W', 64), k.get('H', 48), k.get('n', 100), k.get('out', OUT),
                                    k.get('pitch', 256), None)
    for k in (dict(ws=None), dict(out=None), dict(bytes=need - 1), dict(H=0), dict(n=0), dict(pitch=252), dict(pitch=258), dict(out=P((1 << 23) + 2))):
        assert paint(**k) == -22, k


def test_workspace_sizes_are_the_documented_ones(lib):
    dev_h = open(os.path.join(native.CSRC, 'regions_dev.h')).read()
    assert 'constexpr int LIMIT = 32768;' in dev_h and 'constexpr int CHUNK = 1024;' in dev_h and 'constexpr int RECORD_WORDS = 16;' in dev_h
    assert (R.LIMIT, RF.CHUNK, O.CHUNK, O.LIMIT) == (32768, 1024, 1024, 32768) and R.FIELDS == O.FIELDS and len(R.FIELDS) == 16
    src = open(os.path.join(native.CSRC, 'regions.hip')).read()                 # the scan is the shared one: its constants are map_kernels.h's,
    assert 'wsi_map::CHUNK == CHUNK' in src                                     # pinned to the layout's chunk where both are visible
    consts = dict(re.findall(r'constexpr int (\w+) = ([^;]+);', open(os.path.join(native.CSRC, 'map_kernels.h')).read()))
    assert int(consts['THREADS']) * int(consts['PER_THREAD']) == RF.CHUNK and consts['SUMS_TILE'] == 'THREADS * SUMS_PER_LANE'
    assert int(consts['THREADS']) * int(consts['SUMS_PER_LANE']) == RF.SCAN_SPAN and RF.SCAN_SECOND == 256 * RF.CHUNK
    fields = re.search(r'enum Field \{([^}]*)\}', dev_h).group(1).replace('= 0', '').replace('BOX_', '').lower().split(',')
    assert tuple(f.strip() for f in fields) == O.FIELDS
    hdr = open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read()
    for word in ('runs ', 'row_first', 'parent', 'up ', 'root', 'flag', 'rank', 'id ', 'sums'):
        assert re.search(r'^ \*     %s' % word, hdr, re.M), word
    r256 = lambda b: (b + 255) // 256 * 256
    for w, h, n in ((1, 1, 1), (64, 48, 100), (1024, 3, 1023), (1025, 3, 1025), (2048, 1536, 262144), (2048, 1536, 262145), (32768, 32768, 1 << 30)):
        want = r256(16 * n) + r256(4 * (h + 1)) + 4 * r256(4 * n) + 2 * r256(4 * (n + 1)) + r256(4 * (-(-n // 1024) + 1))
        assert lib.wsi_region_workspace_bytes(w, h, n) == want, (w, h, n)
        assert lib.wsi_region_count_workspace_bytes(w, h) == r256(4 * (h * -(-w // 1024) + 1))
    for w, h, n in ((0, 5, 1), (5, 0, 1), (32769, 1, 1), (1, 32769, 1), (4, 4, 0), (4, 4, 17)):
        assert lib.wsi_region_workspace_bytes(w, h, n) == 0
    assert lib.wsi_region_count_workspace_bytes(0, 1) == lib.wsi_region_count_workspace_bytes(1, 32769) == 0


# ----------------------------------------------------------------------------------- the shared arithmetic under the sanitizers
def san_cases():
    cases = [dict(c, kind=0) for c in RF.random_cases(200)]
    cases += [dict(c, kind=0, classes=None, connectivity=(4, 8)[k % 2], weight=np.full(c['m'].shape, 255, np.uint8)) for k, c in enumerate(RF.shape_cases())]
    wide = np.zeros((3, 2100), np.uint8)
    wide[1, 1000:1030] = 1                                      # a run across one chunk border
    wide[2, 5:2079] = 2                                         # and across two
    wide[0, 1023], wide[0, 1024] = 3, 4                         # an end and a start at the border itself
    cases.append(dict(name='chunk borders', m=wide, classes=None, connectivity=8, weight=None, kind=0))
    cases.append(dict(name='one row', m=np.ones((1, 32768), np.uint8), classes=None, connectivity=8, weight=np.full((1, 32768), 255, np.uint8), kind=0))
    cases.append(dict(name='one column', m=np.ones((32768, 1), np.uint8), classes=None, connectivity=4, weight=None, kind=0))
    cases.append(dict(name='largest operands', runs=[(32767, 0, 32768), (32767, 32767, 32768), (0, 0, 1), (32767, 1, 32768)], kind=1))
    return cases


@pytest.fixture(scope='module')
def sanitizer_run(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('regions_san')
    exe = str(d / 'regions_san')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
           os.path.join(ROOT, 'tests', 'regions_san_main.cpp'), '-o', exe]
    if os.path.basename(cxx) == 'g++':
        cmd += ['-static-libasan', '-static-libubsan']          # the runtimes inside the program: nothing has to be preloaded or come first
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode:
        if re.search(r'cannot find .*(asan|ubsan)|libasan|libubsan', res.stdout):
            pytest.skip('the sanitizer runtime is not installed')
        raise AssertionError(res.stdout)
    cases = san_cases()
    with open(d / 'corpus.bin', 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for k, c in enumerate(cases):
            if c['kind'] == 1:
                f.write(struct.pack('<8i', 1, 0, 0, 0, 0, 0, 0, len(c['runs'])) + np.asarray(c['runs'], '<i4').tobytes())
                continue
            h, w = c['m'].shape
            f.write(struct.pack('<8i', 0, w, h, c['connectivity'], (0, 1, 3, 8, 15)[k % 5], w + (0, 5, 16)[k % 3], int(c['weight'] is not None), 0))
            f.write(O.traced_table(c['classes']).tobytes() + np.ascontiguousarray(c['m']).tobytes())
            if c['weight'] is not None:
                f.write(np.ascontiguousarray(c['weight']).tobytes())
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    res = subprocess.run([exe, str(d / 'corpus.bin'), str(d / 'results.bin')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0, res.stdout[-4000:]
    assert 'runtime error' not in res.stdout and 'Sanitizer' not in res.stdout, res.stdout[-4000:]
    raw = open(d / 'results.bin', 'rb').read()
    results, at = [], 0
    for c in cases:
        if c['kind'] == 1:
            results.append(np.frombuffer(raw, '<i8', 6 * len(c['runs']), at).reshape(-1, 6))
            at += 48 * len(c['runs'])
            continue
        h, w = c['m'].shape
        n_runs, n = struct.unpack_from('<2I', raw, at)
        table = np.frombuffer(raw, '<i8', 16 * n, at + 8).reshape(n, 16)
        labels = np.frombuffer(raw, '<i4', h * w, at + 8 + 128 * n).reshape(h, w)
        results.append((n_runs, table, labels))
        at += 8 + 128 * n + 4 * h * w
    assert at == len(raw)
    return cases, results


def test_sanitized_walk_equals_the_spec(sanitizer_run):
    """the header the kernels compile, walked on the host the way the kernels' lanes walk a map, under ASan and UBSan: 0 differences from
    the spec's tables and label maps, case by case, and the largest operands the closed forms can meet"""
    cases, results = sanitizer_run
    assert len(cases) >= 210
    differences = regions = 0
    for c, got in zip(cases, results):
        if c['kind'] == 1:
            for (y, x0, x1), row in zip(c['runs'], got.tolist()):
                xs = range(x0, x1)
                assert row == [x1 - x0, sum(xs), y * (x1 - x0), sum(x * x for x in xs), y * sum(xs), y * y * (x1 - x0)]
            continue
        want = O.label(c['m'], c['classes'], c['connectivity'], c['weight'])
        differences += int(got[0] != len(want.runs)) + int(got[1].shape != want.table.shape or (got[1] != want.table).sum()) + int((got[2] != want.labels).sum())
        regions += want.n
        assert differences == 0, c['name']
    assert differences == 0 and regions > 3000
    by_name = {c['name']: r for c, r in zip(cases, results)}
    assert by_name['largest operands'][0].tolist() == [32768, 32767 * 32768 // 2, 32767 * 32768, 32767 * 32768 * 65535 // 6, 32767 * (32767 * 32768 // 2), 32767 ** 2 * 32768]
    row = by_name['one row'][1]
    assert row.shape == (1, 16) and row[0, F['wsum']] == 255 * 32768 and row[0, F['perim']] == 2 * 32768 + 2 and row[0, F['sxx']] == 32767 * 32768 * 65535 // 6
    col = by_name['one column']
    assert col[0] == 32768 and col[1].shape == (1, 16) and col[1][0, F['syy']] == 32767 * 32768 * 65535 // 6 and col[1][0, F['perim']] == 2 * 32768 + 2
    assert by_name['chunk borders'][0] == 4 and by_name['chunk borders'][1][:, F['area']].tolist() == [1, 1, 30, 2074]
