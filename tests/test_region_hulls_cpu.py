"""CPU side of the region hulls: the row rule (tests/region_hulls_oracle.py) against SciPy's ConvexHull and the brute-force definitions
of the diameters, against the boundary tracer's outer loops, hand-written records, the host layer of
wsi_segmentation_pipeline_amd.regions with the spec standing in for the device, the C-ABI entries, their argument checks and the
documented workspace size, and the shared arithmetic (csrc/region_hulls_dev.h) as a stand-alone program under the host sanitizers, equal
to the spec on the whole corpus."""
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
import contours_oracle as CO                                   # noqa: E402
import region_fixture as RF                                    # noqa: E402
import region_hulls_oracle as HO                               # noqa: E402
import regions_oracle as O                                     # noqa: E402
from wsi_segmentation_pipeline_amd import native, regions as R      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = HO.F


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


@pytest.fixture(scope='module')
def corpus():
    """[(name, connectivity, regions, hulls)] over the random and the named cases at both connectivities, made once"""
    out = []
    for c in RF.random_cases(120) + RF.shape_cases():
        for conn in (4, 8):
            r, h = HO.label(c['m'], c.get('classes'), conn)
            out.append((c['name'], conn, r, h, c))
    return out


# ---------------------------------------------------------------------------------------------------------------------- the spec
def test_spec_equals_scipy_and_the_brute_force_definitions(corpus):
    spatial = pytest.importorskip('scipy.spatial')
    regions = 0
    for name, conn, r, h, _ in corpus:
        assert h.table.dtype == np.int64 and h.vertices.dtype == np.int32 and h.table.shape == (r.n, 16) and not h.table[:, 11:].any()
        for k, points in enumerate(HO.corners_of(r)):
            v, rec = h.polys[k], h.table[k].tolist()
            hull = spatial.ConvexHull(np.asarray(points, np.float64))
            assert int(round(hull.volume * 2)) == rec[F['hull_area2']] and abs(hull.volume * 2 - rec[F['hull_area2']]) < 1e-6, (name, conn, k)
            assert len(hull.vertices) == len(v) == rec[F['hull_n']] and {points[i] for i in hull.vertices} == set(v) == HO.plain_hull(points), (name, conn, k)
            assert rec[F['hull_first']] == sum(len(p) for p in h.polys[:k])
            # the order: from the smallest (y, x), clockwise with y down, strictly convex, top and bottom edges horizontal
            n = len(v)
            assert n >= 4 and v[0] == min(v, key=lambda p: (p[1], p[0])) and v[1][1] == v[0][1] and v[1][0] > v[0][0]
            assert all(HO.cross(v[(i + 1) % n][0] - v[i][0], v[(i + 1) % n][1] - v[i][1], v[(i + 2) % n][0] - v[(i + 1) % n][0],
                                v[(i + 2) % n][1] - v[(i + 1) % n][1]) > 0 for i in range(n))
            bottom = max(p[1] for p in v)
            assert sum(p[1] == bottom for p in v) == 2
            # the diameters over ALL run corners of the region, not over the vertices
            assert HO.brute_feret_sq(points) == rec[F['feret_sq']]
            a, b = v[rec[F['feret_a']]], v[rec[F['feret_b']]]
            assert rec[F['feret_a']] < rec[F['feret_b']] and (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 == rec[F['feret_sq']]
            num, den = HO.brute_width(points, v)
            assert num * rec[F['width_den']] == rec[F['width_num']] * den and (num, den) == (rec[F['width_num']], rec[F['width_den']]), (name, conn, k)
            assert rec[F['hull_area2']] >= 2 * int(r.table[k, O.F['area']])
            assert 0 < rec[F['orth_num']] and rec[F['orth_num']] ** 2 <= rec[F['feret_sq']] * 4 * rec[F['feret_sq']]
            assert rec[F['width_num']] * rec[F['feret_sq']] <= rec[F['orth_num']] ** 2 * rec[F['width_den']]       # the least width is no wider
        regions += r.n
    assert regions >= 2900


def test_connectivity_4_hull_is_the_hull_of_the_traced_outer_loop(corpus):
    checked = 0
    for name, conn, r, h, c in corpus:
        if conn != 4:
            continue
        t = CO.trace(c['m'], c.get('classes'), 1, (0, 0))
        outer = {}
        for loop, a2 in zip(t.loops(), t.area2.tolist()):
            if a2 > 0:
                pts = [tuple(p) for p in loop.tolist()]
                outer[min(pts, key=lambda p: (p[1], p[0]))] = pts
        assert len(outer) == r.n
        w = c['m'].shape[1]
        for k in range(r.n):
            first = int(r.table[k, O.F['first']])
            assert HO.plain_hull(outer[(first % w, first // w)]) == set(h.polys[k]), (name, k)
            checked += 1
    assert checked > 1000


def rec(*words):
    return list(words) + [0] * (16 - len(words))


def test_hand_written_records():
    one = np.zeros((3, 4), np.uint8)
    one[1, 2] = 7
    r, h = HO.label(one)
    assert h.polys == [[(2, 1), (3, 1), (3, 2), (2, 2)]] and h.vertices.tolist() == [[2, 1], [3, 1], [3, 2], [2, 2]]
    assert h.table.tolist() == [rec(0, 4, 2, 2, 0, 2, 1, 1, 0, 2, 2)]          # feret_sq 2 from vertex 0 to 2, width 1 / 1 on edge 0, orth_num 2
    block = np.zeros((8, 8), np.uint8)
    block[1:6, 2:5] = 2                                         # 3 wide, 5 high
    r, h = HO.label(block)
    assert h.polys == [[(2, 1), (5, 1), (5, 6), (2, 6)]]
    assert h.table.tolist() == [rec(0, 4, 30, 34, 0, 2, 225, 25, 1, 0, 30)]    # the width 15^2 / 5^2 is first met on edge 1; edge 3 only ties
    ell = np.zeros((3, 3), np.uint8)
    ell[:, 0] = ell[2, :] = 1
    r, h = HO.label(ell)
    assert h.polys == [[(0, 0), (1, 0), (3, 2), (3, 3), (0, 3)]]                # the left side's collinear corners are no vertices
    assert h.table.tolist() == [rec(0, 5, 14, 18, 0, 3, 64, 8, 1, 4, 12)]
    diag = np.zeros((2, 2), np.uint8)
    diag[0, 0] = diag[1, 1] = 1
    r, h = HO.label(diag, connectivity=8)
    assert h.polys == [[(0, 0), (1, 0), (2, 1), (2, 2), (1, 2), (0, 1)]]
    assert h.table.tolist() == [rec(0, 6, 6, 8, 0, 3, 4, 2, 1, 4, 4)]          # edges 1 and 4 tie at 4 / 2: the smaller edge
    r, h = HO.label(diag, connectivity=4)
    assert h.table.tolist() == [rec(0, 4, 2, 2, 0, 2, 1, 1, 0, 2, 2), rec(4, 4, 2, 2, 0, 2, 1, 1, 0, 2, 2)] and h.polys[1][0] == (1, 1)
    square = np.ones((2, 2), np.uint8)                          # every tie rule bites: two diagonals, four equal widths, two farthest vertices each
    r, h = HO.label(square)
    assert h.table.tolist() == [rec(0, 4, 8, 8, 0, 2, 16, 4, 0, 2, 8)]
    empty = HO.label(np.zeros((3, 3), np.uint8))[1]
    assert empty.n == 0 and empty.table.shape == (0, 16) and empty.vertices.shape == (0, 2)


def test_row_form_limits():
    """one row and one column at the largest size: the operand sizes the device header is written for"""
    r, h = HO.label(np.ones((1, 32768), np.uint8))
    assert h.table.tolist() == [rec(0, 4, 2 * 32768, 32768 ** 2 + 1, 0, 2, 32768 ** 2, 32768 ** 2, 0, 2, 2 * 32768)]
    r, h = HO.label(np.ones((32768, 1), np.uint8))
    assert h.polys == [[(0, 0), (1, 0), (1, 32768), (0, 32768)]] and len(h.lo) == 32769 and h.table[0, F['width_num']] == 32768 ** 2
    assert h.table[0, F['width_den']] == 32768 ** 2 and h.table[0, F['width_edge']] == 1


# ------------------------------------------------------------------------------------- the host layer, the spec in the device's place
@pytest.fixture
def spec_device(monkeypatch):
    def label(m, classes=None, connectivity=8, labels=True, weight=None, hulls=False, **kw):
        assert m.dtype == torch.uint8 and not kw
        r, h = HO.label(m.numpy(), classes, connectivity, None if weight is None else weight.numpy())
        made = R.Hulls(torch.from_numpy(h.table), torch.from_numpy(h.vertices)) if hulls else None
        return R.Regions(torch.from_numpy(r.table), torch.from_numpy(r.labels) if labels else None, m.shape[::-1], len(r.runs), made)
    monkeypatch.setattr(R, 'label', label)


def test_rows_csv_and_views_with_hulls(spec_device, tmp_path):
    two = np.zeros((6, 8), np.uint8)
    two[1:3, 2:6] = 3                                           # 4 wide, 2 high
    two[4, 0] = 1
    plain = R.label(torch.from_numpy(two))
    assert plain.hulls is None
    with pytest.raises(ValueError):
        plain.rows(hulls=True)
    r = R.label(torch.from_numpy(two), hulls=True)
    assert r.rows(16, (5, -3), 0.25) == plain.rows(16, (5, -3), 0.25) and set(r.rows()[0]) == set(R.CSV_COLUMNS) - {'name'}       # the dicts of before
    rows = r.rows(16, (5, -3), 0.25, hulls=True)
    assert set(rows[0]) == (set(R.CSV_COLUMNS) - {'name'}) | set(R.HULL_COLUMNS)
    um = 16 * 0.25
    assert rows[0]['feret_max'] == math.sqrt(20) and rows[0]['feret_min'] == 2.0 and abs(rows[0]['feret_orth'] - 16 / math.sqrt(20)) < 1e-12
    assert rows[0]['feret_max_um'] == math.sqrt(20) * um and rows[0]['feret_min_um'] == 2.0 * um and rows[0]['solidity'] == 1.0 and rows[0]['hull_area_px'] == 8.0
    assert rows[1]['feret_max'] == math.sqrt(2) and rows[1]['feret_min'] == 1.0 and abs(rows[1]['feret_orth'] - math.sqrt(2)) < 1e-12
    assert r.rows(16, (0, 0), None, hulls=True)[0]['feret_max_um'] is None and r.rows((16, 8), (0, 0), 0.25, hulls=True)[0]['feret_min_um'] is None
    h = r.hulls
    assert len(h) == 2 and h.hull_n.tolist() == [4, 4] and h.hull_first.tolist() == [0, 4] and h.feret_sq.tolist() == [20, 2] and h.hull_area2.tolist() == [16, 2]
    assert h.feret_pair.tolist() == [[0, 2], [0, 2]] and h.width.tolist() == [[64, 16], [1, 1]] and h.orth_num.tolist() == [16, 2]
    assert [p.tolist() for p in h.polygons()] == [[[2, 1], [6, 1], [6, 3], [2, 3]], [[0, 4], [1, 4], [1, 5], [0, 5]]]
    assert h.polygons(16, (5, -3))[0].tolist() == [[37, 13], [101, 13], [101, 45], [37, 45]]      # the box corners of Regions.rows: no half-step shift
    assert (rows[0]['x0'], rows[0]['y0'], rows[0]['x1'], rows[0]['y1']) == (37, 13, 101, 45)
    assert h.polygons((2, 3))[1].tolist() == [[0, 12], [2, 12], [2, 15], [0, 15]]
    assert np.allclose(h.feret_angle(), [math.atan2(2, 4), math.atan2(1, 1)]) and h.hull_perimeter().tolist() == [12.0, 4.0]
    assert h.hull_area().tolist() == [8.0, 1.0] and h.solidity(r.area).tolist() == [1.0, 1.0] and h.solidity(np.asarray([4, 1])).tolist() == [0.5, 1.0]
    # the CSV: today's file by default, HULL_COLUMNS after CSV_COLUMNS on request
    a = open(R.write_csv(str(tmp_path / 'a.csv'), r, 16, (5, -3), 0.25, {3: 'Invasive'})).read()
    b = open(R.write_csv(str(tmp_path / 'b.csv'), plain, 16, (5, -3), 0.25, {3: 'Invasive'})).read()
    assert a == b and a.splitlines()[0] == ','.join(R.CSV_COLUMNS)
    back = list(csv.DictReader(open(R.write_csv(str(tmp_path / 'c.csv'), r, 16, (5, -3), 0.25, {3: 'Invasive'}, hulls=True))))
    assert list(back[0]) == list(R.CSV_COLUMNS + R.HULL_COLUMNS) and len(back) == 2 and [row[:len(R.CSV_COLUMNS)] for row in csv.reader(open(tmp_path / 'c.csv'))] == list(csv.reader(open(tmp_path / 'a.csv')))
    assert (back[0]['feret_max'], back[0]['feret_min'], back[0]['feret_max_um'], back[0]['solidity'], back[0]['hull_area_px']) == ('4.4721', '2.0000', '17.8885', '1.0000', '8.0000')
    assert list(csv.DictReader(open(R.write_csv(str(tmp_path / 'd.csv'), r, hulls=True))))[0]['feret_max_um'] == ''


def test_bed_size_on_the_spec(spec_device):
    mask = np.zeros((40, 60), np.uint8)
    yy, xx = np.mgrid[0:40, 0:60]
    mask[((xx - 30) / 22.0) ** 2 + ((yy - 18) / 9.0) ** 2 <= 1] = 1         # an ellipse, the bed
    mask[35:38, 2:6] = 1                                        # a speck
    got = R.bed_size(torch.from_numpy(mask), 16, 0.5)
    want = HO.bed_size(mask, 16, 0.5)
    assert got == want and set(got) == {'d1', 'd2', 'area', 'hull_area', 'solidity', 'd1_mm', 'd2_mm', 'area_mm2'}
    assert 43 <= got['d1'] <= 46 and 18 <= got['d2'] <= 20 and got['solidity'] <= 1 and got['area'] == int(mask[:30].sum())
    assert got['d1_mm'] == got['d1'] * 16 * 0.5 / 1000 and got['area_mm2'] == got['area'] * (16 * 0.5 / 1000) ** 2
    assert set(R.bed_size(torch.from_numpy(mask))) == {'d1', 'd2', 'area', 'hull_area', 'solidity'} and R.bed_size(torch.from_numpy(mask)) == HO.bed_size(mask)
    assert R.bed_size(torch.from_numpy(mask).bool()) == HO.bed_size(mask)
    assert R.bed_size(torch.zeros((4, 5), dtype=torch.uint8)) is None
    tie = np.zeros((5, 9), np.uint8)
    tie[0, 0:3] = tie[3, 4:7] = 1                               # two largest regions: the smaller id
    tie[2, 0] = 1
    assert R.bed_size(torch.from_numpy(tie))['d1'] == math.sqrt(10) and R.bed_size(torch.from_numpy(tie))['area'] == 3


# ------------------------------------------------------------------------------------------------------------------ the C entries
NAMES = {'wsi_regionhull_workspace_bytes', 'wsi_regionhull_rows', 'wsi_regionhull_chains', 'wsi_regionhull_emit', 'wsi_regionhull_measure'}


def test_entries_declared_mirrored_and_checked(lib):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read(), flags=re.S)
    assert set(re.findall(r'\b(wsi_regionhull_[a-z0-9_]+)\s*\(', hdr)) == {n for n in native.SIGNATURES if n.startswith('wsi_regionhull_')} == NAMES
    assert all(hasattr(lib, n) for n in NAMES)
    for n in NAMES:
        args = re.search(r'\b%s\s*\(([^)]*)\)' % n, hdr).group(1)
        assert len(args.split(',')) == len(native.SIGNATURES[n][1]), n
    internal = open(os.path.join(native.CSRC, 'internal.h')).read()
    assert all(n + '_dispatch' in internal for n in NAMES - {'wsi_regionhull_workspace_bytes'})
    assert int(re.search(r'#define WSI_HIP_ABI_VERSION (\d+)', hdr).group(1)) == native.ABI_VERSION == 9 == lib.wsi_hip_abi_version()     # additive
    mk = open(os.path.join(native.CSRC, 'Makefile')).read()
    assert re.search(r'^SRCS\s*=.*\bregion_hulls\.hip\b', mk, re.M) and re.search(r'^build/%\.o:.*\bregion_hulls_dev\.h\b', mk, re.M)
    # every check comes before any device work, so the entries answer without a GPU.  Fake, aligned addresses.
    P = lambda a: C.c_void_p(a)
    RWS, WS, TAB, N, V, OUT = P(1 << 22), P(1 << 24), P(1 << 20), P(1 << 19), P(1 << 26), P(1 << 27)
    rneed, need = lib.wsi_region_workspace_bytes(64, 48, 100), lib.wsi_regionhull_workspace_bytes(64, 48, 100, 7)
    big = dict(bytes=1 << 40, rbytes=1 << 40)

    def rows(**k):
        return lib.wsi_regionhull_rows(k.get('rws', RWS), k.get('rbytes', rneed), k.get('tab', TAB), k.get('W', 64), k.get('H', 48), k.get('n', 100),
                                       k.get('regions', 7), k.get('ws', WS), k.get('bytes', need), None)
    for k in (dict(rws=None), dict(tab=None), dict(ws=None), dict(W=0), dict(H=0), dict(W=32769, **big), dict(H=32769, **big), dict(n=0), dict(n=64 * 48 + 1, **big),
              dict(regions=0), dict(regions=101, **big), dict(bytes=need - 1), dict(rbytes=rneed - 1), dict(ws=P((1 << 24) + 8)), dict(rws=P((1 << 22) + 8)),
              dict(tab=P((1 << 20) + 4))):
        assert rows(**k) == -22, k

    def chains(**k):
        return lib.wsi_regionhull_chains(k.get('ws', WS), k.get('bytes', need), k.get('W', 64), k.get('H', 48), k.get('n', 100), k.get('regions', 7),
                                         k.get('counts', N), None)
    for k in (dict(ws=None), dict(counts=None), dict(bytes=need - 1), dict(W=0), dict(H=32769, **big), dict(n=0), dict(regions=0), dict(regions=101, **big),
              dict(ws=P((1 << 24) + 4)), dict(counts=P((1 << 19) + 2))):
        assert chains(**k) == -22, k

    def emit(**k):
        return lib.wsi_regionhull_emit(k.get('ws', WS), k.get('bytes', need), k.get('tab', TAB), k.get('W', 64), k.get('H', 48), k.get('n', 100),
                                       k.get('regions', 7), k.get('V', 40), k.get('out', V), None)
    for k in (dict(ws=None), dict(tab=None), dict(out=None), dict(bytes=need - 1), dict(W=-1), dict(n=0), dict(regions=0), dict(V=27), dict(V=2 * 107 + 1),
              dict(out=P((1 << 26) + 4)), dict(tab=P((1 << 20) + 4))):
        assert emit(**k) == -22, k

    def measure(**k):
        return lib.wsi_regionhull_measure(k.get('ws', WS), k.get('bytes', need), k.get('W', 64), k.get('H', 48), k.get('n', 100), k.get('regions', 7),
                                          k.get('v', V), k.get('V', 40), k.get('out', OUT), None)
    for k in (dict(ws=None), dict(v=None), dict(out=None), dict(bytes=need - 1), dict(H=0), dict(n=0), dict(regions=101, **big), dict(V=27), dict(V=215),
              dict(out=P((1 << 27) + 4)), dict(v=P((1 << 26) + 4)), dict(ws=P((1 << 24) + 8))):
        assert measure(**k) == -22, k


def test_workspace_size_is_the_documented_one(lib):
    dev_h = open(os.path.join(native.CSRC, 'region_hulls_dev.h')).read()
    assert 'constexpr int PIECE = 64;' in dev_h and 'constexpr int GROUP = 64;' in dev_h and 'constexpr int STACK = 4096;' in dev_h
    assert (HO.PIECE, HO.GROUP_ROWS) == (64, 4096) and R.HULL_FIELDS == HO.FIELDS[:11]
    fields = re.search(r'enum Field \{([^}]*)\}', dev_h).group(1).replace('= 0', '').lower().split(',')
    assert tuple(f.strip() for f in fields) == HO.FIELDS[:11]
    hdr = open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read()
    for word in ('height', 'row_off', 'lo ', 'hi ', 'st_r', 'st_l', 'seg_r', 'seg_l', 'n_r', 'n_l', 'count', 'first', 'sums', 'picks'):
        assert re.search(r'^ \*     %s' % word, hdr, re.M), word
    r256 = lambda b: (b + 255) // 256 * 256
    for w, h, n, k in ((1, 1, 1, 1), (64, 48, 100, 7), (64, 48, 100, 100), (2048, 1536, 262144, 1023), (2048, 1536, 262145, 1024), (32768, 32768, 1 << 30, 1 << 29)):
        rows = n + k
        want = 4 * r256(4 * (k + 1)) + 6 * r256(4 * rows) + 2 * r256(4 * k) + r256(4 * (-(-(k + 1) // 1024) + 1)) + r256(64 * rows)
        assert lib.wsi_regionhull_workspace_bytes(w, h, n, k) == want, (w, h, n, k)
    for w, h, n, k in ((0, 5, 1, 1), (5, 0, 1, 1), (32769, 1, 1, 1), (1, 32769, 1, 1), (4, 4, 0, 1), (4, 4, 17, 1), (4, 4, 8, 0), (4, 4, 8, 9)):
        assert lib.wsi_regionhull_workspace_bytes(w, h, n, k) == 0


# ----------------------------------------------------------------------------------- the shared arithmetic under the sanitizers
def column_map(heights, gap=2):
    """columns of the given heights side by side, one region each"""
    m = np.zeros((max(heights), gap * len(heights)), np.uint8)
    for k, hgt in enumerate(heights):
        m[:hgt, gap * k] = 1
    return m


WIDE = [(1 << 60, 1 << 31, 1 << 60, 1 << 31), ((1 << 60) - 1, 1 << 31, 1 << 60, 1 << 31), (1 << 60, 1 << 31, (1 << 60) - 1, 1 << 31),
        (1 << 60, (1 << 31) - 1, 1 << 60, 1 << 31), (1 << 60, 1 << 31, 1 << 60, (1 << 31) - 1), (((1 << 30) - 1) ** 2, (1 << 31) - 1, 1 << 60, 1 << 31),
        (1, 1, 1, 1), (0, 1, 1, 1 << 31), (3, 2, 6, 4), ((1 << 64) - 1, 1, (1 << 64) - 1, (1 << 64) - 1)]


def san_cases():
    cases = []
    for c in RF.random_cases(120) + RF.shape_cases():
        for conn in (4, 8):
            cases.append(dict(name='%s/%d' % (c['name'], conn), m=c['m'], classes=c.get('classes'), connectivity=conn, kind=0))
    cases.append(dict(name='one column', m=np.ones((32768, 1), np.uint8), classes=None, connectivity=4, kind=0))
    cases.append(dict(name='one row', m=np.ones((1, 32768), np.uint8), classes=None, connectivity=8, kind=0))
    cases.append(dict(name='piece borders', m=column_map([62, 63, 64, 1, 61, 65, 126, 127, 128, 129, 3, 200]), classes=None, connectivity=8, kind=0))
    yy, xx = np.mgrid[0:301, 0:301]
    cases.append(dict(name='disc', m=((xx - 150) ** 2 + (yy - 150) ** 2 <= 150 ** 2).astype(np.uint8), classes=None, connectivity=8, kind=0))
    cases.append(dict(name='largest operands', kind=1))
    return cases


@pytest.fixture(scope='module')
def sanitizer_run(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('region_hulls_san')
    exe = str(d / 'region_hulls_san')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
           os.path.join(ROOT, 'tests', 'region_hulls_san_main.cpp'), '-o', exe]
    if os.path.basename(cxx) == 'g++':
        cmd += ['-static-libasan', '-static-libubsan']          # the runtimes inside the program: nothing has to be preloaded or come first
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode:
        if re.search(r'cannot find .*(asan|ubsan)|libasan|libubsan', res.stdout):
            pytest.skip('the sanitizer runtime is not installed')
        raise AssertionError(res.stdout)
    cases, want = [], []
    for c in san_cases():                                       # a map without a region launches nothing: it is no case here
        w = None if c['kind'] == 1 else HO.label(c['m'], c['classes'], c['connectivity'])
        if w is None or w[0].n:
            cases.append(c)
            want.append(w)
    with open(d / 'corpus.bin', 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for c, w in zip(cases, want):
            if c['kind'] == 1:
                f.write(struct.pack('<3i', 1, len(WIDE), 0) + b''.join(struct.pack('<4Q', *v) for v in WIDE))
                continue
            r, h = w
            f.write(struct.pack('<3i', 0, len(r.runs), r.n))
            f.write(np.column_stack([r.runs[:, :3], r.id.astype(np.int32)]).astype('<i4').tobytes())
            f.write(r.table[:, [O.F['y0'], O.F['y1']]].astype('<i4').tobytes())
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    res = subprocess.run([exe, str(d / 'corpus.bin'), str(d / 'results.bin')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0, res.stdout[-4000:]
    assert 'runtime error' not in res.stdout and 'Sanitizer' not in res.stdout, res.stdout[-4000:]
    raw = open(d / 'results.bin', 'rb').read()
    results, at = [], 0
    for c, w in zip(cases, want):
        if c['kind'] == 1:
            results.append(np.frombuffer(raw, '<u8', 3 * len(WIDE), at).reshape(-1, 3))
            at += 24 * len(WIDE)
            continue
        n = w[0].n
        total, = struct.unpack_from('<I', raw, at)
        table = np.frombuffer(raw, '<i8', 16 * n, at + 4).reshape(n, 16)
        vertices = np.frombuffer(raw, '<i4', 2 * total, at + 4 + 128 * n).reshape(total, 2)
        results.append((table, vertices))
        at += 4 + 128 * n + 8 * total
    assert at == len(raw)
    return cases, want, results


def test_sanitized_walk_equals_the_spec(sanitizer_run):
    """the header the kernels compile, walked on the host the way the kernels' lanes walk a region table, under ASan and UBSan: 0
    differences from the spec's tables and vertex lists, case by case, and the 128-bit comparison at its largest operands"""
    cases, want, results = sanitizer_run
    assert len(cases) >= 250
    differences = regions = 0
    for c, w, got in zip(cases, want, results):
        if c['kind'] == 1:
            for (n1, d1, n2, d2), row in zip(WIDE, got.tolist()):
                assert (row[0] << 64 | row[1]) == n1 * d2 and row[2] == int(n1 * d2 < n2 * d1), (n1, d1, n2, d2)
            continue
        differences += int(got[0].shape != w[1].table.shape or (got[0] != w[1].table).sum()) + int(got[1].shape != w[1].vertices.shape or (got[1] != w[1].vertices).sum())
        regions += w[0].n
        assert differences == 0, c['name']
    assert differences == 0 and regions > 2900
    by_name = {c['name']: r for c, r in zip(cases, results)}
    assert by_name['one column'][1].tolist() == [[0, 0], [1, 0], [1, 32768], [0, 32768]]
    assert by_name['disc'][0][0, F['hull_n']] > 64 and by_name['piece borders'][0].shape == (12, 16)
    assert (1 << 60, 1 << 31, 1 << 60, 1 << 31) in WIDE and int(results[-1][1, 2]) == 1 and int(results[-1][0, 2]) == 0
