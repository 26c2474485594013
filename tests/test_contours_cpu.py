"""CPU side of the boundary tracer: the spec (tests/contours_oracle.py) pinned by its exact round trip through the rasteriser's spec
(tests/annotations_oracle.py) and by hand-written cases, the XML writer and the reader's `negative` keyword with the spec standing in
for the device, the C-ABI entries and their argument checks, and the shared per-edge rule (csrc/contour_dev.h) as a stand-alone program
under the host sanitizers, equal to the spec on the whole corpus."""
import ctypes as C
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
import annotation_fixture as AF                                # noqa: E402
import annotations_oracle as AO                                # noqa: E402
import contour_fixture as F                                    # noqa: E402
import contours_oracle as O                                    # noqa: E402
from wsi_segmentation_pipeline_amd import annotations as A, contours as CT, native      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


def as_contours(t):
    """the spec's result as the host layer's Contours (CPU tensors): the spec standing in for the device"""
    tt = torch.from_numpy
    return CT.Contours(tt(t.vertices), tt(t.first), tt(t.count), tt(t.edges), tt(t.label), tt(t.area2), t.size, t.step, t.origin, t.bounds)


def hand(m, **kw):
    t = O.trace(np.asarray(m, np.uint8), step=1, **kw)
    return [l.tolist() for l in t.loops()], t.label.tolist(), t.area2.tolist(), t.edges.tolist()


# ---------------------------------------------------------------------------------------------------------------------- the spec
def test_round_trip_through_the_rasteriser_spec():
    cases = F.random_cases(120)
    assert sum(c['bounds'] is not None for c in cases) >= 25 and sum(c['classes'] is not None and 0 in c['classes'] for c in cases) >= 10
    assert sum(c['origin'][0] < 0 or c['origin'][1] < 0 for c in cases) >= 30
    pixels = loops = holes = 0
    for c in cases:
        t = O.trace(c['m'], c['classes'], c['step'], c['origin'], c['bounds'])
        coords, labels = t.paint_list()
        got = AO.rasterize(coords, labels, t.size, c['step'], c['origin'])
        want = F.traced_part(c['m'], O.traced_table(c['classes']))
        assert np.array_equal(got, want), c['name']
        assert int(t.count.sum()) == len(t.vertices) and int(t.edges.sum()) % 2 == 0
        if c['bounds'] is not None and len(t.vertices):
            assert t.vertices.min() >= 0 and t.vertices[:, 0].max() <= c['bounds'][0] - 1 and t.vertices[:, 1].max() <= c['bounds'][1] - 1
        pixels, loops, holes = pixels + int((want > 0).sum()), loops + len(t.first), holes + int((t.area2 < 0).sum())
    assert pixels > 5000 and loops > 1500 and holes > 50


def test_round_trip_fails_at_step_1():
    m = F.noise_map(12, 17, 2, 3)
    t = O.trace(m, step=1)
    got = AO.rasterize(*t.paint_list(), t.size, 1, (0, 0))
    assert (got != m).sum() > 0                                  # closed edges: crack polygons gain a column and a row
    t = O.trace(m, step=2)
    assert np.array_equal(AO.rasterize(*t.paint_list(), t.size, 2, (0, 0)), m)


def test_hand_written_cases():
    sq = lambda x, y: [[x, y], [x + 1, y], [x + 1, y + 1], [x, y + 1]]
    assert hand([[1]]) == ([sq(0, 0)], [1], [2], [4])
    assert hand([[7] * 5]) == ([[[0, 0], [5, 0], [5, 1], [0, 1]]], [7], [10], [12])
    # a diagonal pair: 4-connected foreground, so two loops of four that touch at (1, 1)
    assert hand([[1, 0], [0, 1]]) == ([sq(0, 0), sq(1, 1)], [1, 1], [2, 2], [4, 4])
    # a ring whose hole another label fills: the hole (walked the other way round, negative) and the filling tie on |area2|
    loops, label, area2, edges = hand([[1, 1, 1], [1, 2, 1], [1, 1, 1]])
    assert loops == [[[0, 0], [3, 0], [3, 3], [0, 3]], sq(1, 1), [[1, 1], [1, 2], [2, 2], [2, 1]]]
    assert (label, area2, edges) == ([1, 2, 1], [18, 2, -2], [12, 4, 4])
    assert O.paint_order(area2) == [0, 2, 1]                     # the hole erases before the filling paints
    # a diagonal ring: its inside leaks through the saddles, no hole
    assert hand([[0, 1, 0], [1, 0, 1], [0, 1, 0]]) == ([sq(1, 0), sq(0, 1), sq(2, 1), sq(1, 2)], [1] * 4, [2] * 4, [4] * 4)
    # collinear corners are dropped, a concave corner is kept
    assert hand([[1, 0], [1, 1]]) == ([[[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [0, 2]]], [1], [6], [8])
    for h, w in ((4, 6), (6, 3)):
        one, two = O.trace(F.checkerboard(h, w, 1, 0)), O.trace(F.checkerboard(h, w, 1, 2))
        assert int(one.edges.sum()) == 2 * h * w and int(two.edges.sum()) == 4 * h * w
        assert len(two.first) == h * w and (two.edges == 4).all() and (two.area2 == 2).all()


def test_isolated_pixels_closed_form_is_the_spec():
    """the closed form the GPU test of a million edges expects (contour_fixture.isolated_pixels_trace), pinned to the spec at small sizes"""
    for h, w, step, origin in ((6, 10, (2, 2), (0, 0)), (5, 7, (3, 2), (-4, 9)), (1, 1, (16, 16), (0, 0)), (2, 9, (5, 4), (1, -1))):
        want, got = O.trace(F.isolated_pixels(h, w), None, step, origin), F.isolated_pixels_trace(h, w, step, origin)
        assert len(want.first) == ((h + 1) // 2) * ((w + 1) // 2)
        for name in ('vertices', 'first', 'count', 'edges', 'label', 'area2'):
            assert np.array_equal(getattr(want, name), got[name]) and getattr(want, name).dtype == got[name].dtype, (h, w, name)


def test_start_vertex_loop_order_and_area_sign():
    for c in F.random_cases(40, seed=23):
        w = c['m'].shape[1]
        t = O.trace(c['m'], c['classes'], 1)
        starts = [int(l[0][1]) * (w + 1) + int(l[0][0]) for l in t.loops()]
        assert starts == sorted(starts)                          # loops by the corner of their smallest key (ties share a corner: a saddle)
        for l, a2, n in zip(t.loops(), t.area2.tolist(), t.edges.tolist()):
            key = l[:, 1] * (w + 1) + l[:, 0]
            assert key.min() == key[0]                           # the start is the loop's top-most, then left-most corner
            x, y = l[:, 0], l[:, 1]
            assert a2 == int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum()) and a2 != 0
            assert n == int(np.abs(l - np.roll(l, -1, 0)).sum())                 # the rectilinear perimeter
            d = np.roll(l, -1, 0) - l
            assert ((d != 0).sum(1) == 1).all() and (d * np.roll(d, -1, 0)).sum(1).tolist() == [0] * len(l)       # every vertex is a turn
        # a traced pixel count: outer areas minus holes
        assert int(t.area2.sum()) == 2 * int(O.traced_table(c['classes'])[c['m']].sum())


def test_min_area_drops_loops_with_what_they_hold():
    m = np.zeros((12, 12), np.uint8)
    m[1:8, 1:8] = 1
    m[3:6, 3:6] = 0                                             # a 9-pixel hole,
    m[4, 4] = 2                                                 # a pixel in it,
    m[10, 10] = 3                                               # and a pixel outside
    full = O.trace(m, step=2)
    assert sorted(full.area2.tolist()) == [-18, 2, 2, 98]
    for a, kept in ((0, 4), (1, 4), (2, 2), (9, 2), (10, 1), (49, 1), (50, 0)):
        t = O.trace(m, step=2, min_area=a)
        assert len(t.first) == kept and (np.abs(t.area2) >= 2 * a).all()
        assert t.first.tolist() == np.concatenate(([0], np.cumsum(t.count)[:-1])).tolist()[:kept]
    t = O.trace(m, step=2, min_area=2)                          # the painter's order stays valid: ring and hole, without what was inside
    want = np.where(m == 1, 1, 0)
    assert np.array_equal(AO.rasterize(*t.paint_list(), t.size, 2), want)


def test_refusals():
    m = np.zeros((4, 4), np.uint8)
    for bad, word in ((dict(classes=[256]), '256'), (dict(classes=[-1]), '-1'), (dict(step=0), '0'), (dict(step=(2, -3)), '-3'),
                      (dict(origin=(1 << 29, 0), step=4), str((1 << 29) + 14)), (dict(origin=(0, -(1 << 29) - 1)), str(-(1 << 29) - 1)),
                      (dict(bounds=(0, 5)), '0')):
        with pytest.raises(ValueError, match=re.escape(word)):
            O.trace(m, **bad)
        with pytest.raises(ValueError, match=re.escape(word)):  # the host layer refuses the same before it asks for a device
            CT.trace(torch.from_numpy(m), **bad)
    with pytest.raises(ValueError):
        CT.trace(torch.zeros((4, 4), dtype=torch.float32))
    with pytest.raises(ValueError):
        CT.trace(torch.zeros((4, 8), dtype=torch.uint8)[:, ::2])
    with pytest.raises(RuntimeError, match='GPU'):
        CT.trace(torch.from_numpy(m))
    assert CT.traced_table(None).tolist() == [0] + [1] * 255 and CT.traced_table([0, 3]).nonzero()[0].tolist() == [0, 3]
    assert np.array_equal(CT.traced_table([2, 5]) > 0, O.traced_table([2, 5])) and CT.LIMIT == O.LIMIT and CT.MAX_PIXELS == O.MAX_PIXELS


# -------------------------------------------------------------------------------------------------------------------- the writer
def test_write_imagescope_reads_back_and_restores_the_map(tmp_path):
    m = np.zeros((14, 18), np.uint8)
    m[1:12, 1:15] = 1
    m[3:9, 3:9] = 0
    m[4:7, 4:7] = 3
    m[2:5, 11:14] = 2
    m[12, 16] = 3
    step, origin = (4, 3), (-5, 2)
    t = O.trace(m, None, step, origin)
    p = str(tmp_path / 'pred.xml')
    assert CT.write_imagescope(p, as_contours(t), mpp=0.25) == p
    order = O.paint_order(t.area2)
    coords, labels, length, area, mpp = A.read_imagescope(p, negative='erase')
    assert mpp == 0.25 and [np.asarray(c).tolist() for c in coords] == [t.loops()[k].tolist() for k in order]
    assert labels == [int(t.label[k]) if t.area2[k] > 0 else 0 for k in order] and 0 in labels
    assert np.array_equal(AO.rasterize(coords, labels, t.size, step, origin), m)
    plain = A.read_imagescope(p)                                # the default reads a negative region like any other: its enclosing label
    assert plain[1] == [int(t.label[k]) for k in order] and plain[0] == coords and plain[2:] == (length, area, mpp)
    for k, a_um, l_um in zip(order, area, length):
        v = t.loops()[k]
        assert a_um == pytest.approx(abs(int(t.area2[k])) / 2 * 4 * 3 * 0.25 ** 2, abs=1e-3)
        assert l_um == pytest.approx(int(np.abs(v - np.roll(v, -1, 0)).sum()) * 0.25, abs=1e-3)
    # the structure both readers walk
    import xml.etree.ElementTree as ET
    root = ET.parse(p).getroot()
    assert root.tag == 'Annotations' and root[0].tag == 'Annotation' and root[0][0].tag == 'Attributes' and root[0][1].tag == 'Regions'
    r = root[0][1][0]
    assert r.tag == 'Region' and r[0].tag == 'Attributes' and r[0][0].get('Value') == 'Benign' and r[1].tag == 'Vertices' and r[1][0].get('Z') == '0'
    assert {k for k in r.keys()} >= {'Id', 'Text', 'NegativeROA', 'AreaMicrons', 'LengthMicrons'}
    assert [x.get('NegativeROA') for x in root[0][1]] == ['1' if t.area2[k] < 0 else '0' for k in order]
    # holes='drop' and a second layer that no reader sees
    CT.write_imagescope(p, as_contours(t), mpp=0.5, holes='drop', layers=[(as_contours(O.trace((m > 0).astype(np.uint8), None, step, origin)), {1: 'Invasive'})])
    coords2, labels2 = A.read_imagescope(p, negative='erase')[:2]
    assert labels2 == [int(t.label[k]) for k in order if t.area2[k] > 0]
    root = ET.parse(p).getroot()
    assert len(root) == 2 and [x[0][0].get('Value') for x in root[1][1]] == ['Invasive'] * 3


def test_known_rectangle_area_and_length(tmp_path):
    m = np.zeros((6, 9), np.uint8)
    m[1:4, 2:7] = 2                                             # 5 x 3 map pixels at step 16: 80 x 48 level-0 pixels
    p = str(tmp_path / 'rect.xml')
    CT.write_imagescope(p, as_contours(O.trace(m, None, 16)), mpp=0.5, names={2: 'in situ carcinoma'})
    coords, labels, length, area, mpp = A.read_imagescope(p)
    assert coords == [[[24, 8], [104, 8], [104, 56], [24, 56]]] and labels == [2]
    assert area == [80 * 48 * 0.25] and length == [(80 + 48) * 2 * 0.5] and mpp == 0.5


def test_writer_and_reader_refusals(tmp_path):
    t = as_contours(O.trace(np.array([[1, 4]], np.uint8), None, 2))
    p = str(tmp_path / 'never.xml')
    with pytest.raises(ValueError, match='label 4'):
        CT.write_imagescope(p, t)
    with pytest.raises(ValueError, match='holes'):
        CT.write_imagescope(p, t, names={1: 'Benign', 4: 'Invasive'}, holes='keep')
    with pytest.raises(ValueError, match='mpp'):
        CT.write_imagescope(p, t, names={1: 'Benign', 4: 'Invasive'}, mpp=0)
    assert not os.path.exists(p)                                # refused before anything is written
    isc = str(tmp_path / 'imagescope.xml')
    AF.write_imagescope(isc)
    with pytest.raises(ValueError, match='negative'):
        A.read_imagescope(isc, negative='subtract')
    assert A.read_imagescope(isc) == A.read_imagescope(isc, negative=None) == A.read_imagescope(isc, negative='erase')      # no negative region in it
    assert A.read_imagescope(isc)[1] == [1, 2, 3, 3, 1]
    e = as_contours(O.trace(np.zeros((3, 3), np.uint8)))
    assert len(e) == 0 and e.loops() == [] and e.paint_list() == ([], [])
    CT.write_imagescope(p, e)                                   # an empty map is no error
    assert A.read_imagescope(p)[0] == []


# ------------------------------------------------------------------------------------------------------------------ the C entries
def test_entries_declared_mirrored_and_checked(lib):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read(), flags=re.S)
    names = {'wsi_contour_count_workspace_bytes', 'wsi_contour_workspace_bytes', 'wsi_contour_count', 'wsi_contour_build', 'wsi_contour_ranks',
             'wsi_contour_order', 'wsi_contour_emit'}
    assert set(re.findall(r'\b(wsi_contour_[a-z0-9_]+)\s*\(', hdr)) == {n for n in native.SIGNATURES if n.startswith('wsi_contour_')} == names
    assert all(hasattr(lib, n) for n in names)
    for n in names:                                             # argument counts of the header and of the ctypes mirror agree
        args = re.search(r'\b%s\s*\(([^)]*)\)' % n, hdr).group(1)
        assert len(args.split(',')) == len(native.SIGNATURES[n][1]), n
    assert int(re.search(r'#define WSI_HIP_ABI_VERSION (\d+)', hdr).group(1)) == native.ABI_VERSION == 9       # additive: the version stays
    dev_h = open(os.path.join(native.CSRC, 'contour_dev.h')).read()
    assert 'constexpr int LIMIT = 1 << 29;' in dev_h and 'constexpr long long MAX_PIXELS = 1LL << 28;' in dev_h
    src = open(os.path.join(native.CSRC, 'contour.hip')).read()                 # the scan is the shared one: its constants are map_kernels.h's
    assert '#include "map_kernels.h"' in src and not re.search(r'constexpr int (THREADS|PER_THREAD|CHUNK|SUMS_TILE)\b', src)
    consts = dict(re.findall(r'constexpr int (\w+) = ([^;]+);', open(os.path.join(native.CSRC, 'map_kernels.h')).read()))
    assert int(consts['THREADS']) * int(consts['PER_THREAD']) == F.SCAN_CHUNK and consts['CHUNK'] == 'THREADS * PER_THREAD'
    assert consts['SUMS_TILE'] == 'THREADS * SUMS_PER_LANE' and int(consts['THREADS']) * int(consts['SUMS_PER_LANE']) == F.SCAN_SPAN
    assert F.SCAN_SECOND == F.SCAN_CHUNK * int(consts['THREADS']) and F.SCAN_STEP == F.SCAN_CHUNK * F.SCAN_SPAN
    mk = open(os.path.join(native.CSRC, 'Makefile')).read()
    assert re.search(r'^SRCS\s*=.*\bcontour\.hip\b', mk, re.M) and re.search(r'^build/%\.o:.*\bcontour_dev\.h\b', mk, re.M)
    assert re.search(r'^build/%\.o:.*\bmap_dev\.h\b.*\bmap_kernels\.h\b', mk, re.M)

    assert lib.wsi_contour_count_workspace_bytes(0, 5) == lib.wsi_contour_count_workspace_bytes(1 << 15, 1 << 14) == 0
    assert lib.wsi_contour_count_workspace_bytes(1 << 14, 1 << 14) > 0 and lib.wsi_contour_count_workspace_bytes(1, 1) == 256
    assert lib.wsi_contour_workspace_bytes(0) == lib.wsi_contour_workspace_bytes((1 << 30) + 1) == 0
    assert 61 * 1000 <= lib.wsi_contour_workspace_bytes(1000) <= 61 * 1000 + 13 * 512 + 64
    # every check comes before any device work, so the entries answer without a GPU.  Fake, aligned addresses.
    P, L = (lambda a: C.c_void_p(a)), 1 << 29
    table = (C.c_uint8 * 256)(*([0] + [1] * 255))
    M, WS = P((1 << 21) + 3), P(1 << 22)

    def count(**k):
        return lib.wsi_contour_count(k.get('map', M), k.get('W', 64), k.get('H', 48), k.get('pitch', 69), k.get('table', table), k.get('cws', P(1 << 20)),
                                     k.get('n', P(1 << 19)), None)
    for k in (dict(map=None), dict(table=None), dict(cws=None), dict(n=None), dict(W=0), dict(H=0), dict(W=-2), dict(pitch=63), dict(W=1 << 15, H=1 << 14, pitch=1 << 15),
              dict(cws=P((1 << 20) + 2)), dict(n=P((1 << 19) + 1))):
        assert count(**k) == -22, k
    need = lib.wsi_contour_workspace_bytes(100)

    def build(**k):
        return lib.wsi_contour_build(k.get('map', M), k.get('W', 64), k.get('H', 48), k.get('pitch', 69), k.get('table', table), k.get('cws', P(1 << 20)),
                                     k.get('ne', 100), k.get('ws', WS), k.get('bytes', need), None)
    for k in (dict(map=None), dict(table=None), dict(cws=None), dict(ws=None), dict(W=0), dict(H=-1), dict(pitch=10), dict(ne=0), dict(ne=-4),
              dict(ne=4 * 64 * 48 + 1), dict(bytes=need - 1), dict(ws=P((1 << 22) + 8)), dict(cws=P((1 << 20) + 1)), dict(W=1 << 15, H=1 << 14, pitch=1 << 15)):
        assert build(**k) == -22, k
    for k in (dict(ws=None), dict(ws=P((1 << 22) + 8)), dict(ne=0), dict(ne=(1 << 30) + 1), dict(bytes=need - 1)):
        assert lib.wsi_contour_ranks(k.get('ws', WS), k.get('bytes', need), k.get('ne', 100), None) == -22, k
    for k in (dict(ws=None), dict(ws=P((1 << 22) + 4)), dict(ne=0), dict(ne=-1), dict(bytes=need - 1), dict(W=0), dict(W=(1 << 28) + 1), dict(counts=None),
              dict(counts=P((1 << 19) + 2))):
        assert lib.wsi_contour_order(k.get('ws', WS), k.get('bytes', need), k.get('ne', 100), k.get('W', 64), k.get('counts', P(1 << 19)), None) == -22, k

    def emit(**k):
        return lib.wsi_contour_emit(k.get('map', M), k.get('W', 64), k.get('H', 48), k.get('pitch', 69), k.get('ws', WS), k.get('bytes', need), k.get('ne', 100),
                                    k.get('ox', 0), k.get('oy', 0), k.get('sx', 16), k.get('sy', 16), k.get('bw', 0), k.get('bh', 0), k.get('v', P(1 << 23)),
                                    k.get('cv', 10), k.get('loops', P(1 << 24)), k.get('a2', P(1 << 25)), k.get('cl', 10), None)
    for k in (dict(map=None), dict(ws=None), dict(v=None), dict(loops=None), dict(a2=None), dict(W=0), dict(pitch=63), dict(ne=0), dict(bytes=need - 1),
              dict(sx=0), dict(sy=-1), dict(bw=-1), dict(bh=-5), dict(cv=-1), dict(cl=-1), dict(v=P((1 << 23) + 4)), dict(loops=P((1 << 24) + 8)),
              dict(a2=P((1 << 25) + 4)), dict(ws=P((1 << 22) + 4)), dict(ox=L + 1), dict(oy=-L - 1), dict(ox=L - 64 * 16 + 9), dict(oy=-L + 7),
              dict(sx=1 << 24), dict(sy=1 << 25), dict(ox=-L + 7, bh=100)):
        assert emit(**k) == -22, k
    # (the last one: bounds_h clamps y alone, x = -L + 7 - 8 still leaves the range)


# --------------------------------------------------------------------------------------------------- the shared rule under sanitizers
def san_cases():
    cases = F.random_cases(120)
    extra = [('one', np.ones((1, 1), np.uint8)), ('row', np.full((1, 37), 7, np.uint8)), ('column', np.full((41, 1), 255, np.uint8)),
             ('empty', np.zeros((5, 9), np.uint8)), ('board2', F.checkerboard(13, 21, 1, 2)), ('board1', F.checkerboard(16, 17, 0, 9)),
             ('rings', F.nested_rings(12)), ('serpentine', F.serpentine(31, 40)), ('count', F.edge_count_map(1026, 40, 40)),
             ('blob', F.blob_map(96, 130, 3, 8))]
    for k, (name, m) in enumerate(extra):
        cases.append(dict(name=name, m=m, classes=None if k % 2 == 0 else [0, 1, 2, 9, 255], step=(3, 2) if k % 3 else (16, 16), origin=(-9, 4), bounds=None))
    return cases


@pytest.fixture(scope='module')
def sanitizer_run(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('contour_san')
    exe = str(d / 'contour_san')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
           os.path.join(ROOT, 'tests', 'contour_san_main.cpp'), '-o', exe]
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
            h, w = c['m'].shape
            bw, bh = c['bounds'] or (0, 0)
            f.write(struct.pack('<10i', w, h, c['origin'][0], c['origin'][1], c['step'][0], c['step'][1], bw, bh, (0, 1, 3, 8, 15)[k % 5], w + (0, 5, 16)[k % 3]))
            f.write(O.traced_table(c['classes']).astype(np.uint8).tobytes() + np.ascontiguousarray(c['m']).tobytes())
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    res = subprocess.run([exe, str(d / 'corpus.bin'), str(d / 'results.bin')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0, res.stdout[-4000:]
    raw = open(d / 'results.bin', 'rb').read()
    results, at = [], 0
    for _ in cases:
        ne, nl, nv = struct.unpack('<3I', raw[at:at + 12])
        at += 12
        v = np.frombuffer(raw, '<i4', 2 * nv, at).reshape(nv, 2)
        rec = np.frombuffer(raw, '<i4', 8 * nl, at + 8 * nv).reshape(nl, 8)
        a2 = np.frombuffer(raw, '<i8', nl, at + 8 * nv + 32 * nl)
        at += 8 * nv + 40 * nl
        results.append((ne, v, rec, a2))
    assert at == len(raw)
    return cases, results


def test_sanitized_rule_equals_the_spec(sanitizer_run):
    """the header the kernels compile, walked on the host the way the kernels' lanes walk a map, under ASan and UBSan: the spec's vertices,
    loop records and area2, case by case"""
    cases, results = sanitizer_run
    assert len(cases) >= 130
    edges = 0
    for c, (ne, v, rec, a2) in zip(cases, results):
        t = O.trace(c['m'], c['classes'], c['step'], c['origin'], c['bounds'])
        assert ne == int(t.edges.sum()), c['name']
        assert np.array_equal(v, t.vertices) and np.array_equal(rec, t.records()) and np.array_equal(a2, t.area2), c['name']
        edges += ne
    assert edges > 40000
