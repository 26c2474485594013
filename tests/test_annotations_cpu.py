"""CPU side of the annotation rasteriser: the spec (tests/annotations_oracle.py) against matplotlib off the boundary and against
gcd-stepped lattice points on it, the XML parsers against what the reference's own readers recorded (tests/golden/annotation_parse.json,
written by tools/gen_golden_annotations.py), the host-side refusals, the C-ABI entry and its argument checks, and the shared coverage
test (csrc/poly_dev.h) as a stand-alone program under the host sanitizers, equal to the spec on the whole corpus."""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import annotation_fixture as AF                                # noqa: E402
import annotations_oracle as O                                 # noqa: E402
from wsi_segmentation_pipeline_amd import annotations as A, native      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'annotation_parse.json')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------------------------- the spec
def test_oracle_equals_matplotlib_off_the_boundary():
    from matplotlib.path import Path
    polys = AF.random_polygons(200, seed=5)
    assert all(3 <= len(p) <= 11 and p.min() >= -10 and p.max() <= 74 for p in polys)
    ys, xs = np.mgrid[0:64, 0:64]
    pts = np.stack((xs.ravel(), ys.ravel()), 1)
    checked = mismatches = 0
    for p in polys:
        inside = O.covered(p, xs, ys).ravel()
        off = ~O.boundary(p, xs, ys).ravel()
        ref = Path(np.concatenate((p, p[:1])).astype(np.float64), closed=True).contains_points(pts.astype(np.float64))
        # Path.contains_points counts crossings (even-odd), as the spec does; on a boundary it is not defined, so those points are left
        # to test_oracle_boundary_is_the_gcd_stepped_lattice
        checked += int(off.sum())
        mismatches += int((inside[off] != ref[off]).sum())
    assert checked > 800000 and mismatches == 0, (checked, mismatches)


def test_oracle_boundary_is_the_gcd_stepped_lattice():
    ys, xs = np.mgrid[-12:80, -12:80]
    polys = AF.random_polygons(200, seed=5) + [np.asarray(v) for v in AF.SHAPES.values()]
    total = 0
    for p in polys:
        want = np.zeros(xs.shape, bool)
        for x, y in O.edge_lattice_points(p):
            if -12 <= x < 80 and -12 <= y < 80:
                want[y + 12, x + 12] = True
        got = O.boundary(p, xs, ys)
        assert np.array_equal(got, want)
        assert not (got & ~O.covered(p, xs, ys)).any()          # every boundary point is covered
        total += int(want.sum())
    assert total > 4000                                         # at least the vertices and a few interior lattice points per polygon


def test_oracle_small_polygons_and_painting():
    m = O.rasterize([[(3, 2)], [(5, 5), (9, 9)], [(0, 0), (20, 0), (20, 20), (0, 20)], [(1, 1), (4, 1), (4, 4), (1, 4)]], [5, 6, 1, 0], (12, 12))
    assert m[0, 0] == 1 and m[11, 11] == 1 and m[0, 3] == 1 and (m[1:5, 1:5] == 0).all() and m[5, 5] == 1 and m[0, 5] == 1
    m = O.rasterize([[(3, 2)], [(5, 5), (9, 9)]], [5, 6], (12, 12), out=np.full((12, 12), 7, np.uint8))
    assert m[2, 3] == 5 and [m[k, k] for k in range(4, 11)] == [7, 6, 6, 6, 6, 6, 7] and (m == 7).sum() == 144 - 6
    m = O.rasterize([[(4, 4), (12, 12)]], [9], (4, 4), step=(4, 2), origin=(0, 2))     # samples (0..12 step 4, 2..8 step 2): (4, 4), (8, 8)
    assert (m > 0).sum() == 2 and m[1, 1] == 9 and m[3, 2] == 9


# ------------------------------------------------------------------------------------------------------------------- the parsers
@pytest.fixture(scope='module')
def xml_files(tmp_path_factory):
    d = tmp_path_factory.mktemp('xml')
    isc, sed = str(d / 'imagescope.xml'), str(d / 'sedeen.session.xml')
    AF.write_imagescope(isc)
    AF.write_sedeen(sed)
    return isc, sed


def test_parsers_equal_the_reference_record(golden, xml_files):
    isc, sed = xml_files
    coords, labels, length, area, mpp = A.read_imagescope(isc)
    g = golden['imagescope']
    assert coords == g['coords'] and labels == g['labels'] == [1, 2, 3, 3, 1] and length == g['length'] and area == g['area'] and mpp == g['mpp']
    coords, labels = A.read_sedeen(sed)
    assert [[list(p) for p in c] for c in coords] == golden['sedeen']['coords'] and labels == golden['sedeen']['labels']
    assert labels == ['IDC', 'DCIS', 'no DCIS', 'benign', 'UDH', 'I']     # class 0 and the point / ellipse / text graphics are gone
    assert coords[0][0] == (20, 30) and coords[0][3] == (40, 280)       # int(float(.)) truncates
    coords, labels = A.read_sedeen_tb(sed)
    assert [[list(p) for p in c] for c in coords] == golden['sedeen_tb']['coords'] and labels == golden['sedeen_tb']['labels'] == ['tb1', 'tbtwo']
    assert len(golden['class_dictionary']) >= 40 and [s for s, _ in golden['class_dictionary']] == AF.LABEL_STRINGS
    for s, c in golden['class_dictionary']:
        assert A.class_dictionary(s) == c, s
    assert {c for _, c in golden['class_dictionary']} == {0, 1, 2, 3}
    from utils import read_xml, read_xml_sunnybrook as RS
    for s, rgb in golden['mapToClass']:
        assert list(RS.mapToClass(s)) == rgb, s
    assert RS.class_dictionary is A.class_dictionary and RS.readXML(sed)[1] == golden['sedeen']['labels']
    assert read_xml.readXML(isc)[1] == g['labels'] and read_xml.findExtension(os.path.dirname(isc)) == ['imagescope.xml', 'sedeen.session.xml']
    for mod in (read_xml, RS):
        src = open(mod.__file__).read()
        assert not re.search(r'^\s*(import|from)\s+(cv2|skimage|scipy)', src, re.M)


def test_sedeen_clamp_and_100_pixel_rule(xml_files):
    coords, labels = A.read_sedeen(xml_files[1])
    kept, classes = A.sedeen_polygons(coords, [A.class_dictionary(l) for l in labels], (800, 640))
    assert classes == [3, 2, 2, 1, 3]                            # UDH (50 wide) is rejected; 'no DCIS' stays class 2, as the reference has it
    assert kept[3].tolist() == [[600, 400], [790, 400], [799, 640], [600, 639]]    # x 1200 > 800 -> 799, y 700 > 640 -> 639, y 640 stays
    assert A.sedeen_polygons([[(0, 0), (100, 0), (100, 200), (0, 200)]], [1], (800, 640)) == ([], [])      # exactly 100 wide: rejected
    assert len(A.sedeen_polygons([[(0, 0), (101, 0), (101, 101), (0, 101)]], [1], (800, 640))[0]) == 1


def test_host_refusals(tmp_path):
    bad = str(tmp_path / 'bad.xml')
    AF.write_imagescope(bad, AF.IMAGESCOPE_REGIONS[:2] + [('necrosis', 'Value', [(1, 1), (2, 2), (3, 1)])])
    with pytest.raises(ValueError, match=r'region 3 .*necrosis'):
        A.read_imagescope(bad)
    L = A.LIMIT
    assert L == O.LIMIT == 1 << 29
    edges, polys = A.pack_polygons([[(-L, L), (0, 0), (L, -L)]], [3])
    assert edges.dtype == np.int32 and edges.tolist() == [[-L, L, 0, 0], [0, 0, L, -L], [L, -L, -L, L]]
    assert polys.tolist() == [[0, 3, -L, -L, L, L, 3, 0]]
    with pytest.raises(ValueError, match=str(L + 1)):
        A.pack_polygons([[(0, 0), (L + 1, 5), (3, 3)]], [1])
    with pytest.raises(ValueError, match=str(-L - 7)):
        A.pack_polygons([[(0, 0), (4, 4)], [(1, -L - 7)]], [1, 2])
    for kw, val in ((dict(origin=(L + 1, 0)), L + 1), (dict(origin=(0, -L - 2)), -L - 2), (dict(origin=(L - 10, 0), step=2), L - 10 + 2 * 63),
                    (dict(origin=(0, 0), step=(1, 1 << 24), size=(4, 64)), 63 << 24)):
        with pytest.raises(ValueError, match=str(val)):         # refused before anything touches a device
            A.rasterize([[(0, 0), (5, 5), (0, 5)]], [1], kw.pop('size', (64, 64)), **kw)
    for bad_call in (lambda: A.pack_polygons([[]], [1]), lambda: A.pack_polygons([[(0, 0)]], []), lambda: A.pack_polygons([[(0.5, 1.0)]], [1]),
                     lambda: A.pack_polygons([[(0, 0)]], [256]), lambda: A.rasterize([], [], (0, 4)), lambda: A.rasterize([], [], (4, 4), step=0)):
        with pytest.raises(ValueError):
            bad_call()
    e, p = A.pack_polygons([[(7, 8)], [(1, 2), (3, 4)]], [9, 0])
    assert e.tolist() == [[7, 8, 7, 8], [1, 2, 3, 4], [3, 4, 1, 2]] and p.tolist() == [[0, 1, 7, 8, 7, 8, 9, 0], [1, 2, 1, 2, 3, 4, 0, 0]]
    assert A.pack_polygons([], [])[0].shape == (0, 4)


def test_level_step_rule():
    class Scan:
        level_downsamples = (1.0, 4.0, 16.0003, 63.5, 2.03)
    assert [A.level_step(Scan, k) for k in range(4)] == [1, 4, 16, 64]
    with pytest.raises(ValueError, match='explicit step'):
        A.level_step(Scan, 4)


def test_gpu_path_refuses_a_cpu_process_loudly():
    import torch
    with pytest.raises(RuntimeError, match='GPU'):
        A.rasterize([[(0, 0), (5, 5), (0, 5)]], [1], (8, 8), out=torch.zeros((8, 8), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='GPU'):
        A.tumor_bed_map(torch.zeros((8, 8), dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------------------ the C entry
def test_entry_declared_mirrored_and_checked(lib):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read(), flags=re.S)
    assert set(re.findall(r'\b(wsi_poly_[a-z0-9_]+)\s*\(', hdr)) == {n for n in native.SIGNATURES if n.startswith('wsi_poly_')} == {'wsi_poly_raster'}
    assert hasattr(lib, 'wsi_poly_raster')
    assert int(re.search(r'#define WSI_HIP_ABI_VERSION (\d+)', hdr).group(1)) == native.ABI_VERSION == lib.wsi_hip_abi_version() == 9
    dev_h = open(os.path.join(native.CSRC, 'poly_dev.h')).read()
    consts = {k: v for k, v in re.findall(r'constexpr int (\w+) = ([^;]+);', dev_h)}
    assert consts['LIMIT'] == '1 << 29' and consts['RUN'] == '16' and int(consts['TILE_RUNS']) * 16 == A.TILE_W and int(consts['TILE_H']) == A.TILE_H
    assert consts['THREADS'] == 'TILE_RUNS * TILE_H' and consts['EDGE_CHUNK'] == 'THREADS' and A.EDGE_CHUNK == int(consts['TILE_RUNS']) * A.TILE_H
    assert consts['EDGE_CAP'] == '2 * EDGE_CHUNK' and A.EDGE_CAP == 2 * A.EDGE_CHUNK
    mk = open(os.path.join(native.CSRC, 'Makefile')).read()
    assert re.search(r'^SRCS\s*=.*\bpoly\.hip\b', mk, re.M) and re.search(r'^build/%\.o:.*\bpoly_dev\.h\b', mk, re.M)
    # every check comes before any device work, so the entry answers without a GPU.  Fake, aligned addresses.
    A16, L = C.c_void_p(1 << 20), 1 << 29

    def call(**k):
        return lib.wsi_poly_raster(k.get('edges', A16), k.get('ne', 10), k.get('polys', A16), k.get('np', 2), k.get('out', C.c_void_p((1 << 21) + 3)),
                                   k.get('W', 64), k.get('H', 48), k.get('pitch', 69), k.get('ox', 0), k.get('oy', 0), k.get('sx', 1), k.get('sy', 1), None)
    for k in (dict(out=None), dict(edges=None), dict(polys=None), dict(W=0), dict(W=-3), dict(H=0), dict(H=-1), dict(sx=0), dict(sy=0), dict(sx=-4),
              dict(ne=-1), dict(np=-1), dict(pitch=63), dict(pitch=-64), dict(edges=C.c_void_p((1 << 20) + 8)), dict(polys=C.c_void_p((1 << 20) + 2)),
              dict(ox=L + 1), dict(oy=-L - 1), dict(ox=L - 62), dict(oy=L - 46), dict(ox=-L, sx=1 << 25), dict(sy=1 << 30),
              dict(W=1 << 30, H=1 << 30, pitch=1 << 30, ox=-L, oy=-L)):
        assert call(**k) == -22, k                               # the last one: more tiles than a launch has workgroups
    assert call(np=0, edges=None, polys=None) == 0               # an empty list: nothing to launch
    assert call(np=0, out=None) == -22


# --------------------------------------------------------------------------------------------------- the shared test under sanitizers
def _san_cases():
    """(case, shift, pitch): the corpus of the GPU tests, every map at an aligned and at a misaligned address"""
    out = []
    for k, c in enumerate(AF.all_cases(A.EDGE_CHUNK)):
        w = c['size'][0]
        out.append((c, 0, w))
        out.append((c, (1, 3, 8, 15)[k % 4], w + 5))
    return out


@pytest.fixture(scope='module')
def sanitizer_run(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('poly_san')
    exe = str(d / 'poly_san')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
           os.path.join(ROOT, 'tests', 'poly_san_main.cpp'), '-o', exe]
    if os.path.basename(cxx) == 'g++':
        cmd += ['-static-libasan', '-static-libubsan']          # the runtimes inside the program: nothing has to be preloaded or come first
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode:
        if re.search(r'cannot find .*(asan|ubsan)|libasan|libubsan', res.stdout):
            pytest.skip('the sanitizer runtime is not installed')
        raise AssertionError(res.stdout)
    cases = _san_cases()
    with open(d / 'corpus.bin', 'wb') as f:
        f.write(struct.pack('<I', len(cases) + 1))
        for c, shift, pitch in cases:
            edges, polys = A.pack_polygons(c['coords'], c['labels'])
            f.write(struct.pack('<11i', c['size'][0], c['size'][1], c['origin'][0], c['origin'][1], c['step'][0], c['step'][1], shift, pitch, c['fill'],
                                len(polys), len(edges)) + polys.astype('<i4').tobytes() + edges.astype('<i4').tobytes())
        # a record that leaves the edge array: skipped (status 1), the other polygon is painted
        f.write(struct.pack('<11i', 8, 8, 0, 0, 1, 1, 0, 8, 0, 2, 3) + np.array([[2, 2, 0, 0, 9, 9, 5, 0], [0, 3, 0, 0, 6, 6, 4, 0]], '<i4').tobytes()
                + np.array([[0, 0, 6, 0], [6, 0, 0, 6], [0, 6, 0, 0]], '<i4').tobytes())
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    res = subprocess.run([exe, str(d / 'corpus.bin'), str(d / 'results.bin')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0, res.stdout[-4000:]
    raw = open(d / 'results.bin', 'rb').read()
    results, at = [], 0
    for c, _, _ in cases + [({'size': (8, 8)}, 0, 8)]:
        w, h = c['size']
        results.append((struct.unpack('<i', raw[at:at + 4])[0], np.frombuffer(raw, np.uint8, w * h, at + 4).reshape(h, w)))
        at += 4 + w * h
    assert at == len(raw)
    return cases, results


def test_sanitized_coverage_test_equals_the_spec(sanitizer_run):
    """the header the kernel compiles, walked on the host the way the kernel's lanes walk a map, under ASan and UBSan (signed overflow
    above all: the large-coordinate cases reach products of 2^60): the spec's bytes, case by case"""
    cases, results = sanitizer_run
    assert len(cases) >= 800
    painted = 0
    for (c, shift, pitch), (status, got) in zip(cases, results):
        want = O.rasterize(c['coords'], c['labels'], c['size'], c['step'], c['origin'], out=np.full(c['size'][::-1], c['fill'], np.uint8))
        assert status == 0 and np.array_equal(got, want), (c['name'], shift)
        painted += int((want != c['fill']).sum())
    assert painted > 500000
    status, got = results[-1]
    assert status == 1 and np.array_equal(got, O.rasterize([[(0, 0), (6, 0), (0, 6)]], [4], (8, 8)))
