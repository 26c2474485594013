"""CPU side of the distance transform: the two-pass spec (tests/edt_oracle.py) against the brute-force definition and against SciPy,
hand-computed surface scores, morph_disc and margin_band with the spec standing in for the device, the C-ABI entries, their argument
checks and the documented workspace layout, and the shared per-column step and per-pixel scan (csrc/edt_dev.h) as a stand-alone
program under the host sanitizers, equal to the spec on the whole corpus."""
import ctypes as C
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
import edt_fixture as F                                        # noqa: E402
import edt_oracle as O                                         # noqa: E402
from wsi_segmentation_pipeline_amd import distance as D, native      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


# ---------------------------------------------------------------------------------------------------------------------- the spec
def test_two_pass_spec_equals_brute_force():
    cases = F.random_cases(240)
    assert {c['density'] for c in cases} == set(F.DENSITIES) and min(F.DENSITIES) == 0.001 and max(F.DENSITIES) == 0.9
    assert sum(c['invert'] for c in cases) >= 100 and sum(not c['invert'] for c in cases) >= 100
    none = finite = 0
    for c in cases:
        want, got = O.brute(c['m'], c['invert']), O.distance_sq(c['m'], c['invert'])
        assert got.dtype == np.int32 and np.array_equal(got, want), c['name']
        none, finite = none + int((want == O.EDT_NONE).all()), finite + int((want != O.EDT_NONE).all())
        assert (want == O.EDT_NONE).all() or (want != O.EDT_NONE).all()          # a map has a feature or it has none
    assert none >= 3 and finite >= 200
    empty = np.zeros((7, 9), np.uint8)
    assert (O.distance_sq(empty) == O.EDT_NONE).all() and (O.distance_sq(empty, True) == 0).all()
    assert (O.column_distances(empty) == O.G_NONE).all() and np.isinf(O.distance(empty)).all()
    one = np.zeros((5, 6), np.uint8)
    one[1, 2] = 9
    y, x = np.mgrid[0:5, 0:6]
    assert np.array_equal(O.distance_sq(one), (y - 1) ** 2 + (x - 2) ** 2)
    assert O.column_distances(one)[:, 2].tolist() == [1, 0, 1, 2, 3] and (np.delete(O.column_distances(one), 2, 1) == O.G_NONE).all()


def test_spec_equals_scipy():
    ndi = pytest.importorskip('scipy.ndimage')
    maps = [(c['m'], c['invert']) for c in F.random_cases(40, seed=9) if (c['m'] != 0).any() and (c['m'] == 0).any()]
    maps += [(F.random_map(200, 300, 0.002, 1), False), (F.random_map(200, 300, 0.6, 2), True), (F.random_map(97, 131, 0.05, 3), False)]
    assert len(maps) >= 30
    for m, invert in maps:
        f = O.features(m, invert)
        want = np.rint(ndi.distance_transform_edt(~f) ** 2).astype(np.int64)     # SciPy measures to the nearest ZERO: the mirror image
        assert np.array_equal(O.distance_sq(m, invert), want)
    for n in (2 ** 31 - 1, 2 * 32767 ** 2, 2 ** 30 + 12345):
        assert int(np.rint(np.sqrt(np.float64(n)) ** 2)) == n


# ---------------------------------------------------------------------------------------------------------- surface scores by hand
def _rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def _surface_brute(a, b):
    """every surface pixel against every surface pixel of the other mask"""
    pa, pb = np.argwhere(O.bwperim(a) > 0), np.argwhere(O.bwperim(b) > 0)
    d = ((pa[:, None, :] - pb[None, :, :]) ** 2).sum(-1)
    return sorted(d.min(1).tolist() + d.min(0).tolist())


def test_surface_distances_by_hand():
    a, b = _rect(24, 24, 2, 12, 2, 12), _rect(24, 24, 6, 16, 5, 15)              # 10 x 10, moved by (4, 3): corner to corner is 5
    s = O.surface_distances(a, b)
    assert s['hd'] == 5.0 and s['n_a'] == s['n_b'] == 36
    pooled = _surface_brute(a, b)
    assert len(pooled) == 72 and pooled[-1] == 25
    assert s['hd95'] == math.sqrt(pooled[(95 * 72 + 99) // 100 - 1]) and abs(s['assd'] - sum(math.sqrt(v) for v in pooled) / 72) < 1e-12
    assert O.surface_distances(a, b, spacing=0.5)['hd'] == 2.5
    same = O.surface_distances(a, a)
    assert (same['hd'], same['hd95'], same['assd']) == (0.0, 0.0, 0.0) and same['n_a'] == 36
    # the surface of a one-pixel-wide bar is the bar; that of a filled rectangle its outline
    assert np.array_equal(O.bwperim(_rect(5, 9, 2, 3, 1, 8)), _rect(5, 9, 2, 3, 1, 8))
    assert int(O.bwperim(_rect(9, 9, 0, 9, 0, 9)).sum()) == 32                  # outside the map counts as unset
    # nearest rank: 20 values -> the 19th smallest, 21 values -> the 20th
    for fn in (O.pooled_scores, D.pooled_scores):
        s20 = fn([0, 1, 4, 100], [10, 5, 4, 1], 12, 8)
        assert (s20['hd'], s20['hd95']) == (10.0, 2.0) and s20['assd'] == (5 * 1.0 + 4 * 2.0 + 10.0) / 20
        s21 = fn([0, 1, 4, 100], [10, 5, 4, 2], 12, 9, spacing=2.0)
        assert (s21['hd'], s21['hd95']) == (20.0, 20.0)
        assert fn([49], [1], 1, 0)['hd'] == math.inf             # one surface empty: whatever the multiset
    # one far pixel among 40 surface pixels moves the Hausdorff distance, not HD95
    spur = a.copy()
    spur[22, 22] = 1
    s = O.surface_distances(spur, a)
    assert s['hd'] == math.sqrt(11 ** 2 + 11 ** 2) == math.sqrt(_surface_brute(spur, a)[-1]) and s['hd95'] == 0.0 and (s['n_a'], s['n_b']) == (37, 36)


def test_surface_distances_empty_rules():
    z, a = np.zeros((6, 7), np.uint8), _rect(6, 7, 1, 4, 1, 5)
    assert O.surface_distances(z, z) == {'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'n_a': 0, 'n_b': 0}
    for s, n_a, n_b in ((O.surface_distances(a, z), 10, 0), (O.surface_distances(z, a), 0, 10)):
        assert s['hd'] == s['hd95'] == s['assd'] == math.inf and (s['n_a'], s['n_b']) == (n_a, n_b)
    assert D.pooled_scores([], [], 0, 0) == O.pooled_scores([], [], 0, 0)
    assert D.pooled_scores([], [], 3, 0) == O.pooled_scores([], [], 3, 0) and D.pooled_scores([], [], 0, 2)['assd'] == math.inf


# ------------------------------------------------------------------------------- the Python layer, the spec standing in for the device
@pytest.fixture
def spec_device(monkeypatch):
    def distance_sq(features, invert=False, out=None):
        assert features.dtype == torch.uint8 and out is None
        return torch.from_numpy(O.distance_sq(features.numpy(), invert))
    monkeypatch.setattr(D, 'distance_sq', distance_sq)


def test_morph_disc_and_margin_band_are_thresholds_of_the_spec(spec_device):
    m = (F.disc(40, 52, 18, 20, 9) | F.disc(40, 52, 25, 40, 6)).astype(np.uint8)
    m[18, 20] = 0                                               # a one-pixel hole: closing fills it, opening keeps it
    m[3, 45] = 1                                                # a speck: opening removes it
    t = torch.from_numpy(m)
    d2, d2i = O.distance_sq(m), O.distance_sq(m, True)
    for r in (0, 1, 3, 7):
        assert np.array_equal(D.morph_disc(t, r, 'dilate').numpy(), (d2 <= r * r).astype(np.uint8))
        assert np.array_equal(D.morph_disc(t, r, 'erode').numpy(), (d2i > r * r).astype(np.uint8))
        for op in ('dilate', 'erode', 'open', 'close'):
            got = D.morph_disc(t, r, op)
            assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), O.morph_disc(m, r, op)), (r, op)
    assert np.array_equal(D.morph_disc(t, 0, 'erode').numpy(), m) and np.array_equal(D.morph_disc(t, 0, 'dilate').numpy(), m)
    assert D.morph_disc(t, 2, 'open')[3, 45] == 0 and D.morph_disc(t, 2, 'open')[18, 20] == 0 and D.morph_disc(t, 2, 'close')[18, 20] == 1
    # dilation by a disc: exactly the pixels within r of the mask, by the definition
    ys, xs = np.nonzero(m)
    y, x = np.mgrid[0:40, 0:52]
    near = (((y[..., None] - ys) ** 2 + (x[..., None] - xs) ** 2).min(-1) <= 9).astype(np.uint8)
    assert np.array_equal(D.morph_disc(t, 3, 'dilate').numpy(), near)
    # erosion does not eat from the border: a full map stays full, and a mask on the border keeps its border pixels
    full = torch.ones((9, 11), dtype=torch.uint8)
    assert D.morph_disc(full, 4, 'erode').all()
    half = torch.zeros((9, 11), dtype=torch.uint8)
    half[:, :6] = 1
    assert D.morph_disc(half, 2, 'erode').numpy().tolist() == [[1] * 4 + [0] * 7] * 9
    for inner, outer in ((0, 0), (1, 0), (0, 2), (3, 5)):
        got = D.margin_band(t, inner, outer).numpy()
        want = ((m > 0) & (d2i <= inner * inner)) | ((m == 0) & (d2 <= outer * outer))
        assert np.array_equal(got, want.astype(np.uint8)) and np.array_equal(got, O.margin_band(m, inner, outer))
    assert not D.margin_band(t, 0, 0).any()
    band = D.margin_band(t, 3, 5).numpy()
    assert band[m > 0].sum() > 0 and band[m == 0].sum() > 0 and band.sum() < m.size
    assert np.array_equal(D.margin_band(torch.from_numpy(m > 0), 3, 5).numpy(), band)              # a bool mask is taken as u8


def test_refusals(spec_device):
    t = torch.zeros((4, 5), dtype=torch.uint8)
    for bad in (dict(r=-1), dict(r=1.5), dict(r=True), dict(r=1 << 15), dict(op='gradient')):
        with pytest.raises(ValueError):
            D.morph_disc(t, bad.get('r', 1), bad.get('op', 'dilate'))
    for inner, outer in ((-1, 0), (0, 2.5)):
        with pytest.raises(ValueError):
            D.margin_band(t, inner, outer)
    for m in (torch.zeros((4, 5), dtype=torch.int32), torch.zeros((2, 4, 5), dtype=torch.uint8), torch.zeros((4, 10), dtype=torch.uint8)[:, ::2], np.zeros((4, 5), np.uint8)):
        with pytest.raises(ValueError):
            D.margin_band(m, 1, 1)


def test_distance_sq_needs_the_device():
    with pytest.raises(RuntimeError):
        D.distance_sq(torch.zeros((4, 5), dtype=torch.uint8))
    with pytest.raises(ValueError):
        D.distance_sq(torch.zeros((4, 5), dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------------ the C entries
def test_entries_declared_mirrored_and_checked(lib):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read(), flags=re.S)
    names = {'wsi_edt_workspace_bytes', 'wsi_edt_columns', 'wsi_edt_rows'}
    assert set(re.findall(r'\b(wsi_edt_[a-z0-9_]+)\s*\(', hdr)) == {n for n in native.SIGNATURES if n.startswith('wsi_edt_')} == names
    assert all(hasattr(lib, n) for n in names)
    for n in names:                                             # argument counts of the header and of the ctypes mirror agree
        args = re.search(r'\b%s\s*\(([^)]*)\)' % n, hdr).group(1)
        assert len(args.split(',')) == len(native.SIGNATURES[n][1]), n
    assert int(re.search(r'#define WSI_HIP_ABI_VERSION (\d+)', hdr).group(1)) == native.ABI_VERSION == 9       # additive: the version stays
    mk = open(os.path.join(native.CSRC, 'Makefile')).read()
    assert re.search(r'^SRCS\s*=.*\bedt\.hip\b', mk, re.M) and re.search(r'^build/%\.o:.*\bedt_dev\.h\b', mk, re.M)
    # every check comes before any device work, so the entries answer without a GPU.  Fake, aligned addresses.
    P = lambda a: C.c_void_p(a)
    M, WS, OUT = P((1 << 21) + 3), P(1 << 22), P(1 << 23)
    need = lib.wsi_edt_workspace_bytes(64, 48)

    def columns(**k):
        return lib.wsi_edt_columns(k.get('map', M), k.get('W', 64), k.get('H', 48), k.get('pitch', 69), k.get('invert', 0), k.get('ws', WS),
                                   k.get('bytes', need), None)
    for k in (dict(map=None), dict(ws=None), dict(W=0), dict(H=0), dict(W=-3), dict(W=32769, pitch=40000, bytes=1 << 40), dict(H=32769, bytes=1 << 40),
              dict(pitch=63), dict(pitch=-1), dict(bytes=need - 1), dict(bytes=0), dict(ws=P((1 << 22) + 8))):
        assert columns(**k) == -22, k

    def rows(**k):
        return lib.wsi_edt_rows(k.get('ws', WS), k.get('bytes', need), k.get('W', 64), k.get('H', 48), k.get('out', OUT), k.get('pitch', 256), None)
    for k in (dict(ws=None), dict(out=None), dict(W=0), dict(H=-1), dict(W=32769, pitch=1 << 20, bytes=1 << 40), dict(H=32769, bytes=1 << 40),
              dict(pitch=255), dict(pitch=252), dict(pitch=258), dict(bytes=need - 1), dict(ws=P((1 << 22) + 4)), dict(out=P((1 << 23) + 2))):
        assert rows(**k) == -22, k


def test_workspace_layout_is_the_documented_one(lib):
    """the g plane starts the workspace, H rows of u16 2 * ((W + 127) / 128 * 128) bytes apart; two int32 [bands][W] tables, each
    rounded up to 256 bytes, follow it: that is all of wsi_edt_workspace_bytes"""
    dev_h = open(os.path.join(native.CSRC, 'edt_dev.h')).read()
    assert 'constexpr int LIMIT = 32768;' in dev_h and 'constexpr int BAND = 64;' in dev_h
    assert 'constexpr int32_t EDT_NONE = 0x7FFFFFFF;' in dev_h and 'constexpr uint16_t G_NONE = 0xFFFF;' in dev_h
    assert (D.LIMIT, D.BAND, D.EDT_NONE, D.G_NONE) == (32768, 64, 0x7FFFFFFF, 0xFFFF) == (O.LIMIT, F.BAND, O.EDT_NONE, O.G_NONE)
    src = open(os.path.join(native.CSRC, 'edt.hip')).read()
    consts = dict(re.findall(r'constexpr int (\w+) = ([^;]+);', src))
    assert int(consts['THREADS']) == F.TILE_W and consts['TILE_W'] == 'THREADS' and int(consts['THREADS']) * int(consts['ROW_VEC']) == F.ROW_ROUND
    hdr = open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read()
    assert 'at offset 0' in hdr and '2 * ((W + 127) / 128 * 128) bytes apart' in hdr
    for w, h in ((1, 1), (127, 63), (128, 64), (129, 65), (257, 129), (2048, 1536), (8192, 6144), (32768, 1), (1, 32768), (32768, 32768)):
        assert D.g_pitch(w) % 128 == 0 and w <= D.g_pitch(w) < w + 128
        table = (-(-h // 64) * w * 4 + 255) // 256 * 256
        assert lib.wsi_edt_workspace_bytes(w, h) == h * D.g_pitch(w) * 2 + 2 * table, (w, h)
    for w, h in ((0, 5), (5, 0), (-1, 5), (32769, 1), (1, 32769)):
        assert lib.wsi_edt_workspace_bytes(w, h) == 0


# ----------------------------------------------------------------------------------- the shared step and scan under the sanitizers
def san_cases():
    cases = [dict(c, kind=0) for c in F.random_cases(240)]
    extra = [('band-1', F.random_map(F.BAND - 1, 19, 0.02, 41)), ('band', F.random_map(F.BAND, 17, 0.02, 42)), ('band+1', F.random_map(F.BAND + 1, 16, 0.02, 43)),
             ('2band+1', F.random_map(2 * F.BAND + 1, 9, 0.01, 44)), ('corners', F.corners(3 * F.BAND + 5, 21)), ('wide', F.random_map(3, 300, 0.01, 45)),
             ('last band', np.pad(np.ones((1, 13), np.uint8), ((4 * F.BAND + 2, 0), (0, 0)))), ('far row', F.far_end_row()), ('far column', F.far_end_column())]
    for k, (name, m) in enumerate(extra):
        cases.append(dict(name=name, m=m, invert=name.startswith('band') and k % 2 == 1, kind=0))
    cases.append(dict(name='largest sum', g=F.largest_sum_row(), kind=1))
    return cases


def spec_of(c):
    """(g, out) of a corpus case; the 32768-wide single row goes through rows_single (the same minimum over the finite columns only)"""
    if c['kind'] == 1:
        return None, O.rows_single(c['g'])[None]
    g = O.column_distances(c['m'], c['invert'])
    return g, (O.rows_single(g[0])[None] if g.shape[1] > 4096 else O.rows_from_g(g))


@pytest.fixture(scope='module')
def sanitizer_run(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('edt_san')
    exe = str(d / 'edt_san')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
           os.path.join(ROOT, 'tests', 'edt_san_main.cpp'), '-o', exe]
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
                f.write(struct.pack('<6i', 1, len(c['g']), 1, 0, 0, len(c['g'])) + c['g'].astype('<u2').tobytes())
                continue
            h, w = c['m'].shape
            f.write(struct.pack('<6i', 0, w, h, int(c['invert']), (0, 1, 3, 8, 15)[k % 5], w + (0, 5, 16)[k % 3]))
            f.write(np.ascontiguousarray(c['m']).tobytes())
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    res = subprocess.run([exe, str(d / 'corpus.bin'), str(d / 'results.bin')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0, res.stdout[-4000:]
    assert 'runtime error' not in res.stdout and 'Sanitizer' not in res.stdout, res.stdout[-4000:]
    raw = open(d / 'results.bin', 'rb').read()
    results, at = [], 0
    for c in cases:
        if c['kind'] == 1:
            w = len(c['g'])
            results.append((None, np.frombuffer(raw, '<i4', w, at).reshape(1, w)))
            at += 4 * w
            continue
        h, w = c['m'].shape
        results.append((np.frombuffer(raw, '<u2', h * w, at).reshape(h, w), np.frombuffer(raw, '<i4', h * w, at + 2 * h * w).reshape(h, w)))
        at += 6 * h * w
    assert at == len(raw)
    return cases, results


def test_sanitized_step_and_scan_equal_the_spec(sanitizer_run):
    """the header the kernels compile, walked on the host the way the kernels' lanes walk a map, under ASan and UBSan: 0 differences
    from the spec's g plane and distances, case by case, and the largest sum the rule can form"""
    cases, results = sanitizer_run
    assert len(cases) >= 250
    differences = pixels = 0
    for c, (g, out) in zip(cases, results):
        want_g, want = spec_of(c)
        if g is not None:
            differences += int((g != want_g).sum())
        differences += int((out != want).sum())
        pixels += out.size
        assert differences == 0, c['name']
    assert differences == 0 and pixels > 190000
    by_name = {c['name']: r for c, r in zip(cases, results)}
    assert by_name['largest sum'][1][0, 32767] == 2147352578 == 2 * 32767 ** 2 and by_name['largest sum'][1][0, 0] == 32767 ** 2
    assert by_name['far row'][1][0].tolist() == ((32767 - np.arange(32768, dtype=np.int64)) ** 2).tolist()
    assert by_name['far column'][0][:, 0].tolist() == (32767 - np.arange(32768)).tolist()
    assert by_name['far column'][1][0, 0] == 32767 ** 2
