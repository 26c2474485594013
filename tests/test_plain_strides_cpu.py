"""The host side of tests/test_gpu_plain_strides.py, without a GPU: the launch caps stated in tests/plain_fixture.py still match
the HIP sources, every chosen size really is past its cap (so that a thread goes round its loop, the SLIC centres fill a second
LDS round and the block sums a second scan round), and every oracle finishes at that size."""
import os
import re

import numpy as np
import pytest

from oracle import postprocess_oracle as PPO
from oracle import proposals_oracle as PO
from oracle import wsi_oracle as WO
from tests import plain_fixture as F

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'wsi_segmentation_pipeline_amd', 'csrc')
GRID_FOR = re.compile(r'static int grid_for\(long long total\) \{\s*long long g = \(total \+ 255\) / 256;\s*'
                      r'return \(int\)\(g > (\d+) \? (\d+) : \(g < 1 \? 1 : g\)\);\s*\}')
CLAMP = re.compile(r'> (\d{4,}) \? (\d+)')            # every `> N ? N` with N >= 1000: grid_for's cap and the clamps at launch sites


@pytest.fixture(scope='module')
def src():
    out = {}
    for name in ('proposals', 'postproc', 'slide_ops', 'ingest'):
        with open(os.path.join(CSRC, name + '.hip')) as f:
            out[name] = f.read()
    return out


# ------------------------------------------------------------------------------------------ 1. the constants mirror the sources
@pytest.mark.parametrize('name,cap', [('proposals', F.CAP_PROPOSALS), ('postproc', F.CAP_16384), ('slide_ops', F.CAP_16384),
                                      ('ingest', F.CAP_16384)])
def test_grid_for_caps(src, name, cap):
    found = GRID_FOR.findall(src[name])
    assert len(found) == 1, 'one private grid_for per file'
    assert int(found[0][0]) == int(found[0][1]) and int(found[0][0]) * F.BLOCK == cap


def test_launch_site_clamps(src):
    """The explicit clamps, and no others: a new clamp at a launch site has to show up here (and get its own test size)."""
    def clamps(name):
        found = CLAMP.findall(src[name])
        assert all(a == b for a, b in found)
        return sorted(int(a) * F.BLOCK for a, _ in found)
    assert clamps('proposals') == sorted([F.CAP_LAB, F.CAP_SLIC_SUM, F.CAP_PROPOSALS])
    assert clamps('postproc') == sorted([F.CAP_COUNTS, F.CAP_COUNTS, F.CAP_16384])
    assert clamps('slide_ops') == sorted([F.CAP_COUNTS, F.CAP_16384])
    assert clamps('ingest') == [F.CAP_16384]
    p = src['proposals']
    m = re.search(r'const int g = grid_for\(npix\) > (\d+) \? \1 : grid_for\(npix\);\s*'
                  r'hipLaunchKernelGGL\(lab_a_kernel, dim3\(g\), dim3\(256\)[^\n]*\n\s*hipLaunchKernelGGL\(lab_thresh_kernel, dim3\(g\), dim3\(256\)', p)
    assert m and int(m.group(1)) * F.BLOCK == F.CAP_LAB
    m = re.search(r'hipLaunchKernelGGL\(slic_sum_kernel, dim3\(g1 > (\d+) \? \1 : g1\), dim3\(256\)', p)
    assert m and int(m.group(1)) * F.BLOCK == F.CAP_SLIC_SUM
    for name, n in (('postproc', 2), ('slide_ops', 1)):
        found = re.findall(r'dim3\(grid_for\(n\) > (\d+) \? \1 : grid_for\(n\)\), dim3\(256\)', src[name])
        assert len(found) == n and all(int(v) * F.BLOCK == F.CAP_COUNTS for v in found)


@pytest.mark.parametrize('name,kernel,grid', [
    ('ingest', 'resample_h_kernel', 'grid_for((long long)N * ph * tw)'), ('ingest', 'resample_v_kernel', 'grid_for((long long)N * th * tw)'),
    ('slide_ops', 'tile_gather_kernel', 'grid_for((long long)N * ph * pw)'), ('slide_ops', 'paint_winner_kernel', 'grid_for(n)'),
    ('slide_ops', 'paint_write_kernel', 'grid_for(npix)'), ('postproc', 'resize_bilinear_f64_kernel', 'grid_for((long long)C * Hd * Wd)'),
    ('postproc', 'argmax_kernel', 'grid_for(HW)'), ('proposals', 'hsv_mask_kernel', 'grid_for(npix)'),
    ('proposals', 'tile_keep_kernel', 'grid_for(n)'), ('proposals', 'tile_emit_kernel', 'grid_for(n)'),
    ('proposals', 'cc_rank_kernel', 'g'), ('proposals', 'cc_flatten_kernel', 'g'), ('proposals', 'scan_block_kernel', '(int)nb'),
    ('proposals', 'scan_sums_kernel', '1'), ('proposals', 'slic_assign_kernel', 'g1')])
def test_launch_geometry_of_the_kernels_under_test(src, name, kernel, grid):
    """Each kernel is launched where the fixture's sizes assume: 256 threads, the grid of its file's grid_for (or the stated one)."""
    launches = re.findall(r'hipLaunchKernelGGL\(%s, dim3\((.*?)\), dim3\((\d+)\), 0, st' % kernel, src[name])
    assert launches and all(g == grid and int(b) == F.BLOCK for g, b in launches), launches
    body = re.search(r'void %s\(.*?\n}\n' % kernel, src[name], re.S).group(0)
    if kernel not in ('scan_block_kernel', 'scan_sums_kernel', 'slic_assign_kernel'):
        assert re.search(r'blockIdx\.x \* 256LL \+ threadIdx\.x; \w+ < \w+; \w+ \+= \(long long\)gridDim\.x \* 256\)', body), 'grid-stride loop'


def test_slic_and_scan_literals(src):
    p = src['proposals']
    assert int(re.search(r'#define SLIC_MAXK (\d+)', p).group(1)) == F.SLIC_MAXK
    assign = re.search(r'void slic_assign_kernel\(.*?\n}\n', p, re.S).group(0)
    m = re.search(r'for \(int k0 = 0; k0 < K; k0 \+= (\d+)\)', assign)
    assert int(m.group(1)) == F.SLIC_LDS_ROUND
    assert re.search(r'__shared__ double sg\[%d \* 6\];' % F.SLIC_LDS_ROUND, assign) and 'min(%d, K - k0)' % F.SLIC_LDS_ROUND in assign
    assert 'K > SLIC_MAXK) return 0;' in p                                # the scratch size of 0 that proposals.slic turns into ValueError
    block = re.search(r'void scan_block_kernel\(.*?\n}\n', p, re.S).group(0)
    assert int(re.search(r'\(long long\)blockIdx\.x \* (\d+);', block).group(1)) == F.SCAN_BLOCK
    assert 'threadIdx.x * 4 + k' in block and 4 * F.BLOCK == F.SCAN_BLOCK
    shifts = re.findall(r'block_sums\[\w+ >> (\d+)\]', p)
    assert len(shifts) == 2 and all(1 << int(s) == F.SCAN_BLOCK for s in shifts)   # cc_rank_kernel, tile_emit_kernel
    blocks = re.findall(r'nb = \(n \+ (\d+)\) / (\d+)', p)
    assert len(blocks) == 3 and all(int(a) + 1 == int(b) == F.SCAN_BLOCK for a, b in blocks)
    sums = re.search(r'void scan_sums_kernel\(.*?\n}\n', p, re.S).group(0)
    assert int(re.search(r'for \(int b0 = 0; b0 < nb; b0 \+= (\d+)\)', sums).group(1)) * F.SCAN_BLOCK == F.SCAN_ROUND
    assert 'carry += s[255]' in sums


# ------------------------------------------------------------------------------------------ 2. every size is past its cap
def test_resample_sizes_and_oracle():
    h_both, v_both = F.resample_elements('both_passes')
    h_w, v_w = F.resample_elements('width_only')
    assert (h_both, v_both) == (5632000, 4224000) and h_both > F.CAP_16384 and v_both > F.CAP_16384
    assert h_w > F.CAP_16384 and v_w == 0
    H, W = F.RESAMPLE_LEVEL_HW
    ph, pw = F.RESAMPLE_IN
    o = F.RESAMPLE_ORIGINS
    assert len(o) == 16 and len(np.unique(o, axis=0)) == 16
    over = {'left': (o[:, 0] < 0).sum(), 'top': (o[:, 1] < 0).sum(), 'right': (o[:, 0] + pw > W).sum(), 'bottom': (o[:, 1] + ph > H).sum()}
    assert all(v >= 1 for v in over.values()) and ((o[:, 0] < 0) | (o[:, 1] < 0) | (o[:, 0] + pw > W) | (o[:, 1] + ph > H)).sum() >= 3
    assert (F.resample_level()[:H // 4] == 255).all()
    for case, (n, out_hw) in F.RESAMPLE_CASES.items():
        exp = F.resample_expected(case)
        assert exp.shape == (16,) + out_hw + (3,) and exp.dtype == np.uint8
        assert len({e.tobytes() for e in exp}) == 16                      # a tile placed at the wrong origin cannot pass
        idx = F.resample_origin_of(case)
        assert len(idx) == n and set(idx[F.CAP_16384 // (ph * out_hw[1]):]) == set(range(16))   # all 16 origins recur past the cap


def test_gather_size_and_oracle():
    ph, pw = F.GATHER_HW
    assert F.GATHER_TILES * ph * pw == 4587520 > F.CAP_16384
    H, W = F.GATHER_LEVEL_HW
    o = F.GATHER_ORIGINS
    assert ((o[:, 0] < 0) | (o[:, 1] < 0) | (o[:, 0] + pw > W) | (o[:, 1] + ph > H)).sum() == 2
    exp = F.gather_expected()
    assert exp.shape == (5, 3, ph, pw) and exp.dtype == np.float32 and len({e.tobytes() for e in exp}) == 5
    assert F.GATHER_TILES - F.CAP_16384 // (ph * pw) >= len(o)             # every origin recurs past the cap


def test_resize_argmax_sizes_and_oracle():
    c, (h, w) = F.RESIZE_SRC[0], F.RESIZE_DST
    assert c * h * w > F.CAP_16384 and h * w > F.CAP_16384
    assert h * w - F.ARGMAX_TAIL >= F.CAP_16384                           # the whole tail is read in a thread's second round
    assert F.resize_expected().shape == (c, h, w)
    x, want = F.argmax_input(), F.argmax_expected()
    tail = x.reshape(c, -1)[:, -F.ARGMAX_TAIL:]
    assert np.isnan(tail[0]).any() and np.isnan(tail[1]).any() and np.isnan(tail).all(0).any() and (tail[0] == tail[1]).sum() >= 1500
    assert not np.isnan(x.reshape(c, -1)[:, :-F.ARGMAX_TAIL]).any()
    t = want.ravel()[-F.ARGMAX_TAIL:]
    assert (t == 0).any() and (t == 1).any()


def test_paint_sizes_and_oracle():
    lists, ref = F.paint_case()
    npix = F.PAINT_HW[0] * F.PAINT_HW[1]
    assert npix > F.CAP_16384
    rect_entries = sum(len(i[0]) for i in lists[:3])
    assert rect_entries > F.CAP_16384 and isinstance(lists[3], np.ndarray) and lists[3].ndim == 1
    assert len(set(F.PAINT_CLASSES[:3].tolist())) == 3
    rects = [np.zeros(F.PAINT_HW, bool) for _ in range(3)]
    for r, (y0, y1, x0, x1) in zip(rects, F.PAINT_RECTS):
        r[y0:y1, x0:x1] = True
    assert (rects[0] & rects[1]).any() and (rects[1] & rects[2]).any()
    before = np.zeros(F.PAINT_HW, np.int64)
    for idx, cl in zip(lists[:3], F.PAINT_CLASSES):
        before[idx] = cl
    changed = (before != ref).ravel()
    assert changed[-F.PAINT_TAIL:].sum() > 1000 and npix - F.PAINT_TAIL >= F.CAP_16384
    assert sorted(np.unique(ref).tolist()) == [0, 1, 2, 3]


def test_mask_sizes_and_oracles():
    h, w = F.HSV_HW
    assert h * w > F.CAP_PROPOSALS
    first_second_round_row = -(-F.CAP_PROPOSALS // w)
    img = F.hsv_image()
    for name, (r0, r1) in F.hsv_special_rows().items():
        assert first_second_round_row <= r0 < r1 <= h and h - 40 <= r0, name
    rows = F.hsv_special_rows()
    assert (img[slice(*rows['white'])] == 255).all() and (img[slice(*rows['black'])] == 0).all()
    g = img[slice(*rows['grey'])]
    assert (g[..., 0] == g[..., 1]).all() and (g[..., 1] == g[..., 2]).all() and len(np.unique(g)) > 100
    for mu in F.HSV_MU:
        m = F.hsv_expected(mu)
        assert 0.05 < m.mean() < 0.95 and not m[h - 22:h - 6].any() and m[h - 6:].any()
    h, w = F.LAB_HW
    assert h * w == 540000 > F.CAP_LAB
    y0, y1, x0, x1 = F.LAB_BLOCK
    assert h - 60 <= y0 and y1 * w > F.CAP_LAB + 10 * w                   # ten rows of the block are summed in a second round only
    masks = [F.lab_expected(mu) for mu in F.LAB_MU]
    assert all(m[y0:y1, x0:x1].all() and 0 < m.sum() < m.size for m in masks) and not np.array_equal(*masks)
    # the threshold depends on the second round: a mean over the rows inside the first launch alone gives another mask there
    head = F.CAP_LAB // w
    assert not np.array_equal(WO.find_nuclei_lab(F.lab_image()[:head], F.LAB_MU[0]), masks[0][:head])


def test_slic_sizes_and_oracles():
    k2 = F.slic_centres(F.SLIC_ROUND2)
    assert F.SLIC_LDS_ROUND < k2 == 1728 <= F.SLIC_MAXK
    assert PO.slic_setup(*F.SLIC_ROUND2['hw'], F.SLIC_ROUND2['n_segments'])[1:3] == (2, 2)
    lab = F.slic_expected('round2')
    assert (lab >= F.SLIC_LDS_ROUND).sum() > 1000 and len(np.unique(lab[lab >= F.SLIC_LDS_ROUND])) > 500
    assert (lab < F.SLIC_LDS_ROUND).sum() > 1000
    h, w = F.SLIC_SUMS['hw']
    assert h * w > F.CAP_SLIC_SUM and F.slic_centres(F.SLIC_SUMS) == 64
    lab = F.slic_expected('sums')
    assert len(np.unique(lab.ravel()[F.CAP_SLIC_SUM:])) >= 8              # pixels past the cap feed several centres' sums
    assert F.slic_centres(F.SLIC_TOO_MANY) > F.SLIC_MAXK


def test_cc_closed_forms_match_the_oracle():
    m = F.isolated_mask((513, 512), 0.03)
    assert np.array_equal(PO.connected_components(m), F.isolated_labels(m))
    for n in F.CC_GAPPED_ROWS:
        g = F.gapped_row(n)
        assert np.array_equal(PO.connected_components(g), F.row_labels(g))
    g = F.gapped_row(F.SCAN_BLOCK + 1)
    assert g[0, F.SCAN_BLOCK - 1] and g[0, F.SCAN_BLOCK] and not g[0, F.SCAN_BLOCK - 2]   # the pair straddling the block edge
    for shape, clear in F.CC_ISOLATED[:6]:                                # the one-row masks, small enough for the oracle itself
        m = F.isolated_mask(shape, clear)
        assert np.array_equal(PO.connected_components(m), F.isolated_labels(m))


def test_cc_sizes():
    set_pixels = [int(F.isolated_mask(s, c).sum()) for s, c in F.CC_ISOLATED[:3]]
    assert set_pixels == [F.SCAN_BLOCK - 1, F.SCAN_BLOCK, F.SCAN_BLOCK + 1]
    assert [F.scan_blocks(s[0] * s[1]) for s, _ in F.CC_ISOLATED[:3]] == [2, 2, 3]
    per_round = F.SCAN_ROUND // F.SCAN_BLOCK
    assert [s for s, _ in F.CC_ISOLATED[6:]] == [(512, 512), (513, 512), (512, 513), (700, 800), (511, 514)]
    assert [F.scan_blocks(s[0] * s[1]) for s, _ in F.CC_ISOLATED[6:]] == [per_round, per_round + 1, per_round + 1, 547, per_round + 1]
    assert 2 * per_round < 547 <= 3 * per_round
    # set pixels behind the first round of block sums: their labels need the carry ((512, 513) has none there: see the fixture)
    behind = [int(F.isolated_mask(s, c).ravel()[F.SCAN_ROUND:].sum()) for s, c in F.CC_ISOLATED[6:]]
    assert behind[0] == 0 and behind[2] == 0 and behind[1] > 200 and behind[4] > 200 and behind[3] > 50000
    assert F.CC_GAPPED_ROWS == (1023, 1024, 1025)
    for shape, clear in F.CC_ISOLATED[3:]:
        m = F.isolated_mask(shape, clear)
        full = F.isolated_mask(shape, 0.0)
        share = 1.0 - m.sum() / full.sum()
        assert 0.015 < share < 0.05 and not (m & ~full).any()
        if m.size >= F.SCAN_ROUND:                                        # irregular counts per scan block
            per_block = np.add.reduceat(m.ravel().astype(np.int64), np.arange(0, m.size, F.SCAN_BLOCK))
            assert len(np.unique(per_block)) > 5
            assert F.isolated_labels(m).max() == m.sum()


def test_tile_grid_sizes_and_oracle():
    g = F.TILE_GRID
    n = F.tile_grid_candidates()
    assert n == 265224 > F.SCAN_ROUND and F.scan_blocks(n) > F.SCAN_ROUND // F.SCAN_BLOCK
    every = F.tile_grid_expected(False)
    assert len(every) == n
    kept = F.tile_grid_expected(True)
    assert 0.2 < len(kept) / n < 0.8, len(kept) / n
    # kept and dropped candidates on both sides of the first round of block sums
    flags = np.zeros(n, bool)
    order = {(int(x), int(y)): i for i, (x, y) in enumerate(every)}
    flags[[order[(int(x), int(y))] for x, y in kept]] = True
    assert 0.2 < flags[F.SCAN_ROUND:].mean() < 0.8 and 0.2 < flags[:F.SCAN_ROUND].mean() < 0.8
    mk = F.tile_grid_mask()
    assert mk.shape == (int(g['ih'] * g['m']), int(g['iw'] * g['m']))


def test_degenerate_hulls_and_one_point_contour_oracles():
    assert [n for _, n in F.DEGENERATE_HULLS.values()] == [246, 284, 1, 1, 1, 42, 50]
    for name, (m, n) in F.DEGENERATE_HULLS.items():
        hull = PPO.convex_hull_image(m)
        assert int(hull.sum()) == n and (hull >= m).all(), name
        assert PPO.bwperim(hull).sum() >= 1 and len(PPO.hull_polygon(m)) >= 4, name
    shapes = [m.shape for m, _ in F.DEGENERATE_HULLS.values()]
    assert shapes == [(1, 300), (300, 1), (1, 1), (40, 50), (40, 50), (40, 50), (40, 50)]
    assert [int(m.sum()) for m, _ in F.DEGENERATE_HULLS.values()] == [2, 2, 1, 1, 1, 2, 2]
    for num in F.ONE_POINT_NUMS:
        out = WO.evenly_spaced_points_on_a_contour(F.ONE_POINT_CONTOUR, num)
        assert np.array_equal(out, np.repeat(F.ONE_POINT_CONTOUR, num, 0))
