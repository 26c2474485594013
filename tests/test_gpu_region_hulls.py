"""GPU side of the region hulls (csrc/region_hulls.hip through wsi_segmentation_pipeline_amd.regions): every case byte for byte equal
to the spec (tests/region_hulls_oracle.py) - the hull table and the vertex list, from label(hulls=True) and again from the four entries
driven on guarded buffers, with the map, the region workspace and the region table untouched - each entry alone on a hand-filled
workspace, then bed_size and the bed_size hooks of predict_wsis and predict_tumorbed."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contour_fixture as CF                                   # noqa: E402
import region_fixture as RF                                    # noqa: E402
import region_hulls_oracle as HO                               # noqa: E402
import regions_oracle as O                                     # noqa: E402
from test_gpu_regions import FRONT, GREYS, GUARD, _args, _grey_slide, guarded, place       # noqa: E402
from test_gpu_regions import layout as region_layout           # noqa: E402
from wsi_segmentation_pipeline_amd import native, regions as R      # noqa: E402

pytestmark = pytest.mark.gpu
PIECE = HO.PIECE
P = lambda t: native.C.c_void_p(t.data_ptr())


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def layout(n_runs, n):
    """byte offsets of the hull workspace's arrays as include/wsi_hip.h documents them"""
    r256 = lambda b: (b + 255) // 256 * 256
    rows = n_runs + n
    sizes = (('height', 4 * (n + 1)), ('row_off', 4 * (n + 1)), ('lo', 4 * rows), ('hi', 4 * rows), ('st_r', 4 * rows), ('st_l', 4 * rows), ('seg_r', 4 * rows),
             ('seg_l', 4 * rows), ('n_r', 4 * n), ('n_l', 4 * n), ('count', 4 * (n + 1)), ('first', 4 * (n + 1)), ('sums', 4 * (-(-(n + 1) // 1024) + 1)),
             ('picks', 64 * rows))
    at, out = 0, {}
    for name, b in sizes:
        out[name] = at
        at += r256(b)
    out['bytes'] = at
    return out


def arr(whole, lay, name, count, dtype=np.uint32):
    return whole[FRONT + lay[name]:FRONT + lay[name] + count * np.dtype(dtype).itemsize].view(dtype)


def same(t, a):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def check(dev, m, classes=None, connectivity=8, want=None):
    """label `m` with hulls=True: the spec's hull table and vertices; then the four entries on guarded buffers: the same bytes, nothing
    written outside them, the region workspace, the region table and the map untouched"""
    lib = native.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    m = np.ascontiguousarray(m, np.uint8)
    h, w = m.shape
    r, hu = HO.label(m, classes, connectivity) if want is None else want
    n_runs, n, total = len(r.runs), r.n, len(hu.vertices)
    view, buf, host = place(dev, m, 3, 5)
    rneed = lib.wsi_region_workspace_bytes(w, h, n_runs)
    rws = torch.full((rneed,), GUARD, dtype=torch.uint8, device=dev)
    got = R.label(view, classes, connectivity, labels=False, workspace=rws, hulls=True)
    assert got.n == n and same(got.table, r.table)
    assert got.hulls.n == n and got.hulls.table.dtype == torch.int64 and got.hulls.vertices.dtype == torch.int32 and got.hulls.table.is_cuda
    assert tuple(got.hulls.table.shape) == (n, 16) and tuple(got.hulls.vertices.shape) == (total, 2)
    assert same(got.hulls.vertices, hu.vertices), (connectivity, m.shape)
    assert same(got.hulls.table, hu.table), (connectivity, m.shape)
    rws_before, tab_before = rws.clone(), got.table.clone()
    lay, need = layout(n_runs, n), lib.wsi_regionhull_workspace_bytes(w, h, n_runs, n)
    assert need == lay['bytes']
    ws_buf, ws = guarded(dev, need)
    counts = torch.full((2,), 77, dtype=torch.int32, device=dev)
    v_buf, v = guarded(dev, 8 * total)
    t_buf, t = guarded(dev, 128 * n)
    assert lib.wsi_regionhull_rows(P(rws), rneed, P(got.table), w, h, n_runs, n, P(ws), need, st) == 0
    assert lib.wsi_regionhull_chains(P(ws), need, w, h, n_runs, n, P(counts), st) == 0
    assert counts.tolist() == [total, 0]
    assert lib.wsi_regionhull_emit(P(ws), need, P(got.table), w, h, n_runs, n, total, P(v), st) == 0
    assert lib.wsi_regionhull_measure(P(ws), need, w, h, n_runs, n, P(v), total, P(t), st) == 0
    for whole, inner, size in ((v_buf.cpu().numpy(), hu.vertices, 8 * total), (t_buf.cpu().numpy(), hu.table, 128 * n)):
        assert whole[FRONT:FRONT + size].tobytes() == inner.tobytes() and (whole[:FRONT] == GUARD).all() and (whole[FRONT + size:] == GUARD).all()
    whole = ws_buf.cpu().numpy()
    assert (whole[:FRONT] == GUARD).all() and (whole[FRONT + need:] == GUARD).all()
    rows = int(hu.row_off[-1])
    assert np.array_equal(arr(whole, lay, 'height', n), hu.height[:n]) and np.array_equal(arr(whole, lay, 'row_off', n + 1), hu.row_off)
    assert np.array_equal(arr(whole, lay, 'lo', rows, np.int32), hu.lo) and np.array_equal(arr(whole, lay, 'hi', rows, np.int32), hu.hi)
    assert np.array_equal(arr(whole, lay, 'n_r', n), hu.n_r) and np.array_equal(arr(whole, lay, 'n_l', n), hu.n_l)
    assert np.array_equal(arr(whole, lay, 'count', n), hu.count[:n]) and np.array_equal(arr(whole, lay, 'first', n + 1), hu.first)
    assert torch.equal(rws, rws_before) and torch.equal(got.table, tab_before)          # read-only to the hull entries
    assert np.array_equal(buf.cpu().numpy(), host)
    return got


def column_map(heights, gap=2):
    m = np.zeros((max(heights), gap * len(heights)), np.uint8)
    for k, hgt in enumerate(heights):
        m[:hgt, gap * k] = 1
    return m


# ------------------------------------------------------------------------------------------------------------------------ shapes
def test_single_pixel(dev):
    m = np.zeros((3, 4), np.uint8)
    m[1, 2] = 7
    got = check(dev, m)
    assert got.hulls.table.tolist() == [[0, 4, 2, 2, 0, 2, 1, 1, 0, 2, 2, 0, 0, 0, 0, 0]] and got.hulls.vertices.tolist() == [[2, 1], [3, 1], [3, 2], [2, 2]]
    check(dev, np.ones((1, 1), np.uint8))


def test_one_row_and_one_column_at_the_limit(dev):
    check(dev, np.ones((1, 32768), np.uint8))
    got = check(dev, np.ones((32768, 1), np.uint8), connectivity=4)     # the tallest region: 32 769 corner rows, 513 pieces
    assert got.hulls.vertices.tolist() == [[0, 0], [1, 0], [1, 32768], [0, 32768]]


@pytest.mark.parametrize('rows', (PIECE - 1, PIECE, PIECE + 1, 2 * PIECE - 1, 2 * PIECE, 2 * PIECE + 1))
def test_corner_rows_round_the_piece_size(dev, rows):
    check(dev, np.ones((rows - 1, 1), np.uint8))                # a column of rows - 1 pixels has `rows` corner rows
    yy, xx = np.mgrid[0:rows - 1, 0:rows + 9]
    lens = (np.abs(yy - (rows - 1) / 2.0) * 2 < rows - 1 - np.abs(xx - rows / 2.0)) | (xx == 3)      # a lens and a bar: both chains turn in every piece
    check(dev, lens.astype(np.uint8))


def test_region_starting_in_the_last_slot_of_a_piece(dev):
    m = column_map([PIECE - 2, 5, 200, 176, 1, 2 * PIECE + 1])      # corner rows 63, 6, 201, 177, 2, 130
    r, hu = HO.label(m)
    assert hu.row_off[1] == PIECE - 1 and hu.row_off[4] % PIECE == PIECE - 1          # two regions start in a last slot and cross the border
    check(dev, m, want=(r, hu))


def test_checkerboard_rings_spiral_serpentine_combs(dev):
    board = CF.checkerboard(37, 41, 1, 0)
    four, eight = check(dev, board, connectivity=4), check(dev, board, connectivity=8)
    assert four.n == int(board.sum()) and (four.hulls.hull_n == 4).all() and eight.n == 1
    for conn in (4, 8):
        check(dev, CF.checkerboard(9, 11, 1, 2), connectivity=conn)
        check(dev, CF.nested_rings(20), (0, 1, 2, 3), conn)
        check(dev, RF.spiral(41), connectivity=conn)
        check(dev, CF.serpentine(33, 40), connectivity=conn)
    got = check(dev, RF.combs(7, 2003))                         # many runs of one region in one row on the same two atomics
    assert got.n > 190 and got.n_runs > 4 * got.n


def test_disc_with_more_vertices_than_a_workgroup_has_lanes(dev):
    yy, xx = np.mgrid[0:1411, 0:1411]
    m = ((xx - 705) ** 2 + (yy - 705) ** 2 <= 700 ** 2).astype(np.uint8)
    r, hu = HO.label(m)
    assert r.n == 1 and hu.table[0, HO.F['hull_n']] > 256
    check(dev, m, want=(r, hu))


@pytest.fixture(scope='module')
def blobs():
    m = CF.blob_map(384, 512, 3, 5)
    return m, {key: HO.label(m, *key) for key in ((None, 8), (None, 4), ((2, 3), 8), ((0, 1), 4))}


def test_blob_map_with_class_subsets(dev, blobs):
    m, want = blobs
    for (classes, conn), w in want.items():
        check(dev, m, classes, conn, want=w)
    assert want[(None, 8)][0].n > 1000 and int(want[(None, 8)][1].row_off[-1]) > 64 * PIECE       # more than one first-level workgroup


def test_same_bytes_every_run(dev, blobs):
    m = torch.from_numpy(blobs[0]).to(dev)
    a, b = R.label(m, hulls=True), R.label(m, hulls=True)
    assert torch.equal(a.hulls.table, b.hulls.table) and torch.equal(a.hulls.vertices, b.hulls.vertices) and a.hulls.n > 1000


def test_empty_map_and_untraced_class(dev):
    for m, classes in ((np.zeros((5, 7), np.uint8), None), (np.full((5, 7), 2, np.uint8), [1])):
        got = R.label(torch.from_numpy(m).to(dev), classes, hulls=True)
        assert got.n == 0 and got.hulls.n == 0 and tuple(got.hulls.table.shape) == (0, 16) and tuple(got.hulls.vertices.shape) == (0, 2)
        assert got.hulls.table.dtype == torch.int64 and got.hulls.vertices.dtype == torch.int32 and got.hulls.polygons() == []
    assert R.label(torch.from_numpy(np.ones((2, 2), np.uint8)).to(dev)).hulls is None


@pytest.mark.parametrize('n_runs', (1023, 1024, 1025))
def test_run_counts_round_the_scan_chunk(dev, n_runs):
    got = check(dev, RF.run_count_map(n_runs, 67))
    assert got.n == got.n_runs == n_runs


# ---------------------------------------------------------------------------------------------------------- the entries driven alone
def filled(dev, lay, need, arrays):
    host = np.full(FRONT + need + 64, GUARD, np.uint8)
    for name, a in arrays.items():
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        host[FRONT + lay[name]:FRONT + lay[name] + raw.size] = raw
    buf = torch.from_numpy(host).to(dev)
    return host, buf, buf[FRONT:FRONT + need]


def test_each_entry_alone_on_a_hand_filled_workspace(dev):
    lib = native.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    m = np.zeros((200, 48), np.uint8)
    m[:, :8] = column_map([PIECE - 2, 5, 200, 70])
    m[10:30, 12:43] = CF.blob_map(20, 31, 2, 3)
    h, w = m.shape
    r, hu = HO.label(m)
    n_runs, n, total, rows = len(r.runs), r.n, len(hu.vertices), int(hu.row_off[-1])
    lay, need = layout(n_runs, n), lib.wsi_regionhull_workspace_bytes(w, h, n_runs, n)
    table = torch.from_numpy(r.table).to(dev)
    # rows: reads runs and id of the region workspace and the boxes of the region table
    rlay, rneed = region_layout(h, n_runs), lib.wsi_region_workspace_bytes(w, h, n_runs)
    rhost = np.full(rneed, GUARD, np.uint8)
    for name, a in (('runs', r.runs), ('id', r.id)):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        rhost[rlay[name]:rlay[name] + raw.size] = raw
    rws = torch.from_numpy(rhost).to(dev)
    host, buf, ws = filled(dev, lay, need, {})
    assert lib.wsi_regionhull_rows(P(rws), rneed, P(table), w, h, n_runs, n, P(ws), need, st) == 0
    whole = buf.cpu().numpy()
    assert np.array_equal(arr(whole, lay, 'row_off', n + 1), hu.row_off) and np.array_equal(arr(whole, lay, 'height', n), hu.height[:n])
    lo, hi = arr(whole, lay, 'lo', n_runs + n, np.int32), arr(whole, lay, 'hi', n_runs + n, np.int32)
    assert np.array_equal(lo[:rows], hu.lo) and np.array_equal(hi[:rows], hu.hi) and (lo[rows:] == 2 ** 31 - 1).all() and (hi[rows:] == -2 ** 31).all()
    untouched = np.ones(whole.size, bool)
    for name, nxt in (('height', 'row_off'), ('row_off', 'lo'), ('lo', 'hi'), ('hi', 'st_r'), ('sums', 'picks')):      # what the rows entry may write
        untouched[FRONT + lay[name]:FRONT + lay[nxt]] = False
    assert np.array_equal(whole[untouched], host[untouched]) and np.array_equal(rws.cpu().numpy(), rhost)
    # chains: reads row_off, lo, hi
    host, buf, ws = filled(dev, lay, need, dict(row_off=hu.row_off, lo=hu.lo, hi=hu.hi))
    counts = torch.full((2,), 77, dtype=torch.int32, device=dev)
    assert lib.wsi_regionhull_chains(P(ws), need, w, h, n_runs, n, P(counts), st) == 0
    whole = buf.cpu().numpy()
    assert counts.tolist() == [total, 0] and np.array_equal(arr(whole, lay, 'first', n + 1), hu.first) and np.array_equal(arr(whole, lay, 'count', n), hu.count[:n])
    assert np.array_equal(arr(whole, lay, 'n_r', n), hu.n_r) and np.array_equal(arr(whole, lay, 'n_l', n), hu.n_l)
    for side, cnt in (('st_r', hu.n_r), ('st_l', hu.n_l)):
        got, spec = arr(whole, lay, side, rows), getattr(hu, side)
        for k in range(n):
            s = int(hu.row_off[k])
            assert np.array_equal(got[s:s + int(cnt[k])], spec[s:s + int(cnt[k])]), (side, k)
    for name in ('row_off', 'lo', 'hi'):
        size = 4 * (n + 1) if name == 'row_off' else 4 * rows
        assert np.array_equal(whole[FRONT + lay[name]:FRONT + lay[name] + size], host[FRONT + lay[name]:FRONT + lay[name] + size])
    assert (whole[:FRONT] == GUARD).all() and (whole[FRONT + need:] == GUARD).all() and (whole[FRONT + lay['picks']:FRONT + need] == GUARD).all()
    # emit: reads first, row_off, the chains, lo, hi and y0 of the region table
    host, buf, ws = filled(dev, lay, need, dict(row_off=hu.row_off, lo=hu.lo, hi=hu.hi, st_r=hu.st_r, st_l=hu.st_l, n_r=hu.n_r, n_l=hu.n_l, first=hu.first))
    v_buf, v = guarded(dev, 8 * total)
    assert lib.wsi_regionhull_emit(P(ws), need, P(table), w, h, n_runs, n, total, P(v), st) == 0
    whole = v_buf.cpu().numpy()
    assert whole[FRONT:FRONT + 8 * total].tobytes() == hu.vertices.tobytes() and (whole[:FRONT] == GUARD).all() and (whole[FRONT + 8 * total:] == GUARD).all()
    assert np.array_equal(buf.cpu().numpy(), host) and same(table, r.table)
    # measure: reads count, first and the vertices; writes picks and the table
    host, buf, ws = filled(dev, lay, need, dict(count=hu.count, first=hu.first))
    t_buf, t = guarded(dev, 128 * n)
    assert lib.wsi_regionhull_measure(P(ws), need, w, h, n_runs, n, P(torch.from_numpy(hu.vertices).to(dev)), total, P(t), st) == 0
    whole = t_buf.cpu().numpy()
    assert whole[FRONT:FRONT + 128 * n].tobytes() == hu.table.tobytes() and (whole[:FRONT] == GUARD).all() and (whole[FRONT + 128 * n:] == GUARD).all()
    whole = buf.cpu().numpy()
    assert np.array_equal(whole[:FRONT + lay['picks']], host[:FRONT + lay['picks']]) and (whole[FRONT + need:] == GUARD).all()


def test_measure_alone_at_the_largest_operands(dev):
    """the whole 32768^2 box, and a hull as thin as a triangle whose least width is 2^60 over 32767^2 + 32768^2: the 128-bit comparison
    decides between it and 2^60 / 2^30"""
    lib = native.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    box = [(0, 0), (32768, 0), (32768, 32768), (0, 32768)]
    thin = [(0, 0), (32768, 0), (32768, 32768), (32767, 32768)]
    want = np.zeros((2, 16), np.int64)
    want[0, :11] = (0, 4) + HO.measure(box)
    want[1, :11] = (4, 4) + HO.measure(thin)
    assert want[0, HO.F['width_num']] == 1 << 60 and want[0, HO.F['width_den']] == 1 << 30 and want[0, HO.F['feret_sq']] == 1 << 31
    assert want[1, HO.F['width_num']] == 1 << 60 and want[1, HO.F['width_den']] == 32767 ** 2 + 32768 ** 2 and want[1, HO.F['width_edge']] == 3
    n_runs = n = 2
    lay, need = layout(n_runs, n), lib.wsi_regionhull_workspace_bytes(32768, 32768, n_runs, n)
    host, buf, ws = filled(dev, lay, need, dict(count=np.asarray([4, 4, 0], np.uint32), first=np.asarray([0, 4, 8], np.uint32)))
    v = torch.tensor(box + thin, dtype=torch.int32, device=dev)
    t_buf, t = guarded(dev, 128 * n)
    assert lib.wsi_regionhull_measure(P(ws), need, 32768, 32768, n_runs, n, P(v), 8, P(t), st) == 0
    whole = t_buf.cpu().numpy()
    assert whole[FRONT:FRONT + 128 * n].tobytes() == want.tobytes() and (whole[:FRONT] == GUARD).all() and (whole[FRONT + 128 * n:] == GUARD).all()


# ------------------------------------------------------------------------------------------------------------- the Python layer
def test_bed_size_equals_the_spec(dev):
    yy, xx = np.mgrid[0:150, 0:220]
    mask = (((xx - 100) * 0.8 + (yy - 70) * 0.6) ** 2 / 80.0 ** 2 + ((xx - 100) * -0.6 + (yy - 70) * 0.8) ** 2 / 30.0 ** 2 <= 1).astype(np.uint8)     # a tilted ellipse
    mask[140:145, 5:30] = 1
    for args in ((), (16,), (16, 0.25), (4, 0.5)):
        got = R.bed_size(torch.from_numpy(mask).to(dev), *args)
        assert got == HO.bed_size(mask, *args), args
    assert 158 <= got['d1'] <= 163 and 59 <= got['d2'] <= 63 and 0.95 < got['solidity'] <= 1 and got['d1_mm'] == got['d1'] * 4 * 0.5 / 1000
    assert R.bed_size(torch.from_numpy(mask).to(dev).bool()) == HO.bed_size(mask)
    assert R.bed_size(torch.zeros((6, 9), dtype=torch.uint8, device=dev)) is None
    r = R.label(torch.from_numpy(mask).to(dev), hulls=True)
    _, hu = HO.label(mask)
    assert np.array_equal(r.hulls.feret_max(), HO.feret_max(hu.table)) and np.array_equal(r.hulls.feret_min(), HO.feret_min(hu.table))
    assert np.array_equal(r.hulls.feret_orth(), HO.feret_orth(hu.table)) and [p.tolist() for p in r.hulls.polygons()] == [[list(q) for q in p] for p in hu.polys]
    rows = r.rows(16, (0, 0), 0.25, hulls=True)
    assert rows[0]['feret_max'] == HO.feret_max(hu.table)[0] and rows[0]['feret_max_um'] == HO.feret_max(hu.table)[0] * 4.0 and rows[1]['solidity'] == 1.0


# ----------------------------------------------------------------------------------------------------------------------- the hooks
def test_predict_wsis_bed_size(dev, tmp_path, monkeypatch):
    """the slide and the one-layer dense model of tests/test_gpu_regions.py: bed_size is the spec's on the returned tumour bed, the errors
    are the differences to the annotated bed's, with and without a stated mpp; unset, the results have the keys of before"""
    import utils.dataset as ds
    import utils.eval as val
    args = _args(monkeypatch, tmp_path, (48, 64))
    gt = CF.blob_map(48, 64, 3, 33, radius=3)
    gt[10:40, 14:52] = 3
    slide = _grey_slide(gt)
    centres = torch.tensor([(g / 255.0 - args.dataset_mean[0]) / args.dataset_std[0] for g in GREYS], device=dev)

    class ReadsTheGrey(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return -(x[:, :1] - centres.view(1, 4, 1, 1)).abs()

    model = ReadsTheGrey().to(dev)
    params = {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}
    tb_truth = np.zeros((48, 64), np.uint8)
    tb_truth[8:44, 10:50] = 255

    def run(ep, **kw):
        dataset = ds.Dataset_wsis({'case.svs': slide}, params, bs=64)
        dataset.wsis['case.svs']['gt'] = torch.from_numpy(gt).to(dev)
        dataset.wsis['case.svs']['tb_gt'] = torch.from_numpy(tb_truth).to(dev)
        return val.predict_wsis(model, dataset, ep, **kw)['case.svs']

    out = str(tmp_path / 'out')
    plain = run(1)
    res = run(2, bed_size=True)
    assert set(res) == set(plain) | {'bed_size', 'bed_size_gt'} and set(res['scores']) == set(plain['scores']) | {'tb_d1_err', 'tb_d2_err'}
    assert set(run(3, region_table=True)) == set(plain) | {'regions'}                       # the other flag alone: the keys of before
    assert list(list(csv.DictReader(open(out + '/3/case.svs_64_regions.csv')))[0]) == list(R.CSV_COLUMNS)
    bed = (res['tumor_bed'].cpu().numpy() > 0).astype(np.uint8)
    want, want_gt = HO.bed_size(bed, 16), HO.bed_size((tb_truth > 0).astype(np.uint8), 16)
    assert bed.any() and res['bed_size'] == want and res['bed_size_gt'] == want_gt and set(want) == {'d1', 'd2', 'area', 'hull_area', 'solidity'}
    assert res['scores']['tb_d1_err'] == want['d1'] - want_gt['d1'] and res['scores']['tb_d2_err'] == want['d2'] - want_gt['d2']
    assert want_gt['d1'] == np.sqrt(40 ** 2 + 36 ** 2) and {k: res['scores'][k] for k in plain['scores']} == plain['scores']
    slide.mpp = 0.25
    both = run(4, bed_size=True, region_table=True)
    assert both['bed_size'] == HO.bed_size(bed, 16, 0.25) and both['bed_size_gt'] == HO.bed_size((tb_truth > 0).astype(np.uint8), 16, 0.25)
    assert both['scores']['tb_d1_err_mm'] == both['bed_size']['d1_mm'] - both['bed_size_gt']['d1_mm'] and 'tb_d2_err_mm' in both['scores']
    assert both['bed_size']['d1_mm'] == want['d1'] * 16 * 0.25 / 1000
    rows = list(csv.DictReader(open(out + '/4/case.svs_64_regions.csv')))
    assert list(rows[0]) == list(R.CSV_COLUMNS + R.HULL_COLUMNS) and both['regions'].hulls is not None and len(rows) == both['regions'].n
    _, hu = HO.label(both['classes_level2'].cpu().numpy(), (1, 2, 3), 8)
    assert same(both['regions'].hulls.table, hu.table) and [r['feret_max'] for r in rows] == ['%.4f' % v for v in HO.feret_max(hu.table)]
    del slide.mpp


def test_predict_tumorbed_bed_size(dev, tmp_path, monkeypatch):
    """the 80 x 80 map and the tile model of tests/test_gpu_regions.py: bed_size is the spec's on the tumour bed of the returned heat map"""
    import utils.dataset as ds
    import utils.eval as val
    from wsi_segmentation_pipeline_amd import postprocess as PP
    args = _args(monkeypatch, tmp_path, (80, 80), mask_value=1)
    gt = np.zeros((80, 80), np.uint8)
    gt[8:68, 12:72] = 1
    gt[72:76, 0:8] = 1
    slide = _grey_slide(gt)
    centres = torch.tensor([(g / 255.0 - args.dataset_mean[0]) / args.dataset_std[0] for g in GREYS], device=dev)

    class Encoder(torch.nn.Module):
        def forward(self, x):
            return (x[:, :1].mean((2, 3)),)

    class Head(torch.nn.Module):
        def forward(self, f):
            return -200.0 * (f - centres.view(1, 4)).abs()

    class TileModel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))
            self.encoder, self.classifier = Encoder(), Head()

    model = TileModel().to(dev)
    params = {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}
    out = str(tmp_path / 'out')
    plain = val.predict_tumorbed(model, ds.Dataset_wsis({'case.svs': slide}, params, bs=64), 1, mode='cls')['case.svs']
    res = val.predict_tumorbed(model, ds.Dataset_wsis({'case.svs': slide}, params, bs=64), 2, mode='cls', bed_size=True)['case.svs']
    assert set(res) == set(plain) | {'bed_size'} and np.array_equal(res['heatmap'], plain['heatmap'])
    bed = (PP.tumor_bed_from_heatmap(torch.from_numpy(np.asarray(res['heatmap'])).to(dev), 0.9, 30, 20).tb_pred > 0).to(torch.uint8).cpu().numpy()
    assert bed.any() and res['bed_size'] == HO.bed_size(bed, 16) and res['bed_size']['area'] >= 3000
    slide.mpp = 0.5
    both = val.predict_tumorbed(model, ds.Dataset_wsis({'case.svs': slide}, params, bs=64), 3, mode='cls', bed_size=True, region_table=True)['case.svs']
    assert set(both) == set(plain) | {'bed_size', 'regions', 'slide_positive'} and both['bed_size'] == HO.bed_size(bed, 16, 0.5)
    assert both['bed_size']['d1_mm'] == res['bed_size']['d1'] * 16 * 0.5 / 1000 and both['regions'].hulls is not None
    rows = list(csv.DictReader(open(out + '/3/case.svs_64_heatmap_regions.csv')))
    assert list(rows[0]) == list(R.CSV_COLUMNS + R.HULL_COLUMNS) and rows[0]['feret_max_um'] == '%.4f' % (float(both['regions'].hulls.feret_max()[0]) * 8.0)
    del slide.mpp
