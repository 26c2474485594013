"""GPU side of the region tables (csrc/regions.hip through wsi_segmentation_pipeline_amd.regions): every case byte for byte equal to the
spec (tests/regions_oracle.py) - the table, n, the int32 label map inside 0xA5 guards at a pitch larger than the row, the arrays of the
workspace inside guards, the map (and the weight map) inside guards at four base alignments and three pitches and never written - the
link, table and paint entries driven alone on hand-filled workspaces, then remove_small, overlaps, lesion_scores, slide_positive and the
region_table hooks of predict_wsis and predict_tumorbed."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contour_fixture as CF                                   # noqa: E402
import region_fixture as RF                                    # noqa: E402
import regions_oracle as O                                     # noqa: E402
from wsi_segmentation_pipeline_amd import native, regions as R      # noqa: E402
from wsi_segmentation_pipeline_amd.slide import ArraySlide     # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0xA5
OFFSETS, EXTRAS = (0, 1, 3, 8), (0, 5, 16)                      # bytes before the map's first byte mod 16; pitch - W
FRONT = 256                                                     # guard bytes before the workspace and the labels (keeps their alignment)


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


def layout(h, n):
    """byte offsets of the workspace arrays as include/wsi_hip.h documents them"""
    r256 = lambda b: (b + 255) // 256 * 256
    sizes = (('runs', 16 * n), ('row_first', 4 * (h + 1)), ('parent', 4 * n), ('up', 4 * n), ('root', 4 * n), ('flag', 4 * (n + 1)), ('rank', 4 * (n + 1)),
             ('id', 4 * n), ('sums', 4 * (-(-n // 1024) + 1)))
    at, out = 0, {}
    for name, b in sizes:
        out[name] = at
        at += r256(b)
    out['bytes'] = at
    return out


def ws_array(whole, lay, name, count, dtype=np.uint32):
    return whole[FRONT + lay[name]:FRONT + lay[name] + count * np.dtype(dtype).itemsize].view(dtype)


def check(dev, m, classes=None, connectivity=8, weight=None, places=((1, 5),), out_extra=3, want=None):
    """label `m` at every placement into a guarded label map of pitch W + out_extra and a guarded workspace: the spec's table, n, labels
    and workspace arrays, no byte written outside either, the allocations of the map and of the weight untouched"""
    lib = native.load()
    m = np.ascontiguousarray(m, np.uint8)
    h, w = m.shape
    want = O.label(m, classes, connectivity, weight) if want is None else want
    n_runs = len(want.runs)
    for offset, extra in places:
        view, buf, host = place(dev, m, offset, extra)
        wview = wbuf = whost = None
        if weight is not None:
            wview, wbuf, whost = place(dev, np.ascontiguousarray(weight, np.uint8), (offset + 5) % 16, (extra + 11) % 17)
        lay = layout(h, max(n_runs, 1))
        need = lib.wsi_region_workspace_bytes(w, h, max(n_runs, 1))
        assert need == lay['bytes']
        ws_buf, ws = guarded(dev, need)
        out_pitch = w + out_extra
        out_buf, out_bytes = guarded(dev, 4 * h * out_pitch)
        out = torch.as_strided(out_bytes.view(torch.int32), (h, w), (out_pitch, 1))
        got = R.label(view, classes, connectivity, labels=True, weight=wview, out=out, workspace=ws)
        where = (offset, extra, connectivity)
        assert got.n == want.n and got.n_runs == n_runs and got.table.dtype == torch.int64 and tuple(got.table.shape) == (want.n, 16), where
        assert got.labels.data_ptr() == out.data_ptr()
        assert got.table.cpu().numpy().tobytes() == want.table.tobytes(), where
        assert np.array_equal(got.labels.cpu().numpy(), want.labels), where
        whole = out_buf.cpu().numpy()
        inner = whole[FRONT:FRONT + 4 * h * out_pitch].reshape(h, 4 * out_pitch)
        assert (whole[:FRONT] == GUARD).all() and (whole[FRONT + 4 * h * out_pitch:] == GUARD).all() and (inner[:, 4 * w:] == GUARD).all()
        whole = ws_buf.cpu().numpy()
        assert (whole[:FRONT] == GUARD).all() and (whole[FRONT + need:] == GUARD).all()
        if n_runs:
            assert np.array_equal(ws_array(whole, lay, 'runs', 4 * n_runs, np.int32).reshape(-1, 4), want.runs), where
            assert np.array_equal(ws_array(whole, lay, 'row_first', h + 1), want.row_first), where
            assert np.array_equal(ws_array(whole, lay, 'up', n_runs), want.up) and np.array_equal(ws_array(whole, lay, 'root', n_runs), want.root), where
            assert np.array_equal(ws_array(whole, lay, 'id', n_runs), want.id) and ws_array(whole, lay, 'rank', n_runs + 1)[n_runs] == want.n, where
            assert (ws_array(whole, lay, 'parent', n_runs) <= np.arange(n_runs)).all()
        else:
            assert (whole == GUARD).all()                        # nothing is launched after the count
        assert np.array_equal(buf.cpu().numpy(), host)           # the map is never written, nor a byte round it
        if wbuf is not None:
            assert np.array_equal(wbuf.cpu().numpy(), whost)
    return want


# ------------------------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize('w', (1, 2, 15, 16, 17, 1023, 1024, 1025, 2049))
def test_widths_at_four_base_alignments_and_three_pitches(dev, w):
    m = CF.noise_map(3, w, 3, 50 + w) if w < 100 else np.repeat(CF.noise_map(3, -(-w // 3), 3, 50 + w), 3, 1)[:, :w]
    weight = np.random.default_rng(w).integers(0, 256, m.shape).astype(np.uint8)
    for conn in (4, 8):
        want = O.label(m, None, conn, weight)
        check(dev, m, None, conn, weight, places=[(o, e) for o in OFFSETS for e in EXTRAS], want=want)
    for h in (1, 2, 65):
        check(dev, CF.blob_map(h, w, 3, 7 * w + h, radius=1) if w >= 3 else CF.noise_map(h, w, 2, 7 * w + h), places=((3, 5),), out_extra=0 if h == 1 else 5)


def test_runs_across_chunk_borders(dev):
    m = np.zeros((4, 3100), np.uint8)
    m[1, 1000:1030] = 1                                         # across one border
    m[2, 5:2079] = 2                                            # across two
    m[0, 1023], m[0, 1024] = 3, 4                               # an end and a start at the border itself
    m[3, 1024:2048] = 1                                         # a run that is exactly the second chunk
    m[3, 2048:3100] = 2                                         # and one that starts the third and ends the row
    weight = np.full(m.shape, 255, np.uint8)
    want = check(dev, m, weight=weight, places=((0, 0), (3, 5), (8, 16)))
    assert len(want.runs) == 6 and sorted(want.area.tolist()) == [1, 1, 30, 1024, 1052 + 2074]
    check(dev, m, classes=[0, 2], connectivity=4)


def test_one_row_and_one_column_of_32768(dev):
    row = check(dev, np.ones((1, 32768), np.uint8), weight=np.full((1, 32768), 255, np.uint8), places=((3, 0),), out_extra=0)
    assert row.table[0, O.F['sxx']] == 32767 * 32768 * 65535 // 6 and row.table[0, O.F['wsum']] == 255 * 32768 and len(row.runs) == 1
    col = check(dev, np.ones((32768, 1), np.uint8), connectivity=4, places=((1, 5),), out_extra=1)
    assert col.n == 1 and len(col.runs) == 32768 and col.table[0, O.F['syy']] == 32767 * 32768 * 65535 // 6
    mixed = np.ones((32768, 1), np.uint8)
    mixed[::3] = 2
    assert check(dev, mixed, places=((8, 0),), out_extra=0).n == 21846


@pytest.mark.parametrize('n_runs', (1023, 1024, 1025, RF.SCAN_SECOND - 1, RF.SCAN_SECOND, RF.SCAN_SECOND + 1))
def test_run_counts_round_the_scan_sizes(dev, n_runs):
    """one scan chunk of runs +- 1, and 256 scan chunks of runs +- 1 (the rank stage's chunk sums, scanned by the same kernel as below)"""
    m = RF.run_count_map(n_runs, 70 if n_runs < 2000 else 2049)
    want = check(dev, m, connectivity=8 if n_runs % 2 else 4)
    assert len(want.runs) == want.n == n_runs


@pytest.mark.parametrize('chunks', (RF.SCAN_SPAN - 1, RF.SCAN_SPAN, RF.SCAN_SPAN + 1, 2 * RF.SCAN_SPAN + 1))
def test_chunk_sums_round_one_workgroups_span(dev, chunks):
    """as many chunk sums as the one scanning workgroup takes in one step of its loop, +- 1: a chunk is at most 1024 pixels of one row, so
    narrow maps of that many rows, and 1025-wide ones of half as many"""
    check(dev, CF.noise_map(chunks, 3, 2, chunks), connectivity=4)
    if chunks % 2 == 0:
        m = np.zeros((chunks // 2, 1025), np.uint8)
        m[:, 1020:] = 1 + np.arange(chunks // 2)[:, None] % 2       # every row's last run crosses into its second chunk
        m[::7, 3] = 5
        assert check(dev, m, places=((3, 16),)).n == chunks // 2 + len(m[::7])


def test_empty_map_and_map_without_a_traced_class(dev):
    for h, w in ((1, 1), (70, 300)):
        want = check(dev, np.zeros((h, w), np.uint8))
        assert want.n == 0
    m = CF.blob_map(40, 50, 2, 3)
    assert check(dev, m, classes=[3, 7]).n == 0 and check(dev, np.zeros((5, 5), np.uint8), classes=[0]).n == 1
    r = R.label(torch.zeros((6, 9), dtype=torch.uint8, device=dev))
    assert r.n == 0 and tuple(r.table.shape) == (0, 16) and r.labels.dtype == torch.int32 and not r.labels.any() and r.rows() == []
    assert R.label(torch.zeros((6, 9), dtype=torch.uint8, device=dev), labels=False).labels is None


# ----------------------------------------------------------------------------------------------------------------------- contents
def test_one_region_covering_512_x_384(dev):
    """all H runs go onto one record; with weight 255 everywhere the largest wsum of the set"""
    want = check(dev, np.full((384, 512), 3, np.uint8), weight=np.full((384, 512), 255, np.uint8), places=((0, 0), (3, 5)))
    assert want.n == 1 and len(want.runs) == 384
    assert want.table[0].tolist() == [512 * 384, 0, 0, 512, 384, 384 * 511 * 512 // 2, 512 * 383 * 384 // 2, 384 * (511 * 512 * 1023 // 6),
                                      (511 * 512 // 2) * (383 * 384 // 2), 512 * (383 * 384 * 767 // 6), 2 * (512 + 384), 255 * 512 * 384, 0, 3, 1, 0]


def test_checkerboard_at_both_connectivities(dev):
    m = CF.checkerboard(33, 47, 1, 2)
    four = check(dev, m, connectivity=4, weight=m * 100)
    assert four.n == 33 * 47 and (four.area == 1).all() and (four.perim == 4).all()
    eight = check(dev, m, connectivity=8)
    assert eight.n == 2 and eight.cls.tolist() == [1, 2] and eight.perim.sum() == 4 * 33 * 47
    assert check(dev, CF.checkerboard(20, 1300, 1, 0), connectivity=8, places=((8, 16),)).n == 1


def test_long_union_chains_and_late_roots(dev):
    rings = check(dev, CF.nested_rings(40), classes=[0, 1, 2, 3], connectivity=4)
    assert rings.n == 40
    assert check(dev, CF.serpentine(65, 70)).n == 1
    combs = RF.combs(300, 1035)
    assert check(dev, combs, connectivity=8).n == 104 and check(dev, combs[:-1], connectivity=4).n == 4 * 104 - 1
    assert check(dev, np.ascontiguousarray(combs[::-1]), connectivity=8).n == 104          # the arms join in the first row
    spiral = RF.spiral(201)
    assert check(dev, spiral, connectivity=4).n == 1 and check(dev, np.ascontiguousarray(spiral[::-1, ::-1])).n == 1


def test_blob_map_512_x_384_and_the_same_bytes_twice(dev):
    m = CF.blob_map(384, 512, 3, 5)
    weight = CF.noise_map(384, 512, 255, 9)
    for conn, classes in ((8, None), (4, None), (8, (2, 3)), (4, [0, 1])):
        want = check(dev, m, classes, conn, weight if classes is None else None, places=((1, 5),) if conn == 8 else ((8, 16),))
        assert want.n > 100
    t, wt = torch.from_numpy(m).to(dev), torch.from_numpy(weight).to(dev)
    a, b = R.label(t, weight=wt), R.label(t, weight=wt)
    assert torch.equal(a.table, b.table) and torch.equal(a.labels, b.labels) and a.table.is_cuda and a.n == b.n > 1000


# ---------------------------------------------------------------------------------------------------------- the entries driven alone
def test_link_table_and_paint_alone_on_a_hand_filled_workspace(dev):
    lib = native.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    P = lambda t: native.C.c_void_p(t.data_ptr())
    m = np.where(RF.combs(40, 1100) > 0, 2, 0).astype(np.uint8)
    m[5:9, 100:130] = 5
    h, w = m.shape
    for conn in (4, 8):
        want = O.label(m, None, conn)
        n = len(want.runs)
        lay = layout(h, n)
        need = lib.wsi_region_workspace_bytes(w, h, n)
        host = np.full(FRONT + need + 64, GUARD, np.uint8)

        def put(name, a):
            raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            host[FRONT + lay[name]:FRONT + lay[name] + raw.size] = raw
        put('runs', want.runs)
        put('row_first', want.row_first)
        put('parent', np.arange(n, dtype=np.uint32))
        ws_buf = torch.from_numpy(host).to(dev)
        ws = ws_buf[FRONT:FRONT + need]
        assert lib.wsi_region_link(P(ws), need, w, h, n, conn, st) == 0
        whole = ws_buf.cpu().numpy()
        parent = ws_array(whole, lay, 'parent', n)
        root = parent.copy()
        for _ in range(64):                                     # chase the forest to its roots on the host
            root = root[root]
        assert np.array_equal(root, want.root) and np.array_equal(ws_array(whole, lay, 'up', n), want.up)
        untouched = np.ones(whole.size, bool)
        for name in ('parent', 'up'):
            untouched[FRONT + lay[name]:FRONT + lay[name] + 4 * n] = False
        assert np.array_equal(whole[untouched], host[untouched])  # the link wrote parent and up, nothing else
        # table and paint read runs, row_first, up, root and id: filled by hand, the other arrays left as guard bytes
        put('up', want.up)
        put('root', want.root)
        put('id', want.id)
        put('parent', np.full(n, 0xA5A5A5A5, np.uint32))
        ws_buf = torch.from_numpy(host).to(dev)
        ws = ws_buf[FRONT:FRONT + need]
        tab_buf, tab = guarded(dev, 128 * want.n)
        assert lib.wsi_region_table(P(ws), need, w, h, n, want.n, None, 0, P(tab), st) == 0
        assert tab.cpu().numpy().tobytes() == want.table.tobytes()
        whole = tab_buf.cpu().numpy()
        assert (whole[:FRONT] == GUARD).all() and (whole[FRONT + 128 * want.n:] == GUARD).all()
        pitch = 4 * (w + 3)
        lab_buf, lab = guarded(dev, h * pitch)
        assert lib.wsi_region_paint(P(ws), need, w, h, n, P(lab), pitch, st) == 0
        whole = lab_buf.cpu().numpy()
        inner = whole[FRONT:FRONT + h * pitch].reshape(h, pitch)
        assert np.array_equal(inner[:, :4 * w].copy().view(np.int32), want.labels) and (inner[:, 4 * w:] == GUARD).all()
        assert (whole[:FRONT] == GUARD).all() and (whole[FRONT + h * pitch:] == GUARD).all()
        assert np.array_equal(ws_buf.cpu().numpy(), host)        # both entries only read the workspace


def test_rank_reports_joined_runs_left_apart(dev):
    """the status word: a workspace whose parents were never united has as many joined pairs in different regions as the spec has joins"""
    lib = native.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    P = lambda t: native.C.c_void_p(t.data_ptr())
    m = CF.blob_map(30, 40, 2, 4)
    want = O.label(m, None, 8)
    n, h, w = len(want.runs), 30, 40
    lay, need = layout(h, n), lib.wsi_region_workspace_bytes(w, h, n)
    host = np.zeros(need, np.uint8)
    for name, a in (('runs', want.runs), ('row_first', want.row_first), ('parent', np.arange(n, dtype=np.uint32))):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        host[lay[name]:lay[name] + raw.size] = raw
    ws = torch.from_numpy(host).to(dev)
    counts = torch.full((2,), 77, dtype=torch.int32, device=dev)
    assert lib.wsi_region_rank(P(ws), need, w, h, n, 8, P(counts), st) == 0
    y, x0, x1, cls = (want.runs[:, k].astype(np.int64) for k in range(4))
    assert counts.tolist() == [n, len(O.joins_of(y, x0, x1, cls, want.row_first.astype(np.int64), 1))] and counts[1] > 0
    assert lib.wsi_region_link(P(ws), need, w, h, n, 8, st) == 0 and lib.wsi_region_rank(P(ws), need, w, h, n, 8, P(counts), st) == 0
    assert counts.tolist() == [want.n, 0]


# ------------------------------------------------------------------------------------------------------------- the Python layer
def test_remove_small_overlaps_lesion_scores_equal_the_spec(dev):
    a, b = CF.blob_map(90, 120, 3, 21, radius=2), CF.blob_map(90, 120, 3, 22, radius=2)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    for conn, classes, fill in ((8, None, 0), (4, (2, 3), 7)):
        got = R.remove_small(ta, 15, conn, classes, fill)
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), O.remove_small(a, 15, conn, classes, fill))
    assert (R.remove_small(ta, 15) != ta).any() and torch.equal(R.remove_small(ta, 1), ta)
    ra, rb = R.label(ta), R.label(tb, connectivity=4)
    ov = R.overlaps(ra, rb)
    assert ov.is_cuda and ov.dtype == torch.int64 and np.array_equal(ov.cpu().numpy(), O.overlaps(O.label(a).labels, O.label(b, None, 4).labels)) and len(ov) > 20
    for kw in (dict(), dict(classes=(2, 3)), dict(classes=(2, 3), connectivity=4, iou=0), dict(iou=0.1, min_area=10), dict(classes=[1], iou=1 / 3)):
        assert R.lesion_scores(ta, tb, **kw) == O.lesion_scores(a, b, **kw), kw
    assert R.lesion_scores(ta, ta)['f1'] == 1.0 and R.lesion_scores(ta, torch.zeros_like(ta))['precision'] == 0.0
    assert R.lesion_scores(ta, tb, iou=0.1)['tp_gt'] > 0


def test_slide_positive_equals_the_spec(dev):
    heat = np.zeros((150, 200), np.uint8)
    heat[20:90, 30:110] = 254
    heat[100:140, 120:190] = 255                                 # 40 rows: the 50 x 50 opening removes it
    heat[60:130, 150:152] = 253
    heat[25, 40] = 252                                           # a hole in the first block: the opening takes more than the pixel
    want, spec = O.slide_positive(heat)
    got = R.slide_positive(torch.from_numpy(heat).to(dev))
    assert got == want and got['positive'] and got['n_regions'] >= 1 and 0 < got['fraction'] < 70 * 80 / heat.size
    assert R.slide_positive(torch.from_numpy(np.minimum(heat, 252)).to(dev)) == dict(positive=False, fraction=0.0, n_regions=0, largest_area=0)
    for kw in (dict(open_k=30), dict(thresh=1.0, open_k=5), dict(open_k=30, min_fraction=0.5)):
        assert R.slide_positive(torch.from_numpy(heat).to(dev), **kw) == O.slide_positive(heat, **kw)[0], kw
    res, r = R._slide_positive(torch.from_numpy(heat).to(dev), 0.99, 50, 0.0)
    assert r.table.cpu().numpy().tobytes() == spec.table.tobytes() and r.wsum.sum() > 0


# ----------------------------------------------------------------------------------------------------------------------- the hooks
GREYS = (225, 165, 105, 45)                                      # the slide's grey of class 0 .. 3


def _args(monkeypatch, tmp_path, hw, mask_value=255):
    import myargs
    from PIL import Image
    for k, v in (('scan_level', 0), ('scan_resize', 1), ('num_classes', 4), ('class_probs', [0., 0., 0., 0.]), ('tile_w', 64), ('tile_h', 64),
                 ('tile_stride_w', 64), ('tile_stride_h', 64), ('val_save_pth', str(tmp_path / 'out')), ('wsi_mask_pth', str(tmp_path / 'nomask'))):
        monkeypatch.setattr(myargs.args, k, v)
    os.makedirs(str(tmp_path / 'nomask'))
    Image.fromarray(np.full(hw, mask_value, np.uint8)).save(str(tmp_path / 'nomask' / 'case.svs.png'))     # every tile is foreground
    return myargs.args


def _grey_slide(gt):
    l2 = np.repeat(np.asarray(GREYS, np.uint8)[gt][..., None], 3, -1)
    slide = ArraySlide([np.repeat(np.repeat(l2, 16, 0), 16, 1), np.repeat(np.repeat(l2, 4, 0), 4, 1), l2], [1.0, 4.0, 16.0])
    slide.name = 'case.svs'
    return slide


def test_predict_wsis_region_table(dev, tmp_path, monkeypatch):
    """the slide and the one-layer dense model of tests/test_gpu_edt.py: the table is the spec's on the returned class map, the CSV read
    back holds its rows in level-0 coordinates, the lesion scores are the spec's, and the results are equal with the keyword unset"""
    import utils.dataset as ds
    import utils.eval as val
    args = _args(monkeypatch, tmp_path, (48, 64))
    gt = CF.blob_map(48, 64, 3, 33, radius=3)
    gt[20:40, 20:50] = 3
    slide = _grey_slide(gt)
    centres = torch.tensor([(g / 255.0 - args.dataset_mean[0]) / args.dataset_std[0] for g in GREYS], device=dev)

    class ReadsTheGrey(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):                                     # (B, 3, h, w) -> (B, 4, h, w): minus the distance to each class's grey
            return -(x[:, :1] - centres.view(1, 4, 1, 1)).abs()

    model = ReadsTheGrey().to(dev)
    params = {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}
    truth = gt.copy()
    truth[0:12, 40:64] = 0                                      # the pathologist left some lesions out
    truth[42:47, 2:9] = 2                                       # and drew one the model does not see

    def run(ep, **kw):
        dataset = ds.Dataset_wsis({'case.svs': slide}, params, bs=64)
        dataset.wsis['case.svs']['gt'] = torch.from_numpy(truth).to(dev)
        return val.predict_wsis(model, dataset, ep, **kw)['case.svs']

    out = str(tmp_path / 'out')
    plain = run(1)
    parent_keys = {'acc', 's', 'acc_masked', 's_masked', 'iou_fg', 'iou_tb'}
    assert set(plain['scores']) == parent_keys and 'regions' not in plain and not os.path.exists(out + '/1/case.svs_64_regions.csv')
    res = run(2, region_table=True)
    assert set(res) == set(plain) | {'regions'} and torch.equal(res['classes_level2'], plain['classes_level2'])
    assert {k: res['scores'][k] for k in parent_keys} == plain['scores']
    assert open(out + '/2/case.svs_64.png', 'rb').read() == open(out + '/1/case.svs_64.png', 'rb').read()
    p = res['classes_level2'].cpu().numpy()
    want = O.label(p, (1, 2, 3), 8)
    assert want.n > 3 and res['regions'].n == want.n and res['regions'].table.cpu().numpy().tobytes() == want.table.tobytes()
    ls = O.lesion_scores(p, truth, (2, 3))
    sc = res['scores']
    assert set(sc) == parent_keys | {'lesions_pred', 'lesions_gt', 'lesion_precision', 'lesion_recall', 'lesion_f1'}
    assert (sc['lesions_pred'], sc['lesions_gt'], sc['lesion_precision'], sc['lesion_recall'], sc['lesion_f1']) == (
        ls['n_pred'], ls['n_gt'], ls['precision'], ls['recall'], ls['f1'])
    assert 0 < ls['tp_gt'] and (ls['fn'] > 0 or ls['fp'] > 0)
    rows = list(csv.DictReader(open(out + '/2/case.svs_64_regions.csv')))
    assert len(rows) == want.n and list(rows[0]) == list(R.CSV_COLUMNS)
    for k, row in enumerate(rows):                               # level-0 coordinates: the map's step is 16; the slide states no mpp
        assert [int(row[c]) for c in ('id', 'class', 'area_px', 'x0', 'y0', 'x1', 'y1', 'perim')] == [
            k + 1, want.cls[k], want.area[k], 16 * want.x0[k], 16 * want.y0[k], 16 * want.x1[k], 16 * want.y1[k], want.perim[k]]
        assert row['area_um2'] == '' and row['name'] == {1: 'Benign', 2: 'In situ', 3: 'Invasive'}[int(row['class'])]
    slide.mpp = 0.25
    run(3, region_table=True)
    rows = list(csv.DictReader(open(out + '/3/case.svs_64_regions.csv')))
    assert [float(r['area_um2']) for r in rows] == [float(a) * 16 * 16 * 0.0625 for a in want.area]
    del slide.mpp
    # without gt the flag adds the table and no scores
    dataset = ds.Dataset_wsis({'case.svs': slide}, params, bs=64)
    alone = val.predict_wsis(model, dataset, 4, save=False, region_table=True)['case.svs']
    assert alone['scores'] is None and alone['regions'].n == want.n and not os.path.exists(out + '/4')


def test_predict_tumorbed_region_table(dev, tmp_path, monkeypatch):
    """an 80 x 80 map whose 60 x 60 tumour block survives the 50 x 50 opening, classified tile by tile by a model that reads the grey:
    slide_positive and the regions are the spec's on the returned heat map; unset, the results are what they were"""
    import utils.dataset as ds
    import utils.eval as val
    args = _args(monkeypatch, tmp_path, (80, 80), mask_value=1)     # the heat map is the probability times the mask's value
    gt = np.zeros((80, 80), np.uint8)
    gt[8:68, 12:72] = 1                                         # mode 'cls' takes the heat from class 1
    gt[72:76, 0:8] = 1                                          # a speck the opening removes
    slide = _grey_slide(gt)
    centres = torch.tensor([(g / 255.0 - args.dataset_mean[0]) / args.dataset_std[0] for g in GREYS], device=dev)

    class Encoder(torch.nn.Module):
        def forward(self, x):
            return (x[:, :1].mean((2, 3)),)

    class Head(torch.nn.Module):
        def forward(self, f):                                     # (B, 1) -> (B, 4): a confident vote for the class of the tile's grey
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
    assert 'regions' not in plain and 'slide_positive' not in plain and not os.path.exists(out + '/1/case.svs_64_heatmap_regions.csv')
    res = val.predict_tumorbed(model, ds.Dataset_wsis({'case.svs': slide}, params, bs=64), 2, mode='cls', region_table=True)['case.svs']
    assert set(res) == set(plain) | {'regions', 'slide_positive'} and np.array_equal(res['heatmap'], plain['heatmap'])
    heat = np.asarray(res['heatmap'])
    want, spec = O.slide_positive(heat)
    assert res['slide_positive'] == want and want['positive'] and want['n_regions'] == 1 and want['largest_area'] == 3600
    # cv2's opening with an even kernel (anchor k // 2 in both passes) moves the block one pixel down and right: 59 x 59 of its pixels are hot
    wsum = int(heat[9:69, 13:73].astype(np.int64).sum())
    assert res['regions'].table.cpu().numpy().tobytes() == spec.table.tobytes() and spec.table[0, O.F['wsum']] == wsum == 255 * 59 * 59
    assert spec.table[0, O.F['x0']:O.F['y1'] + 1].tolist() == [13, 9, 73, 69]
    rows = list(csv.DictReader(open(out + '/2/case.svs_64_heatmap_regions.csv')))
    assert len(rows) == 1 and (rows[0]['name'], int(rows[0]['area_px']), int(rows[0]['x0']), int(rows[0]['y1'])) == ('Invasive', 3600, 13 * 16, 69 * 16)
    assert rows[0]['mean_weight'] == '%.4f' % (wsum / 3600)
