"""GPU side of the boundary tracer (csrc/contour.hip through wsi_segmentation_pipeline_amd.contours): every case byte for byte equal to the
spec (tests/contours_oracle.py) - vertices, loop records and area2 inside 0xA5 guards, the map inside guards at four base alignments and a
pitch > W and never written - and back through the GPU rasteriser to the map; then the writer, the reader's `negative` keyword and the
two save_xml hooks."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import annotation_fixture as AF                                # noqa: E402
import contour_fixture as F                                    # noqa: E402
import contours_oracle as O                                    # noqa: E402
from wsi_segmentation_pipeline_amd import annotations as A, contours as CT     # noqa: E402
from wsi_segmentation_pipeline_amd.slide import ArraySlide     # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0xA5
PLACES = ((0, 0), (1, 5), (3, 5), (8, 5))                       # (bytes before the map's first byte, pitch - W)


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
    return torch.as_strided(buf, (h, w), (pitch, 1), offset), buf, host


def check(dev, m, classes=None, step=(2, 2), origin=(0, 0), bounds=None, places=PLACES, want=None, round_trip=True):
    """trace `m` at every placement into guarded outputs: the spec's bytes, nothing past n_vertices / n_loops, the map's allocation
    untouched; and painted back by the GPU rasteriser the loops give where(traced[m], m, 0)"""
    m = np.ascontiguousarray(m, np.uint8)
    want = O.trace(m, classes, step, origin, bounds) if want is None else want
    table = CT.traced_table(classes)
    for offset, extra in places:
        view, buf, host = place(dev, m, offset, extra)
        bufs = []

        def alloc(nv, nl):
            guarded = lambda nbytes: torch.full((nbytes,), GUARD, dtype=torch.uint8, device=dev)
            bufs.extend([guarded(8 * (nv + 7)).view(torch.int32).view(nv + 7, 2), guarded(32 * (nl + 5)).view(torch.int32).view(nl + 5, 8),
                         guarded(8 * (nl + 5)).view(torch.int64)])
            return tuple(bufs)
        v, rec, a2, ne = CT.trace_raw(view, table, step, origin, bounds, alloc=alloc)
        assert ne == int(want.edges.sum()) and len(v) == len(want.vertices) and len(rec) == len(want.first), (offset, extra, ne, len(v), len(rec))
        assert np.array_equal(v.cpu().numpy(), want.vertices), (offset, extra)
        assert np.array_equal(rec.cpu().numpy(), want.records()) and np.array_equal(a2.cpu().numpy(), want.area2), (offset, extra)
        for b, n in zip(bufs, (len(v), len(rec), len(rec))):    # nothing is written past n_vertices / n_loops
            assert (b[n:].contiguous().view(torch.uint8) == GUARD).all()
        assert np.array_equal(buf.cpu().numpy(), host)           # the map is never written, nor a byte round it
    if round_trip and len(want.first):
        c = CT.Contours(v, rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], a2, m.shape[::-1], step, origin, bounds)
        coords, labels = c.paint_list()
        back = A.rasterize(coords, labels, m.shape[::-1], step, origin, device=dev).cpu().numpy()
        assert int((back != F.traced_part(m, table)).sum()) == 0
    return want


# ------------------------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize('w', (1, 15, 16, 17, 129))
def test_widths_and_heights_round_the_16_byte_piece(dev, w):
    edges = 0
    for h in (1, 2, 33):
        edges += int(check(dev, F.noise_map(h, w, 3, 100 * w + h)).edges.sum())
    assert edges > 0


@pytest.mark.parametrize('w,h', ((1022, 2), (1023, 3), (1024, 2), (2050, 3), (1, 1100), (340, 7), (341, 7)))
def test_corner_chunks(dev, w, h):
    """the corner walk's chunk: whole corner rows while W + 1 <= 1024 (340 -> 3 rows, 341 -> 2; 1 x 1100: 512 rows a chunk, three
    chunks), pieces of one row beyond (1024 -> 2 pieces, the second of one corner; 2050 -> 3)"""
    want = check(dev, F.noise_map(h, w, 3, w + h), places=PLACES[1:3])
    assert int(want.edges.sum()) > 100


def test_empty_and_uniform_maps(dev):
    for m in (np.zeros((1, 1), np.uint8), np.zeros((37, 53), np.uint8)):
        want = check(dev, m)
        assert len(want.first) == 0 and len(want.vertices) == 0
    c = CT.trace(torch.zeros((9, 20), dtype=torch.uint8, device=dev))
    assert len(c) == 0 and tuple(c.vertices.shape) == (0, 2) and c.vertices.is_cuda and c.loops() == [] and c.paint_list() == ([], [])
    assert tuple(c.area2.shape) == (0,) and c.area2.dtype == torch.int64 and c.first.dtype == torch.int32
    want = check(dev, np.full((37, 53), 3, np.uint8), step=(16, 16), origin=(-40, 8))
    assert want.vertices.tolist() == [[-48, 0], [800, 0], [800, 592], [-48, 592]] and want.edges.tolist() == [180] and want.area2.tolist() == [2 * 37 * 53]
    check(dev, np.full((37, 53), 3, np.uint8), classes=[1, 2])   # nothing traced


@pytest.mark.parametrize('n_edges', (F.SCAN_CHUNK - 2, F.SCAN_CHUNK, F.SCAN_CHUNK + 2, F.SCAN_SECOND - 2, F.SCAN_SECOND, F.SCAN_SECOND + 2))
def test_edge_counts_round_the_scan_sizes(dev, n_edges):
    """n_edges just below, at and just above what one workgroup scans and what the scanning workgroup covers per step (a map's edge count
    is even: every loop has as many edges east as west, south as north - so the neighbours are two away)"""
    small = n_edges < 4096
    want = check(dev, F.edge_count_map(n_edges, 40 if small else 384, 40 if small else 512), places=PLACES[1:2])
    assert int(want.edges.sum()) == n_edges


@pytest.mark.parametrize('h', (F.SCAN_SPAN - 2, F.SCAN_SPAN - 1, F.SCAN_SPAN, 2 * F.SCAN_SPAN))
def test_corner_chunk_sums_round_one_workgroups_span(dev, h):
    """the count stage's chunk sums, as many as the one scanning workgroup takes in one step of its loop - 1, + 0, + 1 and twice that + 1:
    a 1023-wide map has one corner row of 1024 corners per chunk and H + 1 chunks.  Sparse maps, so the spec is quick."""
    want = check(dev, F.sparse_rectangles(h, 1023), places=PLACES[1:2])
    assert len(want.first) == 6 and int(want.edges.sum()) == 102


def test_edge_scans_past_one_step_of_the_scanning_workgroup(dev):
    """n_edges just above SCAN_STEP = 1024 x 1024: the u32 scan of the vertex flags and both u64 scans (loops, cross terms) have more chunk
    sums than the scanning workgroup takes in one step.  Isolated pixels, expected in closed form (pinned to the spec at small sizes in
    tests/test_contours_cpu.py); 262 656 loops are too many for the round trip's Python, which other tests make."""
    h, w = 1024, 1026
    t = F.isolated_pixels_trace(h, w, (2, 2), (0, 0))
    want = O.Traced(t['vertices'], t['first'], t['count'], t['edges'], t['label'], t['area2'], (w, h), (2, 2), (0, 0), None)
    assert F.SCAN_STEP < int(want.edges.sum()) == 4 * 513 * 512 < F.SCAN_STEP + 3 * F.SCAN_CHUNK
    check(dev, F.isolated_pixels(h, w), want=want, places=PLACES[1:2], round_trip=False)


@pytest.mark.parametrize('edges', (4, 6, 8, 510, 512, 514))
def test_single_loops_round_a_doubling_round(dev, edges):
    """one loop is the whole map, so n_edges is its length: 512 takes 9 rounds and covers the loop exactly, 514 takes the 10th"""
    want = check(dev, F.row_loop(edges), places=PLACES[:2])
    assert want.edges.tolist() == [edges] and want.count.tolist() == [4]


def test_short_loops_inside_a_long_table(dev):
    m = np.zeros((40, 64), np.uint8)
    m[1, 1], m[1, 3:5], m[1, 6:9] = 1, 2, 3                      # loops of 4, 6 and 8 edges before
    m[3:39:2] = 1                                               # many of 130
    want = check(dev, m)
    assert want.edges.tolist()[:3] == [4, 6, 8] and set(want.edges.tolist()[3:]) == {130}


def test_serpentine_loop_longer_than_2_to_the_16(dev):
    m = F.serpentine(299, 299)
    want = check(dev, m, places=PLACES[2:3])
    assert want.edges.tolist() == [F.serpentine_edges(299, 299)] and want.edges[0] > 1 << 16      # 17 rounds; the rank wraps at the start


def test_two_label_checkerboard(dev):
    want = check(dev, F.checkerboard(96, 96, 1, 2), places=PLACES[1:2])
    assert len(want.first) == 96 * 96 > 8000 and int(want.edges.sum()) == 4 * 96 * 96 and (want.edges == 4).all()


def test_nested_rings(dev):
    want = check(dev, F.nested_rings(40), places=PLACES[3:])
    assert len(want.first) >= 50 and (want.area2 < 0).sum() >= 20
    assert len(set(np.abs(want.area2).tolist())) < len(want.area2)           # ties between a hole and what fills it


def test_blob_map_512_x_384(dev):
    want = check(dev, F.blob_map(384, 512, 3, 5), step=(16, 16), places=PLACES[1:2])
    assert int(want.edges.sum()) > 100000 and len(want.first) > 1000 and set(want.label.tolist()) == {1, 2, 3}


@pytest.mark.parametrize('classes', ([0], [0, 2], [3], [1, 2], [200]))
def test_class_subsets(dev, classes):
    want = check(dev, F.blob_map(96, 130, 3, 8), classes=classes, places=PLACES[1:2])
    assert set(want.label.tolist()) == set(classes) - {200}


@pytest.mark.parametrize('step,origin', (((2, 3), (-7, -5)), ((16, 16), (-100, -3)), ((5, 2), (0, 0))))
def test_steps_origins_and_clamped_bounds(dev, step, origin):
    m = F.blob_map(45, 70, 3, 21, radius=2)
    m[0, :], m[:, -1], m[-1, 10:20] = 1, 2, 3                    # labels on the map's border: corners the clamp moves
    check(dev, m, step=step, origin=origin, places=PLACES[1:2])
    bounds = (69 * step[0] + 1, 44 * step[1] + 1)               # the slide ends inside the last pixel's cell: (W - 1) sx < W0 <= W sx
    want = check(dev, m, step=step, origin=(0, 0), bounds=bounds, places=PLACES[2:3])
    assert want.vertices.min() == 0 and want.vertices[:, 0].max() == bounds[0] - 1 and want.vertices[:, 1].max() == bounds[1] - 1
    check(dev, m, step=(1, 1), origin=origin, places=PLACES[:1], round_trip=False)      # step 1 traces; it does not round-trip


def test_same_call_twice_gives_the_same_bytes(dev):
    m = torch.from_numpy(F.blob_map(200, 300, 3, 9)).to(dev)
    a, b = CT.trace(m, step=4), CT.trace(m, step=4)
    for x, y in ((a.vertices, b.vertices), (a.first, b.first), (a.count, b.count), (a.edges, b.edges), (a.label, b.label), (a.area2, b.area2)):
        assert torch.equal(x, y) and x.is_cuda
    assert len(a) > 100 and a.vertices.dtype == torch.int32 and tuple(a.vertices.shape) == (int(a.count.sum()), 2)


def test_min_area_equals_the_spec(dev):
    m = F.blob_map(120, 160, 3, 4)
    md = torch.from_numpy(m).to(dev)
    full = O.trace(m, None, 4)
    assert (np.abs(full.area2) < 12).any() and (np.abs(full.area2) >= 12).any()
    for a in (6, 50, 200):
        want, got = O.trace(m, None, 4, min_area=a), CT.trace(md, step=4, min_area=a)
        assert np.array_equal(got.vertices.cpu().numpy(), want.vertices) and np.array_equal(got.area2.cpu().numpy(), want.area2)
        for x, y in ((got.first, want.first), (got.count, want.count), (got.edges, want.edges), (got.label, want.label)):
            assert np.array_equal(x.cpu().numpy(), y)
        assert len(want.first) < len(full.first)
        back = A.rasterize(*got.paint_list(), (160, 120), 4, device=dev).cpu().numpy()     # the painter's order stays valid:
        dropped = (int(np.abs(full.area2).sum()) - int(np.abs(want.area2).sum())) // 2      # pixels change only inside a dropped loop
        assert 0 < int((back != m).sum()) <= dropped


# ----------------------------------------------------------------------------------------------------------------------- drivers
def test_write_read_rasterize_restores_the_map(dev, tmp_path):
    m = F.blob_map(90, 140, 3, 17, radius=2)
    c = CT.trace(torch.from_numpy(m).to(dev), step=8, origin=(-3, 5))
    assert (c.area2 < 0).any()
    p = CT.write_imagescope(str(tmp_path / 'pred.xml'), c, mpp=0.25)
    coords, labels, _, area, mpp = A.read_imagescope(p, negative='erase')
    assert mpp == 0.25 and 0 in labels and len(coords) == len(c)
    assert np.array_equal(A.rasterize(coords, labels, (140, 90), 8, (-3, 5), device=dev).cpu().numpy(), m)
    assert sum(area) > 0


def test_rasterize_trace_rasterize_is_the_identity_on_the_annotation_corpus(dev, tmp_path):
    cases = [c for c in AF.shape_cases() + AF.painter_cases() + AF.geometry_cases() if min(c['step']) >= 2 and c['fill'] == 0]
    assert len(cases) >= 40
    traced = 0
    for c in cases:
        first = A.rasterize(c['coords'], c['labels'], c['size'], c['step'], c['origin'], device=dev)
        t = CT.trace(first, None, c['step'], c['origin'])
        again = A.rasterize(*t.paint_list(), c['size'], c['step'], c['origin'], device=dev)
        assert torch.equal(first, again), c['name']
        traced += len(t)
    assert traced >= len(cases)
    # level_map of the XML fixture at two levels of a slide
    isc = str(tmp_path / 'imagescope.xml')
    AF.write_imagescope(isc)
    coords, labels = A.read_imagescope(isc)[:2]
    scan = ArraySlide([np.zeros((h, w, 3), np.uint8) for w, h in ((512, 432), (128, 108), (32, 27))], [1.0, 4.0, 16.0])
    for level in (1, 2):
        gt = A.level_map(coords, labels, scan, level, dev)
        t = CT.trace(gt, None, A.level_step(scan, level), bounds=scan.level_dimensions[0])
        assert set(t.label.tolist()) == {1, 2, 3}
        assert torch.equal(A.level_map(*t.paint_list(), scan, level, dev), gt)


def _args(monkeypatch, tmp_path):
    import myargs
    for k, v in (('scan_level', 0), ('scan_resize', 1), ('num_classes', 4), ('class_probs', [0., 0., 0., 0.]), ('tile_w', 64), ('tile_h', 64),
                 ('tile_stride_w', 64), ('tile_stride_h', 64), ('val_save_pth', str(tmp_path / 'out')), ('wsi_mask_pth', str(tmp_path / 'nomask'))):
        monkeypatch.setattr(myargs.args, k, v)
    return myargs.args


GREYS = (225, 165, 105, 45)                                      # the slide's grey of class 0 .. 3


def test_predict_wsis_save_xml(dev, tmp_path, monkeypatch):
    """an ArraySlide whose 16 x 16 blocks carry the grey of a class and a model that reads the grey: the XML the hook writes, read back and
    rasterised at the hook's step, is the class map the hook traced; the tumour bed sits in a second Annotation no reader visits"""
    import xml.etree.ElementTree as ET
    import utils.dataset as ds
    import utils.eval as val
    from PIL import Image
    from wsi_segmentation_pipeline_amd import engine as E
    args = _args(monkeypatch, tmp_path)
    os.makedirs(str(tmp_path / 'nomask'))
    Image.fromarray(np.full((48, 64), 255, np.uint8)).save(str(tmp_path / 'nomask' / 'case.svs.png'))     # every tile is foreground
    gt = F.blob_map(48, 64, 3, 33, radius=3)
    gt[20:40, 20:50] = 3                                        # a tumour large enough to survive the 20 x 20 opening
    l2 = np.repeat(np.asarray(GREYS, np.uint8)[gt][..., None], 3, -1)
    slide = ArraySlide([np.repeat(np.repeat(l2, 16, 0), 16, 1), np.repeat(np.repeat(l2, 4, 0), 4, 1), l2], [1.0, 4.0, 16.0])
    slide.name = 'case.svs'
    centres = torch.tensor([(g / 255.0 - args.dataset_mean[0]) / args.dataset_std[0] for g in GREYS], device=dev)

    class ReadsTheGrey(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return -(x[:, :1] - centres.view(1, 4, 1, 1)).abs()

    params = {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}
    out = str(tmp_path / 'out')
    model = ReadsTheGrey().to(dev)
    res = val.predict_wsis(model, ds.Dataset_wsis({'case.svs': slide}, params, bs=64), 1)['case.svs']
    assert os.path.exists(out + '/1/case.svs_64.png') and not os.path.exists(out + '/1/case.svs_64.xml')     # off by default
    dataset = ds.Dataset_wsis({'case.svs': slide}, params, bs=64)
    mask = dataset.wsis['case.svs']['mask']
    keep = val._map_u8(mask, (48, 64), dev).cpu().numpy() > 0 if mask is not None else np.ones((48, 64), bool)
    res2 = val.predict_wsis(model, dataset, 2, save_xml=True)['case.svs']
    assert torch.equal(res['classes_level2'], res2['classes_level2'])
    assert open(out + '/2/case.svs_64.png', 'rb').read() == open(out + '/1/case.svs_64.png', 'rb').read()
    # the map the hook was given: the thresholded classes on the foreground mask, what the PNG shows
    shown = E.softmax_threshold_argmax(res2['pred_level2'], args.class_probs, want_probs=False)[0].cpu().numpy() * keep
    assert int((shown > 0).sum()) > 200 and shown.max() <= 3
    p = out + '/2/case.svs_64.xml'
    coords, labels, _, _, mpp = A.read_imagescope(p, negative='erase')
    assert mpp == 1.0                                           # the slide states none
    assert np.array_equal(A.rasterize(coords, labels, (64, 48), 16, device=dev).cpu().numpy(), shown)
    assert max(np.asarray(c).max() for c in coords) <= 1023 and min(np.asarray(c).min() for c in coords) >= 0
    root = ET.parse(p).getroot()
    assert len(root) == 2 and {r[0][0].get('Value') for r in root[1][1]} == {'Invasive'}
    bed = [[[int(v.get('X')), int(v.get('Y'))] for v in r[1]] for r in root[1][1]]
    bed_labels = [0 if r.get('NegativeROA') == '1' else 1 for r in root[1][1]]
    tb = res2['tumor_bed'].cpu().numpy() > 0
    assert tb.any() and np.array_equal(A.rasterize(bed, bed_labels, (64, 48), 16, device=dev).cpu().numpy() > 0, tb)


def test_predict_tumorbed_save_xml(dev, tmp_path, monkeypatch):
    import resnets_shift
    import stain_oracle as SO
    import utils.dataset as ds
    import utils.eval as val
    from models.models import Classifier
    from wsi_segmentation_pipeline_amd import postprocess as PP, synthetic as W
    _args(monkeypatch, tmp_path)
    l0 = SO.shifted_he(31, 1, 512)[0]
    slide = ArraySlide([l0, np.ascontiguousarray(l0[::4, ::4]), np.ascontiguousarray(l0[::16, ::16])], [1.0, 4.0, 16.0])
    slide.name = 'case.svs'
    net = resnets_shift.resnet18(False)
    net.load_state_dict(W.make_resnet18_state_dict(11, with_fc=False), strict=False)
    head = Classifier(512, 4)
    head.load_state_dict(W.make_head_state_dict(22, 'classifier'))
    model = val.SlideClassifierModel(net, head).to(dev)
    params = {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}
    out = str(tmp_path / 'out')
    val.predict_tumorbed(model, ds.Dataset_wsis({'case.svs': slide}, params, bs=16), 1, mode='cls')
    assert os.path.exists(out + '/1/case.svs_64_heatmap.png') and not os.path.exists(out + '/1/case.svs_64_tb.xml')
    res = val.predict_tumorbed(model, ds.Dataset_wsis({'case.svs': slide}, params, bs=16), 2, mode='cls', save_xml=True)['case.svs']
    heat = torch.from_numpy(np.asarray(res['heatmap'])).to(dev)
    bed = (PP.tumor_bed_from_heatmap(heat, 0.9, 30, 20).tb_pred > 0).to(torch.uint8)      # the map the hook traced
    coords, labels = A.read_imagescope(out + '/2/case.svs_64_tb.xml', negative='erase')[:2]
    assert set(labels) <= {0, 3}                                # 'Invasive'
    got = A.rasterize(coords, labels, (32, 32), 16, device=dev)
    assert torch.equal((got > 0).to(torch.uint8), bed)
