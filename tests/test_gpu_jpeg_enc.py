"""GPU tests of the JPEG encode path (csrc/jpeg_enc.hip, tiffwrite.py): scan bytes and sizes against Pillow with 0 differences, the
size pass against the write pass against the spec with guard bytes around every range, the box downsample against NumPy, the written
pyramid read back on the device, and the driver hooks.

Tile sizes (width x height): 16 x 16 (one 4:2:0 MCU), 64 x 48, 256 x 256 (one transform segment of 16 MCUs at 4:2:0 / 4:2:2, two at
4:4:4 and grey) and 272 x 32 (a second, short segment in every sampling).  Every reference is encoded once by Pillow, the edge tiles
from np.pad(mode='edge').  No kernel here splits its work over launches or grid dimensions: the transform is one launch over one grid
dimension (a batch that would pass 2^31 - 1 workgroups is refused with -22), the entropy passes one workgroup per `lanes` tiles."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import jpeg_enc_oracle as E
import jpeg_oracle as O
import tiff_fixture as TF
from wsi_segmentation_pipeline_amd import native, tiffwrite as TW
from wsi_segmentation_pipeline_amd.tiffslide import TiffSlide

pytestmark = pytest.mark.gpu
SS = {None: (1, 1), 0: (1, 1), 1: (2, 1), 2: (2, 2)}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


def _scan(stream):
    d = O.parse(stream)
    return stream[d['scan_off']:d['scan_off'] + d['scan_len']]


def pillow_scans(level, tile, quality, ss, restart=0):
    """the scan bytes Pillow writes for every tile of the level's grid, raster order; edge tiles padded by np.pad(mode='edge')"""
    tw, th = tile
    padded = TF.pad_to_tiles(level, tw, th)
    return [_scan(TF.encode(np.ascontiguousarray(padded[y:y + th, x:x + tw]), quality, 0 if ss is None else ss, restart))
            for y in range(0, padded.shape[0], th) for x in range(0, padded.shape[1], tw)]


def device_scans(level, **kw):
    offs, sizes, scan = TW.encode_level(level, **kw)
    assert (offs % 16 == 0).all() and len(offs) == len(sizes)
    host = scan.cpu().numpy()
    return [host[int(o):int(o) + int(s)].tobytes() for o, s in zip(offs, sizes)]


def _level(w, h, ss, seed, kind=TF.he_like):
    return kind(h, w, seed, 1 if ss is None else 3)


@pytest.mark.parametrize('ss', (None, 0, 1, 2), ids=lambda v: 'grey' if v is None else 'ss%d' % v)
@pytest.mark.parametrize('tile', ((16, 16), (64, 48), (256, 256), (272, 32)), ids=lambda v: '%dx%d' % v)
def test_tile_scans_equal_pillow(dev, tile, ss):
    tw, th = tile
    for k, (kind, q) in enumerate(((TF.he_like, 75), (TF.noise, 90))):
        lv = _level(2 * tw, 2 * th if tw < 256 else th, ss, 10 + k, kind)
        got = device_scans(torch.from_numpy(lv).to(dev), tile=tile, quality=q, subsampling=SS[ss])
        want = pillow_scans(lv, tile, q, ss)
        assert [len(g) for g in got] == [len(w) for w in want]
        assert got == want


@pytest.fixture(scope='module')
def tiles65():
    """65 distinct 16 x 16 tiles side by side and Pillow's scans of them (4:2:0, quality 75)"""
    lv = np.concatenate([TF.noise(16, 16, 300 + k) if k % 3 else TF.he_like(16, 16, 300 + k) for k in range(65)], 1)
    return lv, pillow_scans(lv, (16, 16), 75, 2)


@pytest.mark.parametrize('lanes', (0, 64))
@pytest.mark.parametrize('n', (1, 63, 64, 65))
def test_batch_sizes_around_a_wave(dev, tiles65, n, lanes):
    lv, want = tiles65
    got = device_scans(torch.from_numpy(np.ascontiguousarray(lv[:, :16 * n])).to(dev), tile=(16, 16), quality=75, subsampling=(2, 2), lanes=lanes)
    assert got == want[:n]


def test_several_batches_under_a_small_workspace(dev, tiles65):
    """a byte budget of five tiles: thirteen batches, the offsets running on from batch to batch"""
    lv, want = tiles65
    tile_ws = native.load().wsi_jenc_workspace_bytes(16, 16, 3, 2, 2)
    assert device_scans(torch.from_numpy(lv).to(dev), tile=(16, 16), quality=75, subsampling=(2, 2), workspace_bytes=5 * tile_ws) == want


def _misaligned(dev, lv, offset, extra):
    """the level at byte `offset` of a larger 0x5A buffer, rows `extra` bytes apart beyond their own"""
    h, w = lv.shape[:2]
    c = 1 if lv.ndim == 2 else 3
    pitch = w * c + extra
    buf = torch.full((offset + h * pitch + 64,), 0x5A, dtype=torch.uint8, device=dev)
    view = torch.as_strided(buf, (h, w, c) if c == 3 else (h, w), (pitch, c, 1) if c == 3 else (pitch, 1), offset)
    view.copy_(torch.from_numpy(lv).to(dev))
    return view


@pytest.mark.parametrize('ss', (None, 0, 1, 2), ids=lambda v: 'grey' if v is None else 'ss%d' % v)
@pytest.mark.parametrize('w,h,tile', ((70, 50, (32, 32)), (10, 7, (16, 16)), (10, 7, (32, 32))))
def test_edge_tiles_clamp_and_misaligned_level(dev, w, h, tile, ss):
    """a level that is no multiple of the tile (and one smaller than a tile): pixels outside it repeat the nearest level pixel, as
    np.pad(mode='edge') does; the level's base at an odd byte inside a larger buffer, its pitch larger than the row and odd"""
    lv = _level(w, h, ss, 40 + w, TF.noise)
    want = pillow_scans(lv, tile, 80, ss)
    for offset, extra in ((0, 0), (13, 7)):
        assert device_scans(_misaligned(dev, lv, offset, extra), tile=tile, quality=80, subsampling=SS[ss]) == want


@pytest.mark.parametrize('restart', (0, 1, 4))
@pytest.mark.parametrize('ss', (None, 0, 1, 2), ids=lambda v: 'grey' if v is None else 'ss%d' % v)
def test_size_pass_write_pass_and_spec_agree_inside_guards(dev, ss, restart):
    """the C entries one by one over six 64 x 48 tiles: the workspace holds the spec's coefficients in scan order, the size pass
    reports the spec's lengths, the write pass writes the spec's bytes into ranges 16 bytes apart in a 0xA5 buffer and nothing else"""
    from wsi_segmentation_pipeline_amd.engine import _ptr, _stream
    lib = native.load()
    tw, th, (hs, vs) = 64, 48, SS[ss]
    nc = 1 if ss is None else 3
    lv = _level(3 * tw, 2 * th, ss, 60, TF.noise if restart else TF.he_like)
    q = TW.quality_tables(85)
    spec = [E.encode_tile(lv[y:y + th, x:x + tw], q, (hs, vs), restart) for y in (0, th) for x in (0, tw, 2 * tw)]
    n, tile_ws = 6, lib.wsi_jenc_workspace_bytes(tw, th, nc, hs, vs)
    level = torch.from_numpy(lv).to(dev)
    ws = torch.full((n * tile_ws + 256,), 0xC3, dtype=torch.uint8, device=dev)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    native.check(lib.wsi_jenc_transform(_ptr(level), level.stride(0), 2 * th, 3 * tw, 3, 2, 0, n, tw, th, nc, hs, vs, p(q[0]), p(q[1]), _ptr(ws), n * tile_ws,
                                        _stream()), 'transform')
    wsh = ws.cpu().numpy()
    assert (wsh[n * tile_ws:] == 0xC3).all()
    for i, (coefs, _) in enumerate(spec):
        want = E.mcu_order(coefs, (hs, vs)).reshape(-1)
        assert np.array_equal(wsh[i * tile_ws:i * tile_ws + 2 * want.size].view(np.int16), want), i
    sizes_dev = torch.zeros(n, dtype=torch.int32, device=dev)
    native.check(lib.wsi_jenc_entropy_size(_ptr(ws), n * tile_ws, n, tw, th, nc, hs, vs, restart, _ptr(sizes_dev), 0, _stream()), 'size')
    sizes = sizes_dev.cpu().numpy().view(np.uint32)
    assert sizes.tolist() == [len(s) for _, s in spec]
    offsets = np.zeros(n, np.uint64)
    offsets[0] = 32
    for i in range(1, n):
        offsets[i] = (int(offsets[i - 1]) + int(sizes[i - 1]) + 15) // 16 * 16 + 16
    total = int(offsets[-1]) + int(sizes[-1]) + 48
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    ranges = torch.zeros(12 * n + 8, dtype=torch.uint8, device=dev)
    native.check(lib.wsi_jenc_entropy_write(_ptr(ws), n * tile_ws, n, tw, th, nc, hs, vs, restart, p(offsets), p(sizes), _ptr(ranges), _ptr(out), total, 0,
                                            _stream()), 'write')
    host = out.cpu().numpy()
    touched = np.zeros(total, bool)
    for i, (_, scan) in enumerate(spec):
        o = int(offsets[i])
        assert host[o:o + len(scan)].tobytes() == scan, i
        touched[o:o + len(scan)] = True
    assert (host[~touched] == 0xA5).all() and int((~touched).sum()) >= 16 * n + 64


@pytest.mark.parametrize('f', (2, 4))
@pytest.mark.parametrize('h,w', ((2, 2), (17, 33), (7, 4100), (4100, 7)))
def test_box_downsample_equals_numpy(dev, h, w, f):
    for c in (3, 1):
        lv = TF.noise(h, w, h + w + c, c)
        if h // f < 1 or w // f < 1:
            with pytest.raises(ValueError):
                TW.downsample_level(torch.from_numpy(lv).to(dev), f)
            continue
        dh, dw = h // f, w // f
        blocks = lv[:dh * f, :dw * f].astype(np.int64).reshape((dh, f, dw, f) + lv.shape[2:])
        want = ((blocks.sum((1, 3)) + f * f // 2) // (f * f)).astype(np.uint8)
        for offset, extra in ((0, 0), (3, 5)):
            got = TW.downsample_level(_misaligned(dev, lv, offset, extra), f)
            assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), (c, offset)


def _pillow_roundtrip(level, tile, quality, ss):
    """the level as Pillow decodes Pillow-encoded tiles of it"""
    import io
    from PIL import Image
    tw, th = tile
    padded = TF.pad_to_tiles(level, tw, th)
    out = np.zeros(padded.shape[:2] + (3,), np.uint8)
    for y in range(0, padded.shape[0], th):
        for x in range(0, padded.shape[1], tw):
            s = TF.encode(np.ascontiguousarray(padded[y:y + th, x:x + tw]), quality, 0 if ss is None else ss)
            out[y:y + th, x:x + tw] = np.asarray(Image.open(io.BytesIO(s)).convert('RGB'))
    return out[:level.shape[0], :level.shape[1]]


def _box(lv, f):
    dh, dw = lv.shape[0] // f, lv.shape[1] // f
    b = lv[:dh * f, :dw * f].astype(np.int64).reshape((dh, f, dw, f) + lv.shape[2:])
    return ((b.sum((1, 3)) + f * f // 2) // (f * f)).astype(np.uint8)


def test_pyramid_round_trip_on_the_device(dev, tmp_path):
    """write_pyramid of a 300 x 200 level with 64 x 64 tiles and downsample 2, read back by TiffSlide.device_level: every level equals
    Pillow's decode of the same file, and equals Pillow's encode + decode of the box-downsampled level"""
    l0 = TF.he_like(200, 300, 5)
    path = str(tmp_path / 'rt.tif')
    rep = TW.write_pyramid(path, torch.from_numpy(l0).to(dev), tile=(64, 64), quality=75, subsampling=(2, 2), downsample=2, description='round trip', mpp=0.25,
                           workspace_bytes=6 * 64 * 64 * 3)
    levels = [l0, _box(l0, 2), _box(_box(l0, 2), 2), _box(_box(_box(l0, 2), 2), 2)]
    assert [(l['width'], l['height']) for l in rep['levels']] == [(l.shape[1], l.shape[0]) for l in levels] == [(300, 200), (150, 100), (75, 50), (37, 25)]
    assert rep['tiles'] == 20 + 6 + 2 + 1 and rep['bytes'] == os.path.getsize(path) and not rep['big']
    ref = TF.pillow_levels(path, range(4))
    s = TiffSlide(path)
    try:
        assert s.level_dimensions == ((300, 200), (150, 100), (75, 50), (37, 25))
        for k in range(4):
            got = s.device_level(k, dev).cpu().numpy()
            assert int((got != ref[k]).sum()) == 0, k
            assert int((got != _pillow_roundtrip(levels[k], (64, 64), 75, 2)).sum()) == 0, k
            assert s.decode_report[k] == {'ok': s.levels[k].cols * s.levels[k].rows}
    finally:
        s.close()


# --------------------------------------------------------------------------------------------------------------------- the drivers
def _args(monkeypatch, tmp_path):
    import myargs
    for k, v in (('scan_level', 0), ('scan_resize', 1), ('num_classes', 4), ('class_probs', [0., 0., 0., 0.]), ('tile_w', 64), ('tile_h', 64),
                 ('tile_stride_w', 64), ('tile_stride_h', 64), ('val_save_pth', str(tmp_path / 'out')), ('wsi_mask_pth', str(tmp_path / 'nomask'))):
        monkeypatch.setattr(myargs.args, k, v)


@pytest.fixture(scope='module')
def he_slide():
    """the ArraySlide of tests/test_gpu_jpeg.py: a 512 x 512 H&E-like slide with levels at 1, 4 and 16"""
    import stain_oracle as SO
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    l0 = SO.shifted_he(31, 1, 512)[0]
    arr = ArraySlide([l0, np.ascontiguousarray(l0[::4, ::4]), np.ascontiguousarray(l0[::16, ::16])], [1.0, 4.0, 16.0])
    arr.name = 'case.svs'
    return arr


def test_save_slide_writes_the_normalised_slide(dev, he_slide, tmp_path):
    """save_slide of a StainedSlide: every level of the file is, to the byte, what Pillow gets from Pillow-encoded tiles of the
    NORMALISED level - JPEG loss and nothing else; the raw slide would differ"""
    from wsi_segmentation_pipeline_amd import stain
    stained = stain.StainedSlide(he_slide, stain.Normalizer('macenko'))
    path = str(tmp_path / 'norm.tif')
    rep = TW.save_slide(stained, path, device=dev, tile=(128, 128), quality=85, subsampling=(2, 1))
    assert [(l['width'], l['height']) for l in rep['levels']] == [(512, 512), (128, 128), (32, 32)]
    got = TF.pillow_levels(path, range(3))
    for k in range(3):
        norm = stained.device_level(k, dev).cpu().numpy()
        assert int((got[k] != _pillow_roundtrip(norm, (128, 128), 85, 1)).sum()) == 0, k
    assert int((got[0] != _pillow_roundtrip(he_slide.level_array(0), (128, 128), 85, 1)).sum()) > 0
    only = TW.save_slide(he_slide, str(tmp_path / 'l1.tif'), levels=[1], device=dev, tile=(64, 64))
    assert [(l['width'], l['height'], l['tiles']) for l in only['levels']] == [(128, 128, 4)]


def test_predict_wsis_save_tiff_writes_the_scan_level_mask(dev, he_slide, tmp_path, monkeypatch):
    import utils.dataset as ds
    import utils.eval as val
    _args(monkeypatch, tmp_path)

    class Dense(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor([[0.5, 0.25, -0.25], [-1.0, 0.5, 0.5], [1.0, -2.0, 1.0], [-0.5, -1.0, 2.0]]))

        def forward(self, x):
            return torch.stack([sum(x[:, c] * float(self.w[k, c]) for c in range(3)) for k in range(4)], 1)

    model = Dense().to(dev)
    params = {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}
    out = str(tmp_path / 'out')
    res = val.predict_wsis(model, ds.Dataset_wsis({'case.svs': he_slide}, params, bs=16), 1)['case.svs']
    assert os.path.exists(out + '/1/case.svs_64.png') and not os.path.exists(out + '/1/case.svs_64.tif')
    png = open(out + '/1/case.svs_64.png', 'rb').read()
    dataset = ds.Dataset_wsis({'case.svs': he_slide}, params, bs=16)
    mask = dataset.wsis['case.svs']['mask']
    keep = val._map_u8(mask, (32, 32), dev).cpu().numpy() > 0 if mask is not None else np.ones((32, 32), bool)
    res2 = val.predict_wsis(model, dataset, 2, save_tiff=True)['case.svs']
    assert torch.equal(res['classes'], res2['classes']) and open(out + '/2/case.svs_64.png', 'rb').read() == png
    s = TiffSlide(out + '/2/case.svs_64.tif')
    try:
        assert s.level_dimensions[0] == he_slide.level_dimensions[0] == tuple(res2['classes'].shape[::-1]) and s.level_count == 2
        assert s.level_dimensions[1] == (256, 256) and s.levels[0].samples == 3
        # the mask of the file is the scan-level class map in colour (class k > 0 -> channel k - 1) on the foreground mask, the outline in white, up to JPEG loss
        got = s.device_level(0, dev).cpu().numpy()
        up = lambda m: np.kron(m, np.ones((16, 16), bool))      # level 2 -> the scan level by nearest
        cls, edge = res2['classes'].cpu().numpy(), up(res2['outline'].cpu().numpy() > 0)
        want = np.stack([((cls == k + 1) & up(keep)) * 255 for k in range(3)], -1).astype(np.uint8)
        want[edge] = 255
        assert int((got != _pillow_roundtrip(want, (256, 256), 75, 2)).sum()) == 0
    finally:
        s.close()


def test_predict_tumorbed_save_tiff_writes_the_heat_map(dev, he_slide, tmp_path, monkeypatch):
    import resnets_shift
    import utils.dataset as ds
    import utils.eval as val
    from models.models import Classifier
    from wsi_segmentation_pipeline_amd import synthetic as W
    _args(monkeypatch, tmp_path)
    net = resnets_shift.resnet18(False)
    net.load_state_dict(W.make_resnet18_state_dict(11, with_fc=False), strict=False)
    head = Classifier(512, 4)
    head.load_state_dict(W.make_head_state_dict(22, 'classifier'))
    model = val.SlideClassifierModel(net, head).to(dev)
    params = {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}
    out = str(tmp_path / 'out')
    res = val.predict_tumorbed(model, ds.Dataset_wsis({'case.svs': he_slide}, params, bs=16), 1, mode='cls', save_tiff=True)['case.svs']
    assert os.path.exists(out + '/1/case.svs_64_heatmap.png')
    heat = np.asarray(res['heatmap'])
    s = TiffSlide(out + '/1/case.svs_64_heatmap.tif')
    try:
        assert s.levels[0].samples == 1 and s.level_dimensions[0] == heat.shape[::-1] == (32, 32)
        want = _pillow_roundtrip(heat, (256, 256), 75, None)
        assert int((np.asarray(s.read_region((0, 0), 0, (32, 32)))[..., :3] != want).sum()) == 0
    finally:
        s.close()
    val.predict_tumorbed(model, ds.Dataset_wsis({'case.svs': he_slide}, params, bs=16), 2, mode='cls')
    assert os.path.exists(out + '/2/case.svs_64_heatmap.png') and not os.path.exists(out + '/2/case.svs_64_heatmap.tif')
