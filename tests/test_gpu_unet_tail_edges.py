"""The fused decoder tail (csrc/tail.hip) in the configurations that ship, and the dense path's edges, against a float64 spec.

wsi_unet_tail_dispatch splits every image into 1 .. 16 bands (wsi_unet_tail_bands: depends on the batch and the CU count).  The
shipped batch of 512 tiles of 256 x 256 runs ONE band of 128 ring steps per image; small batches run 16.  Each band count is run
here at the smallest batch that reaches it, in the specialised form (the default), the first form (wsi_conv_set_mode +4194304) and
the three launches (+2097152), on every image against the three launches and on sampled images (first, second, middle, last two)
against oracle/unet_oracle.py evaluated in float64.  Also: 64- and 128-wide maps and a non-square tile; the last batch that fits the
tail's 32-bit buffer offsets (1008 tiles of 256 x 256: x4 above 2 GiB) and the first that does not (1009: the three launches);
no tiles at all, in forward_tiles and in seg-mode predict_tumorbed over two ranks."""
import ctypes as C
import os
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import resnet_oracle as R
from oracle import unet_oracle as U
from oracle import weights as W
from wsi_segmentation_pipeline_amd import native

pytestmark = pytest.mark.gpu

FORM1, THREE_LAUNCHES = native.ConvMode.UNET_TAIL_FORM1, native.ConvMode.UNET_NO_TAIL      # wsi_conv_set_mode A/B switches (include/wsi_hip.h)
SPEC_TOL = 1e-3                                            # absolute, logits scaled to |logit| 16 (the contract of the dense path)
_SPEC = {}                                                 # (th, tw, x, y) -> float64 spec logits of that tile


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from wsi_segmentation_pipeline_amd import native
    return native.load()


@pytest.fixture(scope='module')
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _positions(n, th, tw):
    """Tile corners (x, y): a raster of 8-pixel steps, 128 per row - every tile a different window of the level."""
    i = np.arange(n)
    return np.stack((8 * (i % 128), 8 * (i // 128)), 1).astype(np.int32)


class _Shape:
    """One tile shape: a random u8 level holding 1024 distinct tiles, the seeded decoder with its final conv scaled so the float64
    spec of tile 0 peaks at |logit| 16 (tests/test_gpu_unet.py _scaled_to_logit), and its engine."""

    def __init__(self, dev, th, tw, max_batch=None, sd=None):
        from wsi_segmentation_pipeline_amd.unet import UNetEngine
        self.th, self.tw = th, tw
        g = torch.Generator(device=dev).manual_seed(th * 1000 + tw)
        self.level = torch.randint(0, 256, (8 * 8 + th + 8, 8 * 127 + tw + 8, 3), dtype=torch.uint8, device=dev, generator=g)
        self.level_np = self.level.cpu().numpy()
        if sd is None:
            sd = W.make_unet_state_dict(7, 4)
            with torch.no_grad():
                s = 16.0 / float(U.unet_forward(_f64(sd), self._x(0, 0).double()).abs().max())
            sd = dict(sd)
            for key in ('decoder.final_conv.weight', 'decoder.final_conv.bias'):
                sd[key] = sd[key] * s
        self.sd, self.sd64 = sd, _f64(sd)
        self.eng = UNetEngine(sd, dev, planes=2, max_batch=max_batch)
        assert self.eng.dw.tail_w

    def _x(self, x, y):
        u8 = self.level_np[y:y + self.th, x:x + self.tw][None].transpose(0, 3, 1, 2)
        return R.normalize_u8(np.ascontiguousarray(u8))

    def spec(self, x, y):
        key = (self.th, self.tw, int(x), int(y))
        if key not in _SPEC:
            with torch.no_grad():
                _SPEC[key] = U.unet_forward(self.sd64, self._x(int(x), int(y)).double())[0]
        return _SPEC[key]


def _f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


_SHAPES = {}


def _shape(dev, th, tw):
    if (th, tw) not in _SHAPES:
        _SHAPES[(th, tw)] = _Shape(dev, th, tw)
    return _SHAPES[(th, tw)]


def _timeouts(lib, reset=True):
    torch.cuda.synchronize()
    out = C.c_ulonglong(0)
    assert lib.wsi_unet_tail_timeouts(C.byref(out), 1 if reset else 0) == 0
    return int(out.value)


def _smallest_n(lib, h, cus, bands, limit):
    ns = [n for n in range(1, limit + 1) if lib.wsi_unet_tail_bands(n, h, cus) == bands]
    assert ns, 'no batch <= %d of %d-row maps runs %d bands on %d CUs' % (limit, h, bands, cus)
    return ns[0]


def _check_case(lib, sh, n, bands):
    """n tiles of `sh` in one U-Net call whose tail runs `bands` bands per image: the fused forms against the three launches on every
    image, all three against the float64 spec on sampled images, run-to-run bits, no hand-over timeout."""
    from wsi_segmentation_pipeline_amd.unet import equal_batches
    th, tw, eng = sh.th, sh.tw, sh.eng
    assert equal_batches(n, eng._batch(th, tw)) == [(0, n)]          # one call: the tail sees the whole batch
    xy_np = _positions(n, th, tw)
    xy = torch.from_numpy(xy_np)
    _timeouts(lib)
    fused = eng.forward_tiles(sh.level, xy, th, tw)
    with native.conv_mode(FORM1):
        form1 = eng.forward_tiles(sh.level, xy, th, tw)
    with native.conv_mode(THREE_LAUNCHES):
        plain = eng.forward_tiles(sh.level, xy, th, tw)
    again = eng.forward_tiles(sh.level, xy, th, tw)
    assert tuple(fused.shape) == (n, 4, th, tw)
    assert torch.equal(fused, again)                                 # the LDS counter hand-over: same bits every run
    assert torch.isfinite(fused).all() and torch.isfinite(form1).all()
    scale = float(plain.abs().max())
    bound = 2e-5 * max(scale, 1.0)
    rows = th // bands                                               # output rows per band
    for name, got in (('specialised', fused), ('first form', form1)):
        dimg = (got - plain).abs().amax((1, 2, 3))
        worst = int(dimg.argmax())
        d = float(dimg[worst])
        yrow = int((got[worst] - plain[worst]).abs().amax((0, 2)).argmax())
        print('tail %dx%d n=%d bands=%d %s vs three launches: max |dlogit| %.3g at image %d band %d (row %d), max |logit| %.3g'
              % (th, tw, n, bands, name, d, worst, yrow // rows, yrow, scale))
        assert 0 < d <= bound, (name, n, bands, d, worst, yrow // rows)
    d12 = float((fused - form1).abs().max())
    assert d12 <= 2e-6 * max(scale, 1.0), d12                       # same weights, same products; the head sums in another order
    errs = []
    for i in sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n))):
        ref = sh.spec(*xy_np[i])
        e = [float((t[i].cpu().double() - ref).abs().max()) for t in (fused, form1, plain)]
        errs.append((i, e))
        assert max(e) <= SPEC_TOL, (i, e)
    print('tail %dx%d n=%d bands=%d vs float64 spec (image: fused, first form, three launches): %s'
          % (th, tw, n, bands, ', '.join('%d: %.2e %.2e %.2e' % ((i,) + tuple(e)) for i, e in errs)))
    assert _timeouts(lib) == 0


@pytest.mark.parametrize('bands', [16, 8, 4, 2, 1, 'shipped'])
def test_every_band_count_of_256_tiles(dev, lib, cus, bands):
    """256 x 256 tiles (h = 128 low-resolution rows): the smallest batch <= 512 running each band count, and the shipped batch of 512
    (UNetEngine.TUNED_BATCH_256), which runs one band per image on 256 CUs."""
    from wsi_segmentation_pipeline_amd.unet import UNetEngine
    sh = _shape(dev, 256, 256)
    if bands == 'shipped':
        n = UNetEngine.TUNED_BATCH_256
        bands = lib.wsi_unet_tail_bands(n, 128, cus)
    else:
        n = _smallest_n(lib, 128, cus, bands, 512)
    print('256x256, %d CUs: %d bands at n = %d' % (cus, bands, n))
    _check_case(lib, sh, n, bands)


@pytest.mark.parametrize('tile', [(64, 64), (128, 128), (256, 128)])
@pytest.mark.parametrize('which', ['one band', 'most bands'])
def test_other_widths_at_one_and_most_bands(dev, lib, cus, tile, which):
    """Maps 32 and 64 low-resolution columns wide (the specialised form with one and two MFMA tiles per wave) and a non-square tile:
    the smallest batch that runs one band per image and a single image (the largest band count of the map)."""
    th, tw = tile
    h = th // 2
    most = max(lib.wsi_unet_tail_bands(1, h, cus), 1)
    if which == 'one band':
        bands, n = 1, _smallest_n(lib, h, cus, 1, 1024)
    else:
        bands, n = most, 1
        assert most == max(b for b in (1, 2, 4, 8, 16) if h % b == 0 and h // b >= 8)
    sh = _shape(dev, th, tw)
    _check_case(lib, sh, n, bands)


def test_tail_at_its_32_bit_limit(dev, lib):
    """1008 tiles of 256 x 256 are the last batch whose x4 fits the tail's 32-bit buffer offsets (its last images sit above 2 GiB):
    fused, and right on the last images.  1009 in one call: the tail steps aside, the three launches run (bit-identical)."""
    from wsi_segmentation_pipeline_amd.unet import equal_batches
    for sh in _SHAPES.values():                                      # this test needs ~78 GB of workspace
        sh.eng.release_workspaces()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < 110e9:
        reason = 'the 32-bit limit test needs 110 GB of free device memory, %.1f GB free' % (free / 1e9)
        print(reason)
        pytest.skip(reason)
    base = _shape(dev, 256, 256)
    sh = _Shape(dev, 256, 256, max_batch=1008, sd=base.sd)
    sh.level, sh.level_np = base.level, base.level_np                # the same tiles, hence the same spec cache
    try:
        for n, tail in ((1009, False), (1008, True)):
            assert equal_batches(n, 1008) == [(0, n)]
            xy_np = _positions(n, 256, 256)
            xy = torch.from_numpy(xy_np)
            _timeouts(lib)
            fused = sh.eng.forward_tiles(sh.level, xy, 256, 256)
            with native.conv_mode(THREE_LAUNCHES):
                plain = sh.eng.forward_tiles(sh.level, xy, 256, 256)
            d = float((fused - plain).abs().max())
            scale = float(plain.abs().max())
            errs = []
            for i in (0, n - 3, n - 2, n - 1):
                errs.append(float((fused[i].cpu().double() - sh.spec(*xy_np[i])).abs().max()))
            print('n=%d (tail %s): max |fused - three launches| %.3g at max |logit| %.3g; vs float64 spec, images 0, n-3, n-2, n-1: %s'
                  % (n, 'on' if tail else 'off', d, scale, ' '.join('%.2e' % e for e in errs)))
            if tail:
                assert 0 < d <= 2e-5 * max(scale, 1.0), d
            else:
                assert torch.equal(fused, plain)
            assert max(errs) <= SPEC_TOL, errs
            assert _timeouts(lib) == 0
            del fused, plain
    finally:
        sh.eng.release_workspaces()
        del sh
        torch.cuda.empty_cache()


def test_forward_tiles_of_no_tiles(dev):
    sh = _shape(dev, 256, 256)
    out = sh.eng.forward_tiles(sh.level, torch.zeros((0, 2), dtype=torch.int32), 256, 256)
    assert tuple(out.shape) == (0, 4, 256, 256) and out.dtype == torch.float32 and out.device.type == 'cuda'


# ------------------------------------------------------------------------------ seg-mode predict_tumorbed with empty ranks
def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _seg_few(rank, world, ntiles, tmp):
    """predict_tumorbed(mode='seg') of UNetSeg over `ntiles` foreground tiles of a small slide (tests/test_gpu_unet.py's seg
    setup, the tile list cut down): with one tile rank 1 of two owns nothing, with none neither rank does."""
    import myargs
    import utils.dataset as ds
    import utils.eval as val
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    from wsi_segmentation_pipeline_amd.unet import UNetSeg
    a = myargs.args
    a.scan_level, a.scan_resize, a.num_classes, a.class_probs = 2, 1, 4, [0., 0., 0., 0.]
    a.tile_w = a.tile_h = 64
    a.tile_stride_w = a.tile_stride_h = 48
    a.val_save_pth, a.wsi_mask_pth = os.path.join(tmp, 'out'), os.path.join(tmp, 'nomask')
    rng = np.random.default_rng(13)
    l2 = np.clip(np.kron(rng.integers(60, 250, (7, 9, 3)), np.ones((32, 32, 1))) + rng.integers(-25, 25, (224, 288, 3)), 0, 255).astype(np.uint8)
    slide = ArraySlide([l2[:8, :8], l2[:8, :8], l2], [1.0, 4.0, 16.0])   # only level 2 is read
    slide.level_dimensions = ((288 * 16, 224 * 16), (288 * 4, 224 * 4), (288, 224))
    slide.name = 'seg.svs'
    model = UNetSeg(4)
    model.load_state_dict(W.make_unet_state_dict(7, 4))
    model = model.cuda().eval()
    params = {'ph': 64, 'pw': 64, 'sh': 48, 'sw': 48}
    dataset = ds.Dataset_wsis({'seg.svs': slide}, params, bs=5)
    entry = dataset.wsis['seg.svs']
    d = entry['iterator'].dataset
    assert len(d) >= 12
    d.tile_xy, d.datalist = np.ascontiguousarray(d.tile_xy[5:5 + ntiles]), d.datalist[5:5 + ntiles]
    entry['iterator'] = ds.DeviceTileIterator(d, 5)
    res = val.predict_tumorbed(model, dataset, 1, mode='seg', rank=rank, world=world, save=False)['seg.svs']
    torch.cuda.synchronize()
    return {'heatmap': res['heatmap'], 'classes': res['classes']}


def _seg_worker(rank, world, port, q, ntiles, tmp):
    try:
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        out = _seg_few(rank, world, ntiles, tmp)
    except BaseException:
        q.put((rank, ('error', traceback.format_exc())))
        return
    q.put((rank, ('ok', out)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('ntiles', [1, 0])
def test_seg_two_ranks_with_fewer_tiles_than_ranks(ntiles, tmp_path):
    """Seg mode over two ranks with one tile (rank 1's share is empty) and with no foreground tile: both ranks return the single-rank
    heat map and class map byte for byte.  A rank that raises reports it through the queue and the children are terminated, so a
    failing rank ends the test instead of leaving the other one waiting in the band gather."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_seg_worker, args=(r, 2, port, q, ntiles, str(tmp_path))) for r in range(2)]
    got = {}
    try:
        for p in procs:
            p.start()
        for _ in procs:
            rank, (status, payload) = q.get(timeout=300)
            assert status == 'ok', 'rank %d raised:\n%s' % (rank, payload)
            got[rank] = payload
        for p in procs:
            p.join(120)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(10)
    ref = _seg_few(0, 1, ntiles, str(tmp_path))
    assert ref['heatmap'].shape == ref['classes'].shape == (224, 288)
    for rank in (0, 1):
        for k in ('heatmap', 'classes'):
            assert got[rank][k].dtype == ref[k].dtype and np.array_equal(got[rank][k], ref[k]), (rank, k)
