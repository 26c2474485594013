"""The ResNet trunk at the batch sizes it ships with and at the 2 / 4 GiB edges of its tensors, against the CPU oracle.

cfg3 runs 24 648 tiles of 256 x 256 as four batches of 6 162 on two streams: there the layer-1 tensors, their 96-byte line planes
(mx), the phase-split hand-over to layer 2 and the stem's slide reads all pass 2 GiB and most pass 4 GiB.  The kernels address them
with a 64-bit base per workgroup and 32-bit offsets inside it, so a lost cast would only corrupt images past the crossing.  Tiles on
both sides of every crossing, the first and last tile of each batch and the tiles whose stem reads straddle or lie beyond 2^31 and 2^32
slide bytes are checked against oracle/resnet_oracle.py; every tile against a run in batches of 512.

Patches wider than 256 px enter layer 2 through wsi_conv3x3s2_ds_fused, whose phase-slab kernel reads less than 4 GiB per launch
(wsi_s2_slab_images): 1 008 patches of 512 x 512 in modes 2 and 3.  Larger batches run as image sub-ranges.  The 512-px batches of
1 008, 1 009 and the engine's tuned 1 550, and 288 / 384-px batches at their own limit and one past it, must equal a run in batches of
64 bit for bit; the entry itself is checked at 1 008 / 1 009 images against a float64 reference, and predict_tumorbed(mode='cls') at
the reference's default tile of 512 x 512 over more than 1 008 tiles.

Every crossing index is derived from the library's PF layout (wsi_pf_bytes, wsi_pf_pixel_index, wsi_trunk_workspace_bytes)."""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import resnet_oracle as R
from oracle import weights as W

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3
TOL_PARITY, TOL_MX = 2e-5, 1e-4            # tests/test_gpu_kernels.py: single layer, relative to the tensor's max magnitude
EDGES = (1 << 31, 1 << 32)
SLAB_LIMIT = 0xffffffff                    # the phase-slab kernel's PF input must stay below this many bytes (csrc/conv.hip)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    yield torch.device('cuda:0')
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def lib():
    from wsi_segmentation_pipeline_amd import native
    return native.load()


@pytest.fixture(scope='module')
def weights():
    sd = W.make_resnet18_state_dict(11, with_fc=False)
    cls = W.make_head_state_dict(22, 'classifier')
    return sd, cls, (cls['fc.0.weight'], cls['fc.0.bias'])


@pytest.fixture
def batches(monkeypatch):
    """Records (engine id, images) of every trunk call."""
    from wsi_segmentation_pipeline_amd.engine import TrunkEngine
    seen = []
    orig = TrunkEngine._run

    def run(self, n, *a, **k):
        seen.append((id(self), int(n)))
        return orig(self, n, *a, **k)
    monkeypatch.setattr(TrunkEngine, '_run', run)
    return seen


def _free(*engines):
    for e in engines:
        e.release_workspaces()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _free_bytes(dev):
    free = torch.cuda.mem_get_info(dev)[0]
    return free + max(0, torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev))


def _pf_pixels(lib, n, h, w):
    """pf_alloc_pixels (csrc/common.h): the pixel count of an n-image PF tensor of h x w maps."""
    return lib.wsi_pf_bytes(n, h, w, 64, 1) // 128


def _slab_limit(lib, h, w, planes):
    """Largest batch of h x w patches whose layer-2 entry input (h/4 x w/4 maps, 64 channels) is under the slab kernel's 4 GiB."""
    n = 1
    while lib.wsi_pf_bytes(n + 1, h // 4, w // 4, 64, planes) < SLAB_LIMIT:
        n += 1
    return n


def _image_at(lib, byte, pixbytes, h, w):
    """Image of a PF tensor of h x w maps (pixbytes per pixel) whose block (its pixels and closing pads) holds `byte`."""
    g = lib.wsi_pf_pixel_index(0, 0, 0, h, w)
    s = lib.wsi_pf_pixel_index(1, 0, 0, h, w) - g
    return max(0, (byte // pixbytes - g) // s)


def _crossings(lib, n, cap, h, w, planes):
    """{buffer @ edge: images} of an n-image batch (workspace planned for cap) next to the 2 and 4 GiB byte positions of the trunk's
    large buffers.  Layout (csrc/trunk.hip trunk_plan / trunk_run): the layer-1 tensors are ordinary PF, or, in mx with the phase-split
    hand-over, two planes of 96-byte lines plane96 = pf_alloc_pixels(cap) * 96 apart; the hand-over to layer 2 (modes 2 and 3, layer-2
    maps at most 33 wide) is four phase images of (cap, h/8, w/8) maps; the layer-2 tensors are ordinary PF."""
    bpc = 2 if planes == 1 else 4
    h1, w1, h2, w2 = h // 4, w // 4, h // 8, w // 8
    split0 = planes >= 2 and w2 <= 33
    segs = []                                                  # (name, base byte, bytes per pixel, map h, map w)
    if planes == 3 and split0:
        p96 = _pf_pixels(lib, cap, h1, w1) * 96
        segs += [('layer1 lines plane %d' % j, j * p96, 96, h1, w1) for j in range(2)]
    else:
        segs.append(('layer1', 0, 64 * bpc, h1, w1))
    if split0:
        ps = _pf_pixels(lib, cap, h2, w2) * 64 * bpc
        segs += [('hand-over phase %d' % p, p * ps, 64 * bpc, h2, w2) for p in range(4)]
    segs.append(('layer2', 0, 128 * bpc, h2, w2))
    out = {}
    for name, base, pb, hh, ww in segs:
        end = base + _pf_pixels(lib, cap, hh, ww) * pb
        for b in EDGES:
            if base <= b < end:
                k = _image_at(lib, b - base, pb, hh, ww)
                if k < n:
                    out['%s @ 2^%d' % (name, b.bit_length() - 1)] = [i for i in (k - 1, k, k + 1) if 0 <= i < n]
    return out


def _oracle_err(sd, cls, level_dev, xy, logits, idx, ph, pw):
    """(tiles, max |logit - oracle| of each) for the tiles idx of the corner list xy, read from the device level."""
    idx = np.asarray(sorted(set(int(i) for i in idx)))
    u8 = torch.stack([level_dev[y:y + ph, x:x + pw].cpu() for x, y in xy[idx].tolist()]).permute(0, 3, 1, 2).contiguous().numpy()
    with torch.no_grad():
        ref = R.tile_logits(sd, cls, u8)
    got = logits[torch.from_numpy(idx).to(logits.device)].cpu()
    return idx, (got - ref).abs().amax(1)


def _first_diff(a, b):
    d = (a != b).any(1).nonzero()
    return int(d[0]) if len(d) else None


# ------------------------------------------------------------------------------ a. cfg3 at the shipped batch
@pytest.mark.parametrize('mode', ['mx', 'parity'])
def test_cfg3_shipped_batches(dev, lib, weights, batches, mode):
    """cfg3's 24 648 tiles through a default engine (auto cap, two streams): four batches of 6 162.  Every logit equals the same
    weights run in batches of 512 on one stream; the oracle checks the first and last tile of each batch, the tiles next to the 2 / 4 GiB
    positions of the layer-1 buffers, the 96-byte line planes, the hand-over to layer 2 and the layer-2 buffers (spread over the four
    batches), and the tiles whose stem reads straddle or lie beyond 2^31 and 2^32 bytes of the slide, the bottom-right tile included."""
    from wsi_segmentation_pipeline_amd import engine as E
    from wsi_segmentation_pipeline_amd import slide as S
    sd, cls, head = weights
    planes = {'mx': E.MX, 'parity': E.PARITY}[mode]
    size, tile = 40000, 256
    tiles = S.tile_grid(size, size, tile, tile, tile, tile)
    assert len(tiles) == 24648
    ship = E.batch_sizes(len(tiles), E.TrunkEngine.TUNED_BATCH_256, tile, tile)
    assert ship == [6162] * 4
    g = torch.Generator(device=dev).manual_seed(3)
    level0 = torch.randint(0, 256, (size, size, 3), dtype=torch.uint8, device=dev, generator=g)      # 4.8 GB
    xy = torch.from_numpy(tiles).to(dev)
    eng = E.TrunkEngine(sd, dev, planes=planes, head=head)
    if eng._auto_cap(tile, tile) < max(ship):
        need = 2 * lib.wsi_trunk_workspace_bytes(max(ship), tile, tile, planes)
        del level0
        _free(eng)
        pytest.skip('free HBM %.1f GB cannot hold two workspaces of %d tiles (%.1f GB, with the engine\'s 60 %% margin %.1f GB)'
                    % (_free_bytes(dev) / 1e9, max(ship), need / 1e9, need / 0.6 / 1e9))
    logits = eng.forward_tiles(level0, xy, tile, tile, logits=True)[1]
    ran = [n for e, n in batches if e == id(eng)]
    print('%s: trunk batches %s, workspace %.1f GB per slot' % (mode, ran, lib.wsi_trunk_workspace_bytes(max(ship), tile, tile, planes) / 1e9))
    assert ran == ship
    _free(eng)
    ref_eng = E.TrunkEngine(sd, dev, planes=planes, head=head, max_batch=512, streams=1)
    ref = ref_eng.forward_tiles(level0, xy, tile, tile, logits=True)[1]
    _free(ref_eng)

    starts = np.cumsum([0] + ship[:-1])
    idx = [i for s, m in zip(starts, ship) for i in (s, s + m - 1)]
    cross = _crossings(lib, max(ship), max(ship), tile, tile, planes)
    assert len(cross) >= 3, cross
    for j, (name, ks) in enumerate(sorted(cross.items())):
        idx += [starts[j % len(ship)] + k for k in ks]
    pitch = level0.stride(0)
    lo = tiles[:, 1].astype(np.int64) * pitch + tiles[:, 0].astype(np.int64) * 3
    hi = (tiles[:, 1].astype(np.int64) + tile - 1) * pitch + (tiles[:, 0].astype(np.int64) + tile) * 3 - 1
    for b in EDGES:
        straddle = np.nonzero((lo < b) & (hi >= b))[0]
        beyond = np.nonzero(lo >= b)[0]
        assert len(straddle) and len(beyond)
        row, col = b // pitch, (b % pitch) // 3
        at = [i for i in straddle if tiles[i, 1] <= row < tiles[i, 1] + tile and tiles[i, 0] <= col < tiles[i, 0] + tile]
        assert at, b
        idx += at[:1] + [int(beyond[np.argmin(lo[beyond])])]
    idx.append(int(np.argmax(hi)))                                # the bottom-right tile: the slide's last bytes
    checked, err = _oracle_err(sd, cls, level0, tiles, logits, idx, tile, tile)
    diff = _first_diff(logits, ref)
    print('%s: %d oracle tiles, max err %.2e; crossings %s' % (mode, len(checked), float(err.max()), cross))
    del level0, xy
    gc.collect()
    torch.cuda.empty_cache()
    bad = []
    if diff is not None:
        bad.append('tile %d differs from the 512-tile batches (%s vs %s)' % (diff, logits[diff].tolist(), ref[diff].tolist()))
    if float(err.max()) > LOGIT_TOL:
        bad.append('oracle error %.2e > %.0e at tiles %s' % (float(err.max()), LOGIT_TOL, checked[(err > LOGIT_TOL).numpy()].tolist()))
    assert not bad, '; '.join(bad)


# ------------------------------------------------------------------------------ b. patches wider than 256 px at the entry's edge
_B_CASES = [(512, 'mx'), (512, 'parity'), (512, 'speed'), (288, 'mx'), (288, 'parity'), (384, 'mx'), (384, 'parity')]


@pytest.mark.parametrize('patch,mode', _B_CASES)
def test_wide_patches_at_the_stride2_entry_limit(dev, lib, weights, batches, patch, mode):
    """Batches of patch x patch tiles at the layer-2 entry's 4 GiB limit (modes 2 and 3), one past it and, at 512 px, the engine's
    tuned batch (1 550): no error, every logit equal to the same tiles run in batches of 64; mx / parity also against the oracle on the
    first and last tile and on the tiles next to each 2 / 4 GiB crossing.  Speed mode is outside the logit contract: equality only."""
    from wsi_segmentation_pipeline_amd import engine as E
    sd, cls, head = weights
    planes = {'mx': E.MX, 'parity': E.PARITY, 'speed': E.SPEED}[mode]
    lim = _slab_limit(lib, patch, patch, E.PARITY)
    sizes = [lim, lim + 1]
    if patch == 512:
        sizes.append(max(1, E.TrunkEngine.TUNED_BATCH_256 * 65536 // (patch * patch)))
    total = max(sizes)
    rng = np.random.default_rng(patch + planes)
    side = 8192
    g = torch.Generator(device=dev).manual_seed(patch + planes)
    level0 = torch.randint(0, 256, (side, side, 3), dtype=torch.uint8, device=dev, generator=g)
    xy_np = rng.integers(0, side - patch + 1, (total, 2)).astype(np.int32)
    xy = torch.from_numpy(xy_np).to(dev)
    ref_eng = E.TrunkEngine(sd, dev, planes=planes, head=head, max_batch=64, streams=1)
    ref = ref_eng.forward_tiles(level0, xy, patch, patch, logits=True)[1]
    _free(ref_eng)
    report = []
    for n in sizes:
        eng = E.TrunkEngine(sd, dev, planes=planes, head=head, max_batch=n, streams=1)
        got = eng.forward_tiles(level0, xy[:n], patch, patch, logits=True)[1]
        assert [m for e, m in batches if e == id(eng)] == [n]
        _free(eng)
        diff = _first_diff(got, ref[:n])
        assert diff is None, '%s %d px, batch %d: tile %d differs from batches of 64' % (mode, patch, n, diff)
        if planes != E.SPEED:
            cross = _crossings(lib, n, n, patch, patch, planes)
            idx = [0, n - 1] + [k for ks in cross.values() for k in ks]
            checked, err = _oracle_err(sd, cls, level0, xy_np, got, idx, patch, patch)
            report.append('batch %d: %d oracle tiles, max err %.2e (%s)' % (n, len(checked), float(err.max()), sorted(cross)))
            assert float(err.max()) <= LOGIT_TOL, (n, checked.tolist(), err.tolist())
    print('%s %d px, limit %d: %s' % (mode, patch, lim, '; '.join(report) or 'equal'))
    del level0, xy
    gc.collect()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------ c. the stride-2 entry through the C ABI
@pytest.mark.parametrize('planes', [2, 3])
def test_stride2_entry_at_4gib(dev, lib, planes):
    """wsi_conv3x3s2_ds_fused, 64 -> 128 channels on 128 x 128 maps (the layer-2 entry of 512-px patches) at the last batch whose PF
    input is under 4 GiB and one past it: the 3x3 conv (+ReLU) and the 1x1 downsample of images 0, n-2 and n-1 against float64 on the
    CPU, and every pad position of both outputs still zero."""
    import ctypes as C
    from wsi_segmentation_pipeline_amd import engine as E, native
    h = w = 128
    cin, cout = 64, 128
    tol = TOL_MX if planes == 3 else TOL_PARITY
    lim = _slab_limit(lib, 4 * h, 4 * w, planes)
    gc_ = torch.Generator().manual_seed(9)
    w3 = torch.randn(cout, cin, 3, 3, generator=gc_) * (2.0 / (cin * 9)) ** 0.5
    w1 = torch.randn(cout, cin, 1, 1, generator=gc_) * (2.0 / cin) ** 0.5
    bn3 = [torch.rand(cout, generator=gc_) + 0.5, torch.randn(cout, generator=gc_) * 0.1, torch.randn(cout, generator=gc_) * 0.1,
           torch.rand(cout, generator=gc_) + 0.5]
    bn1 = [torch.rand(cout, generator=gc_) + 0.5, torch.randn(cout, generator=gc_) * 0.1, torch.randn(cout, generator=gc_) * 0.1,
           torch.rand(cout, generator=gc_) + 0.5]
    wp3, b3 = E.prepack_conv(w3, bn3, planes, dev)
    wp1, b1 = E.prepack_conv(w1, bn1, planes, dev)
    for n in (lim, lim + 1):
        assert (lib.wsi_pf_bytes(n, h, w, cin, planes) < SLAB_LIMIT) == (n == lim)
        g = torch.Generator(device=dev).manual_seed(n)
        x = torch.rand(n, cin, h, w, device=dev, generator=g)
        pick = [0, n - 2, n - 1]
        xs = x[pick].cpu().double()
        xpf = E.pf_pack(x, planes)
        del x
        o3, o1 = E.pf_zeros(n, cout, h // 2, w // 2, planes, dev), E.pf_zeros(n, cout, h // 2, w // 2, planes, dev)
        rc = lib.wsi_conv3x3s2_ds_fused(xpf.data_ptr(), o3.data_ptr(), o1.data_ptr(), wp3.data_ptr(), b3.data_ptr(), wp1.data_ptr(),
                                        b1.data_ptr(), n, h, w, cin, cout, planes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        native.check(rc, 'wsi_conv3x3s2_ds_fused, planes %d, n %d' % (planes, n))
        del xpf
        ref3 = F.relu(F.batch_norm(F.conv2d(xs, w3.double(), None, 2, 1), bn3[2].double(), bn3[3].double(), bn3[0].double(),
                                   bn3[1].double(), False, 0.0, 1e-5))
        ref1 = F.batch_norm(F.conv2d(xs, w1.double(), None, 2, 0), bn1[2].double(), bn1[3].double(), bn1[0].double(), bn1[1].double(),
                            False, 0.0, 1e-5)
        for name, o, ref in (('conv', o3, ref3), ('downsample', o1, ref1)):
            got = E.pf_unpack(o, n, cout, h // 2, w // 2, planes)
            ones = torch.ones_like(got) if planes == 3 else torch.full_like(got, 1.0 + 2.0 ** -12)
            sub = got[pick].cpu().double()
            del got
            err = [float((sub[i] - ref[i]).abs().max() / ref[i].abs().max()) for i in range(len(pick))]
            print('planes %d, n %d, %s: images %s rel err %s' % (planes, n, name, pick, ['%.1e' % e for e in err]))
            assert max(err) <= tol, (planes, n, name, err)
            # pad positions stay zero (tests/test_gpu_kernels.py _conv_case)
            if planes == 3:
                real = E.pf_pack(ones, 3).view(-1, 128)[:, :64].ne(0).any(1)
                assert not bool(o.view(-1, 128)[~real].ne(0).any()), '%s: a pad position was written' % name
            else:
                real = E.pf_pack(ones, planes).view(torch.int16) != 0
                assert not bool((o.view(torch.int16)[~real] != 0).any()), '%s: a pad position was written' % name
            del ones, real
        del o3, o1
        gc.collect()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------ d. predict_tumorbed at the reference's default tile
@pytest.mark.parametrize('precision', ['mx', 'auto'])
def test_predict_tumorbed_cls_default_tile(dev, lib, weights, batches, tmp_path, precision):
    """predict_tumorbed(mode='cls') with myargs' tile of 512 x 512 and stride 128 on a 4 608^2 level-0 scan (1 088 tiles, one trunk
    call): heat map, class map and logits equal a second run whose engines (both inner engines of precision 'auto') take 64 tiles per
    call."""
    import myargs
    import resnets_shift
    import utils.dataset as ds
    import utils.eval as val
    from models.models import Classifier
    from wsi_segmentation_pipeline_amd import slide as S
    from wsi_segmentation_pipeline_amd.engine import TrunkEngine
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    sd, cls, _ = weights
    a = myargs.args
    keys = ('tile_w', 'tile_h', 'tile_stride_w', 'tile_stride_h', 'scan_level', 'scan_resize', 'num_classes', 'class_probs',
            'val_save_pth', 'wsi_mask_pth')
    saved = {k: getattr(a, k) for k in keys}
    for k in keys[:4]:                                         # the reference's defaults (other tests leave their own tiles behind)
        setattr(a, k, myargs.parser.get_default(k))
    assert (a.tile_w, a.tile_h, a.tile_stride_w, a.tile_stride_h) == (512, 512, 128, 128)
    a.scan_level, a.scan_resize, a.num_classes, a.class_probs = 0, 1, 4, [0., 0., 0., 0.]
    a.val_save_pth, a.wsi_mask_pth = str(tmp_path / 'out'), str(tmp_path / 'nomask')
    lim = _slab_limit(lib, a.tile_h, a.tile_w, 2)
    rng = np.random.default_rng(21)
    size = 4608
    l0 = np.clip(np.kron(rng.integers(60, 250, (36, 36, 3)), np.ones((128, 128, 1))) + rng.integers(-40, 40, (size, size, 3)),
                 0, 255).astype(np.uint8)
    slide = ArraySlide([l0, l0[::4, ::4], l0[::16, ::16]], [1.0, 4.0, 16.0])
    slide.name = 'default_tile.svs'
    grid = S.tile_grid(size, size, a.tile_h, a.tile_w, a.tile_stride_h, a.tile_stride_w)
    assert len(grid) > lim
    net = resnets_shift.resnet18(False)
    net.load_state_dict(W.make_resnet18_state_dict(11))
    net.precision = precision
    hd = Classifier(512, 4)
    hd.load_state_dict(cls)
    model = val.SlideClassifierModel(net, hd).cuda()
    params = {'ph': a.tile_h, 'pw': a.tile_w, 'sh': a.tile_stride_h, 'sw': a.tile_stride_w}

    def run():
        dataset = ds.Dataset_wsis({slide.name: slide}, params, bs=16)
        d = dataset.wsis[slide.name]['iterator'].dataset
        d.tile_xy, d.datalist = np.ascontiguousarray(grid), [tuple(int(v) for v in t) for t in grid]   # every tile, whatever the mask
        res = val.predict_tumorbed(model, dataset, 1, mode='cls', save=False)[slide.name]
        torch.cuda.synchronize()
        return res

    try:
        first = run()
        eng = net._engine
        inner = [e for e in (getattr(eng, '_par', None), getattr(eng, '_mx', None)) if e is not None] or [eng]
        big = max(n for e, n in batches if e in {id(i) for i in inner})
        if big <= lim:
            per = lib.wsi_trunk_workspace_bytes(len(grid), a.tile_h, a.tile_w, 3)
            pytest.skip('free HBM %.1f GB gave trunk calls of %d tiles only (one call of %d needs %.1f GB per slot)'
                        % (_free_bytes(dev) / 1e9, big, len(grid), per / 1e9))
        for e in inner:
            e.release_workspaces()
            e.max_batch = 64
        del batches[:]
        second = run()
        assert max(n for _, n in batches) == 64
        print('%s: %d tiles, largest trunk call %d, precision %s' % (precision, len(grid), big, first.get('precision')))
        assert first['logits'].shape == (len(grid), 4)
        assert torch.equal(first['logits'], second['logits'])
        for k in ('heatmap', 'classes'):
            assert first[k].dtype == second[k].dtype and np.array_equal(first[k], second[k]), k
    finally:
        for k, v in saved.items():
            setattr(a, k, v)
        eng = net._engine
        for e in (getattr(eng, '_par', None), getattr(eng, '_mx', None), eng):
            if isinstance(e, TrunkEngine):
                e.release_workspaces()
        net._engine = None
        del model, eng
        gc.collect()
        torch.cuda.empty_cache()
