"""The dense column mapping of the integer, mx-output stem (stem.hip stem_pool_dense_kernel: pooled maps 64 or 128 wide) against the
strip form it replaces there, through the A/B switch (native.StemMode.FUSED_STRIPS): every conv value is the same exact integer sum
through the same rounded, monotone map, so the output lines agree bit for bit - the whole buffer is compared, pads included."""
import ctypes as C

import numpy as np
import pytest
import torch

from wsi_segmentation_pipeline_amd import native, synthetic as W
from wsi_segmentation_pipeline_amd.engine import TrunkEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def eng(dev):
    sd = W.make_resnet18_state_dict(11, with_fc=False)
    cls = W.make_head_state_dict(22, 'classifier')
    return TrunkEngine(sd, dev, planes=3, head=(cls['fc.0.weight'], cls['fc.0.bias']))


@pytest.fixture(scope='module')
def slide(dev):
    return torch.from_numpy(np.random.default_rng(5).integers(0, 256, (300, 300, 3), dtype=np.uint8)).to(dev)


ORIGINS = [(0, 0), (-5, -7), (120, 90)]          # inside; black on the left and top; past the right and bottom edge of the 300 x 300 slide


def _stem_lines(eng, slide, xy, tile, mode, rows, lines96):
    """raw output bytes of the stem + pool of the tiles at xy, under wsi_stem_set_mode(mode, rows)"""
    lib, dev = native.load(), slide.device
    n = len(xy)
    xyd = torch.tensor(xy, dtype=torch.int32, device=dev)
    pixels = lib.wsi_pf_bytes(n, tile // 4, tile // 4, 64, 3) // 256
    plane96 = pixels * 96
    out = torch.full((2 * plane96 if lines96 else pixels * 256,), 0xAB, dtype=torch.uint8, device=dev)
    scratch = torch.empty(n * (tile // 2) * (tile // 2) * 64, dtype=torch.float32, device=dev)
    wt = eng.wt
    args = [None, slide.data_ptr(), slide.stride(0), slide.shape[0], slide.shape[1], xyd.data_ptr(), eng.lut.data_ptr(),
            wt.stem_w, wt.stem_b, wt.stem_w_u8, wt.stem_b_u8, C.cast(wt.norm, C.c_void_p), n, tile, tile, scratch.data_ptr(), out.data_ptr()]
    st = torch.cuda.current_stream().cuda_stream
    with native.stem_mode(mode, rows):
        if lines96:
            rc = lib.wsi_stem_conv7x7_bn_relu_maxpool_lines96(*args, plane96, st)
        else:
            rc = lib.wsi_stem_conv7x7_bn_relu_maxpool(*args, 3, st)
    native.check(rc, 'stem')
    torch.cuda.synchronize()
    return out


def _same(eng, slide, xy, tile, rows, lines96):
    new = _stem_lines(eng, slide, xy, tile, native.StemMode.FUSED, rows, lines96)
    old = _stem_lines(eng, slide, xy, tile, native.StemMode.FUSED_STRIPS, rows, lines96)
    assert bool((old != 0xAB).any())                       # the reference route wrote something
    assert torch.equal(new, old), (len(xy), tile, rows, lines96, int((new != old).sum()))


@pytest.mark.parametrize('lines96', [True, False])
@pytest.mark.parametrize('rows', [64, 16, 5])
def test_one_band_both_units_and_segments(eng, slide, rows, lines96):
    """256 x 256 tiles (pooled width 64: one band of two units): the shared column at pooled column 32, the padding lane at column 0,
    the last column 63; one segment, four, and thirteen with a short last one (5 does not divide 64)"""
    _same(eng, slide, ORIGINS, 256, rows, lines96)


@pytest.mark.parametrize('lines96', [True, False])
def test_single_tile(eng, slide, lines96):
    _same(eng, slide, [(17, 3)], 256, 64, lines96)
    _same(eng, slide, [(17, 3)], 256, 24, lines96)         # 64 = 24 + 24 + 16


@pytest.mark.parametrize('lines96', [True, False])
def test_tiles_512(eng, slide, lines96):
    """pooled width 128: four units in a row, three shared columns"""
    _same(eng, slide, [(-9, -4), (40, 30)], 512, 64, lines96)
    _same(eng, slide, [(-9, -4), (40, 30)], 512, 48, lines96)


@pytest.mark.parametrize('lines96', [True, False])
@pytest.mark.parametrize('tile', [288, 64])
def test_other_widths_keep_the_strip_form(eng, slide, tile, lines96):
    """pooled widths 72 and 16 run the strip kernel with the switch in either position"""
    _same(eng, slide, ORIGINS, tile, 64, lines96)


def test_trunk_logits_end_to_end(eng, slide, dev):
    rng = np.random.default_rng(9)
    xy = torch.from_numpy(rng.integers(-20, 120, (8, 2)).astype(np.int32)).to(dev)
    new = eng.forward_tiles(slide, xy, 256, 256, logits=True)[1].clone()
    with native.stem_mode(native.StemMode.FUSED_STRIPS, 64):
        old = eng.forward_tiles(slide, xy, 256, 256, logits=True)[1].clone()
    with native.conv_mode(native.ConvMode.L1_LINES128):                      # 128-byte lines between the stem and layer 1
        new128 = eng.forward_tiles(slide, xy, 256, 256, logits=True)[1].clone()
        with native.stem_mode(native.StemMode.FUSED_STRIPS, 64):
            old128 = eng.forward_tiles(slide, xy, 256, 256, logits=True)[1].clone()
    assert torch.isfinite(old).all() and float(old.abs().max()) > 0
    assert torch.equal(new, old) and torch.equal(new128, old128)
