"""(d') of tests/test_gpu_line_formats.py: the stem writes the model's bytes.  wsi_stem_conv7x7_bn_relu_maxpool (planes 1, 2, 3) and
wsi_stem_conv7x7_bn_relu_maxpool_lines96 against oracle/pf_lines_oracle.py, byte for byte, on inputs for which the expected line
needs no tolerance.

Weights: a tap selector - output channel co has the single weight 2^(co % 3 - 1) at tap (23 co + 5) % 147, read as (kh, kw, colour) -
packed by wsi_prepack_stem with an identity BatchNorm and a dyadic beta.  Inputs: values exact in the stem's 16-bit operand type, so
every conv value is one exact product plus the bias, and max / ReLU are exact.  Expected: that conv on the host, ReLU, the 3x3
stride-2 pad-1 maximum, O.encode.

Routes: f32 input under StemMode.FUSED (the strip kernel's float path) and StemMode.UNFUSED (conv kernel + pool kernel), u8 slide +
a dyadic LUT under StemMode.FUSED_LUT with tile corners left of, above and past the right / bottom edge of the slide - black outside
the slide, zero outside the patch.  The integer routes have non-dyadic folded weights; tests/test_gpu_stem_dense.py,
test_integer_stem_forms_bit_identical and the x0 tests of tests/test_gpu_unet.py tie them bit for bit to one another."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import pf_lines_oracle as O
from tests.test_gpu_line_formats import _host, _ok, _st, dev, lib       # noqa: F401 (dev, lib: fixtures)
from wsi_segmentation_pipeline_amd import native

pytestmark = pytest.mark.gpu

FILL = 0xAB
SHAPES = [(2, 64, 64), (2, 32, 72), (1, 128, 128)]     # pooled width 16: even layout, one strip; 18: odd layout, a second strip of three columns; 32: three strips
ROWS = [64, 5]                                         # pooled rows per workgroup: one segment; carry across segments, short last segment
SCALE_OF_SHAPE = {(2, 64, 64): 0, (2, 32, 72): 7, (1, 128, 128): -3}      # O.grid_values exponent: |x| < 4, < 512, < 0.5
SLIDE_HW = (90, 100)
ORIGINS = {(2, 64, 64): [(-5, -7), (60, 50)], (2, 32, 72): [(-5, -7), (60, 70)], (1, 128, 128): [(-9, -4)]}    # (x, y) tile corners


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _taps():
    t = (23 * np.arange(64) + 5) % 147
    return t // 21, (t // 3) % 7, t % 3, 2.0 ** (np.arange(64) % 3 - 1)            # kh, kw, colour, weight


BETA = (((5 * np.arange(64)) % 13 - 4) / 8.0).astype(np.float32)                   # -0.5 .. 1.0 in steps of 1/8


@functools.lru_cache(maxsize=None)
def _packed(planes):
    """the tap selector through wsi_prepack_stem (gamma 1, mean 0, var 1, eps 0): device tensors (pack, bias)"""
    lib_ = native.load()
    kh, kw, col, wv = _taps()
    w = np.zeros((64, 3, 7, 7), np.float32)
    w[np.arange(64), col, kh, kw] = wv
    one, zero = np.ones(64, np.float32), np.zeros(64, np.float32)
    pk = np.full(lib_.wsi_prepack_stem_bytes(planes), 0xEE, np.uint8)
    bias = np.full(64, np.nan, np.float32)
    _ok(lib_.wsi_prepack_stem(_np_ptr(w), _np_ptr(one), _np_ptr(BETA), _np_ptr(zero), _np_ptr(one), 0.0, planes, _np_ptr(pk), _np_ptr(bias)),
        'wsi_prepack_stem')
    assert np.array_equal(bias, BETA)                                              # the fold is the identity ...
    if planes >= 2:                                                                # ... on the weights too: fp16 hi plane = w, lo plane = 0
        frag = pk.view(np.float16).reshape(2, 14, 2, 64, 8).astype(np.float64)
        assert not frag[:, :, 1].any() and frag[:, :, 0].sum() == wv.sum() and np.count_nonzero(frag) == 64
    d = torch.device('cuda:0')
    return torch.from_numpy(pk).to(d), torch.from_numpy(bias).to(d)


def _round16(x, planes):
    """x rounded to the stem's operand type: bf16 for planes 1, fp16 otherwise"""
    if planes == 1:
        return (O._bf16_bits(x).astype(np.uint32) << 16).view(np.float32).reshape(x.shape)
    return x.astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _f32_input(shape, bf16):
    n, h, w = shape
    rng = np.random.default_rng(sum(shape) + 1000 * bf16)
    x = _round16(O.grid_values(rng, (n, 3, h, w), SCALE_OF_SHAPE[shape]), 1 if bf16 else 2)
    x.setflags(write=False)
    return x


LUT = ((np.arange(256, dtype=np.float64)[None, :] - 128) * 2.0 ** (np.arange(3)[:, None] - 4)).astype(np.float32)   # (b - 128) / 16, / 8, / 4


@functools.lru_cache(maxsize=None)
def _slide():
    s = np.random.default_rng(3).integers(0, 256, SLIDE_HW + (3,), dtype=np.uint8)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _slide_input(shape):
    """what the tiles of `shape` at ORIGINS[shape] hold after the LUT: black (code 0) outside the slide"""
    n, h, w = shape
    s, (sh, sw) = _slide(), SLIDE_HW
    x = np.empty((n, 3, h, w), np.float32)
    for i, (tx, ty) in enumerate(ORIGINS[shape]):
        yy, xx = np.meshgrid(ty + np.arange(h), tx + np.arange(w), indexing='ij')
        inside = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)
        px = np.where(inside[..., None], s[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0)
        for c in range(3):
            x[i, c] = LUT[c][px[..., c]]
    assert not inside.all()                                                        # (the last tile leaves the slide)
    x.setflags(write=False)
    return x


def _pooled(x):
    """conv 7x7 stride 2 pad 3 of the tap selector + beta, ReLU, max 3x3 stride 2 pad 1, on the host: (n, 64, h/4, w/4) float32,
    every value exact (asserted, as _expected_lines of tests/test_gpu_line_formats.py does)"""
    n, _, h, w = x.shape
    hc, wc, hp, wp = h // 2, w // 2, h // 4, w // 4
    xp = np.zeros((n, 3, h + 6, w + 6), np.float64)                                # zero outside the patch
    xp[:, :, 3:-3, 3:-3] = x
    kh, kw, col, wv = _taps()
    conv = np.stack([wv[co] * xp[:, col[co], kh[co]:kh[co] + 2 * hc:2, kw[co]:kw[co] + 2 * wc:2] + float(BETA[co]) for co in range(64)], 1)
    assert np.array_equal(conv.astype(np.float32).astype(np.float64), conv) and np.abs(conv).max() < O.F16_MAX
    act = np.zeros((n, 64, hc + 2, wc + 2), np.float64)                            # post-ReLU values are >= 0: 0 is the pool's padding
    act[:, :, 1:-1, 1:-1] = np.maximum(conv, 0.0)
    pooled = np.max([act[:, :, dy:dy + 2 * hp:2, dx:dx + 2 * wp:2] for dy in range(3) for dx in range(3)], 0)
    assert pooled.shape == (n, 64, hp, wp) and pooled.max() > 0
    return pooled.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _want(shape, source, planes):
    """expected 128-byte lines (n * hp * wp, lines per pixel, 128) of one case"""
    x = _slide_input(shape) if source == 'slide' else _f32_input(shape, planes == 1)
    want = O.encode(O.to_lines(_pooled(x), planes), planes)
    want.setflags(write=False)
    return want


def _lines96(want):
    """the 96-byte form of planes-3 lines: fp16 plane, lo6 bytes 0-15, lo6 bytes 16-23, scale_lo dword, scale_hi dword"""
    return np.concatenate([want[..., 0:64], want[..., 64:80], want[..., 96:104], want[..., 104:108], want[..., 120:124]], -1)


def _run(lib, dev, shape, source, planes, lines96, mode, rows):
    """one stem call; the whole output buffer (filled with FILL first) as host bytes"""
    n, h, w = shape
    hp, wp = h // 4, w // 4
    wpk, bias = _packed(planes)
    nbytes = lib.wsi_pf_bytes(n, hp, wp, 64, planes)
    plane96 = lib.wsi_pf_bytes(n, hp, wp, 64, 3) // 256 * 96
    out = torch.full((2 * plane96 if lines96 else nbytes,), FILL, dtype=torch.uint8, device=dev)
    scratch = torch.empty(n * (h // 2) * (w // 2) * 64, dtype=torch.float32, device=dev)
    if source == 'slide':
        sl = torch.from_numpy(_slide().copy()).to(dev)
        xy = torch.tensor(ORIGINS[shape], dtype=torch.int32, device=dev)
        lut = torch.from_numpy(LUT).to(dev)
        src = [None, sl.data_ptr(), sl.stride(0), sl.shape[0], sl.shape[1], xy.data_ptr(), lut.data_ptr()]
    else:
        x = torch.from_numpy(_f32_input(shape, planes == 1).copy()).to(dev)
        src = [x.data_ptr(), None, 0, 0, 0, None, None]
    args = src + [wpk.data_ptr(), bias.data_ptr(), None, None, None, n, h, w, scratch.data_ptr(), out.data_ptr()]
    with native.stem_mode(mode, rows):
        if lines96:
            rc = lib.wsi_stem_conv7x7_bn_relu_maxpool_lines96(*args, plane96, _st())
        else:
            rc = lib.wsi_stem_conv7x7_bn_relu_maxpool(*args, planes, _st())
    _ok(rc, 'stem planes %d lines96 %d' % (planes, lines96))
    return _host(out)


def _check(lib, dev, shape, source, planes, lines96, mode, rows):
    n, h, w = shape
    hp, wp = h // 4, w // 4
    buf = _run(lib, dev, shape, source, planes, lines96, mode, rows)
    want = _want(shape, source, planes)
    what = '%s %s planes %d lines96 %d mode %s rows %d' % (shape, source, planes, lines96, native.StemMode(mode).name, rows)
    if not lines96:
        d = O.diff_lines(O.real_lines(buf, n, 64, hp, wp, planes), want)
        assert d is None, '%s: %s' % (what, d)
        assert np.all(O.other_bytes(buf, n, 64, hp, wp, planes) == FILL), '%s: a byte outside the real lines was written' % what
        return
    px = O.real_pixels(n, hp, wp)
    got = buf.reshape(2, -1, 96)                                                    # line-planar: [line][pixel][96]
    w96 = _lines96(want)
    for line in range(2):
        bad = np.nonzero((got[line][px] != w96[:, line]).any(1))[0]
        assert bad.size == 0, '%s: %d lines of plane %d differ; first: pixel %d\n  got  %s\n  want %s' % (
            what, bad.size, line, bad[0], got[line][px][bad[0]].tobytes().hex(), w96[bad[0], line].tobytes().hex())
    rest = np.ones(got.shape[1], bool)
    rest[px] = False
    assert np.all(got[:, rest] == FILL), '%s: a byte outside the real lines was written' % what


FORMS = [(1, False), (2, False), (3, False), (3, True)]                             # (planes, 96-byte lines)


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_stem_f32_fused_writes_the_model_bytes(dev, lib, shape, rows):
    for planes, lines96 in FORMS:
        _check(lib, dev, shape, 'f32', planes, lines96, native.StemMode.FUSED, rows)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_stem_f32_unfused_writes_the_model_bytes(dev, lib, shape):
    """the two-kernel form: conv kernel to f32 NHWC, then the pool kernel's line store (it has no segments: rows is not read)"""
    for planes in (1, 2):
        _check(lib, dev, shape, 'f32', planes, False, native.StemMode.UNFUSED, 64)


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_stem_slide_lut_writes_the_model_bytes(dev, lib, shape, rows):
    """u8 slide + LUT on the float kernels: the slide pixel fetch, black outside the slide, zero outside the patch"""
    for planes, lines96 in FORMS:
        _check(lib, dev, shape, 'slide', planes, lines96, native.StemMode.FUSED_LUT, rows)
