"""CPU tests of oracle/pf_lines_oracle.py, the host model that tests/test_gpu_line_formats.py holds every writer and reader
of the 128-byte activation lines to: the model is checked against brute force (fp6 rounding, scale choice), against its own
invariants (position maps, round trips), against the one place the library's own fp6 / scale code runs without a GPU (the
mode-3 weight pack), and it is shown to notice the three mistakes a line codec is most likely to make."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import pf_lines_oracle as O
from wsi_segmentation_pipeline_amd import native


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


def _f32_from_bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


# ---------------------------------------------------------------------------------------------- fp6
def test_fp6_table_is_e2m3():
    t = O.FP6_TABLE.astype(np.float64)
    assert t.shape == (64,) and np.array_equal(t[32:], -t[:32])
    mag = t[:32]
    assert np.unique(mag).size == 32 and np.all(np.diff(mag) > 0) and mag[0] == 0.0 and mag[31] == 7.5
    # e2m3 spacing: 1/8 up to 2 (subnormals and the first binade), 1/4 in [2, 4), 1/2 in [4, 7.5]
    assert np.array_equal(np.diff(mag), np.r_[np.full(16, 0.125), np.full(8, 0.25), np.full(7, 0.5)])
    assert np.array_equal(O.fp6_value(np.arange(64)), O.FP6_TABLE)
    assert np.array_equal(O.fp6_encode(t), np.arange(64))                           # every code is its own nearest (0x20 = -0 included)


def _fp6_brute(y):
    """nearest entry of the 32 magnitudes, ties to the even code; plain loops"""
    mag = O.FP6_TABLE[:32].astype(np.float64)
    out = np.empty(y.shape, np.uint8)
    for i, v in enumerate(y):
        d = np.abs(min(abs(v), 9.0) - mag)                                            # (past the table the nearest entry is its last: inf too)
        best = np.nonzero(d == d.min())[0]                                           # one entry, or two neighbours at a tie
        code = int(best[0]) if best.size == 1 else int(best[best % 2 == 0][0])
        out[i] = code | (32 if np.signbit(v) else 0)
    return out


def test_fp6_encode_equals_brute_force():
    y = np.r_[np.arange(-9 * 64, 9 * 64 + 1) / 64.0, np.inf, -np.inf, -0.0]
    got = O.fp6_encode(y)
    assert np.array_equal(got, _fp6_brute(y))
    assert np.all(O.fp6_value(got[np.abs(y) >= 7.5]).astype(np.float64) == np.sign(y[np.abs(y) >= 7.5]) * 7.5)   # saturation
    # the grid holds every tie of the format (all midpoints are multiples of 2^-4); some by name, both parities
    for v, want in ((0.0625, 0.0), (0.1875, 0.25), (2.125, 2.0), (2.375, 2.5), (4.25, 4.0), (4.75, 5.0), (7.25, 7.0), (1.9375, 2.0)):
        assert float(O.fp6_value(O.fp6_encode(np.float64(v)))) == want and float(O.fp6_value(O.fp6_encode(np.float64(-v)))) == -want
    away = O.fp6_value(O.fp6_encode(np.array([0.0625, 2.125, 4.25]), ties='away'))
    assert np.array_equal(away, np.float32([0.125, 2.25, 4.5]))                      # the wrong rule really is another rule


# ---------------------------------------------------------------------------------------------- scale byte
def test_scale_byte_equals_brute_force():
    """Every fp32 exponent with the mantissas around the bump.  The rule, searched rather than computed: the smallest power of two
    2^(s-127), s in [1, 254], for which the saturating fp6 conversion of amax / scale costs no more than the top binade's own
    rounding error (half a step = 0.25), i.e. amax / scale <= 7.75.  Mantissa 0x780000 is that boundary exactly: 7.75 lies
    halfway between 7.5 and the 8.0 the format does not have, and the saturating convert resolves it to 7.5, so it does not
    bump; 0x780001 does."""
    e = np.arange(0, 255, dtype=np.uint32)
    m = np.array([0, 0x77ffff, 0x780000, 0x780001, 0x7fffff], np.uint32)
    amax = _f32_from_bits((e[:, None] << 23) | m[None, :]).reshape(-1)
    got = O.scale_byte(amax).astype(np.int64)
    s = np.arange(1, 255)
    q = amax.astype(np.float64)[:, None] / np.ldexp(1.0, s - 127)[None, :]                  # exact: powers of two
    ok = q <= 7.75
    want = np.where(ok.any(1), s[np.argmax(ok, 1)], 254)
    want[amax == 0] = 0
    assert np.array_equal(got, want)
    assert got[amax == 0].tolist() == [0] and np.all(got[amax != 0] >= 1)
    # the library's own rule on the same sample, through the only host-side window there is: see test_weight_pack_*
    # quantised maximum in fp6's top binade [4, 7.5] unless the [1, 254] clamp is active (s = 1 for blocks below 3.875 * 2^-126;
    # no finite fp32 reaches s = 254)
    live = (amax != 0) & ~((got == 1) & (q[:, 0] <= 3.875))
    qmax = O.fp6_value(O.fp6_encode(amax.astype(np.float64) / O.scale_value(np.maximum(got, 1)))).astype(np.float64)
    assert np.all(qmax[live] >= 4.0) and np.all(qmax[live] <= 7.5) and live.sum() > 1200
    assert got.max() < 254
    # the bump sits exactly between mantissa 0x780000 and 0x780001
    b = O.scale_byte(_f32_from_bits([0x3ff80000 - 1, 0x3ff80000, 0x3ff80001]))
    assert b.tolist() == [125, 125, 126]


# ---------------------------------------------------------------------------------------------- positions, geometry
def test_position_maps_are_inverse_permutations():
    idx = np.arange(32)
    for a, b in ((O.POS_OF_CHAN, O.CHAN_OF_POS), (O.FIELD_OF_CHAN, O.CHAN_OF_FIELD)):
        assert np.array_equal(np.sort(a), idx) and np.array_equal(a[b], idx) and np.array_equal(b[a], idx)
    assert np.array_equal(O.FIELD_OF_POS, 2 * (idx & 15) + (idx >> 4))                # field 2r + h of position 16h + r
    # a lane (pixel, h) owns channels 8g + 4h + i: 16 contiguous positions, every other field
    for h in (0, 1):
        ch = np.array([8 * g + 4 * h + i for g in range(4) for i in range(4)])
        assert np.array_equal(O.POS_OF_CHAN[ch], 16 * h + np.arange(16)) and np.array_equal(O.FIELD_OF_CHAN[ch], 2 * np.arange(16) + h)
    codes = np.random.default_rng(1).integers(0, 64, (7, 32)).astype(np.uint8)
    assert np.array_equal(O.unpack_fields(O.pack_fields(codes)), codes)
    one = np.zeros(32, np.uint8); one[5] = 63
    assert int.from_bytes(O.pack_fields(one).tobytes(), 'little') == 63 << 30          # field f at bit 6f


def test_pf_geometry_matches_the_library(lib):
    for n, c, h, w, planes in ((3, 64, 5, 7, 1), (2, 96, 3, 9, 3), (1, 512, 2, 2, 2), (2, 128, 4, 33, 3)):
        nbytes = lib.wsi_pf_bytes(n, h, w, c, planes)
        q = O.real_pixels(n, h, w)
        want = [lib.wsi_pf_pixel_index(i, y, x, h, w) for i in range(n) for y in range(h) for x in range(w)]
        assert q.tolist() == want
        bpp = c * O.BYTES_PER_CHANNEL[planes]
        assert nbytes % bpp == 0 and q.max() < nbytes // bpp and np.unique(q).size == n * h * w
        buf = np.zeros(nbytes, np.uint8)
        lines = np.random.default_rng(2).integers(1, 256, (n * h * w, c // O.CHANNELS[planes], 128)).astype(np.uint8)
        O.set_real_lines(buf, lines, n, c, h, w, planes)
        assert np.array_equal(O.real_lines(buf, n, c, h, w, planes), lines)
        other = O.other_bytes(buf, n, c, h, w, planes)
        assert other.size + lines.size == nbytes and not other.any()
        x = np.random.default_rng(3).standard_normal((n, c, h, w)).astype(np.float32)
        assert np.array_equal(O.from_lines(O.to_lines(x, planes), n, c, h, w), x)
        assert O.to_lines(x, planes)[w + 1, 0, 1] == x[0, 1, 1, 1]                     # pixel (0, 1, 1), line 0, channel 1


# ---------------------------------------------------------------------------------------------- round trips
def _sample_lines(planes, count=600):
    rng = np.random.default_rng(10 + planes)
    x = rng.standard_normal((count, O.CHANNELS[planes])) * 2.0 ** rng.integers(-20, 15, (count, 1))
    return np.concatenate([O.crafted_lines(planes), x.astype(np.float32)])


def test_roundtrip_planes3_within_half_an_fp6_step():
    x = _sample_lines(3)
    b = O.encode(x, 3)
    t = np.clip(x, -O.F16_MAX, O.F16_MAX).astype(np.float64)
    step = O.scale_value(b[:, O.SCALE_LO])[:, None]                                    # half the top-binade step 0.5 = 0.25 of the scale
    assert np.all(np.abs(O.decode(b, 3).astype(np.float64) - t) <= 0.25 * step)
    # the s = 1 clamp aside (blocks below 2^-124: not in the sample), the lo block is scaled into the top binade: step <= amax / 3.75
    lo = t - t.astype(np.float16).astype(np.float64)
    assert np.all(b[:, O.SCALE_LO] != 1) and np.all(3.75 * step[:, 0] <= np.abs(lo).max(1) + (step[:, 0] == 0))
    # the hi6 plane stands for the fp16 plane to half a step of ITS scale
    hi = t.astype(np.float16).astype(np.float64)
    assert np.all(np.abs(O.decode_hi6(b) - hi) <= 0.25 * O.scale_value(b[:, O.SCALE_HI])[:, None])
    assert not b[:, 105:112].any() and not b[:, 121:128].any()                         # dwords 27 / 31 (and the scale dwords' upper bytes)


def test_roundtrip_planes2_and_1_exact():
    x = _sample_lines(2)
    t = np.clip(x, np.float32(-O.F16_MAX), np.float32(O.F16_MAX))
    hi = t.astype(np.float16)
    lo = (t - hi.astype(np.float32)).astype(np.float16)
    b = O.encode(x, 2)
    assert np.array_equal(O.decode(b, 2).view(np.uint32), (hi.astype(np.float32) + lo.astype(np.float32)).view(np.uint32))
    assert np.array_equal(b[:, :64].copy().view(np.float16).view(np.uint16), hi.view(np.uint16))
    assert np.array_equal(b[:, 64:].copy().view(np.float16).view(np.uint16), lo.view(np.uint16))
    assert np.all(np.isfinite(O.decode(b, 2)))                                          # 1e6 and +-inf clamp
    x = _sample_lines(1)
    b = O.encode(x, 1)
    d = O.decode(b, 1)
    fin = np.isfinite(x)
    assert np.all(np.abs(d[fin].astype(np.float64) - x[fin]) <= 2.0 ** -8 * np.abs(x[fin])) and np.array_equal(d[~fin], x[~fin])
    assert np.array_equal(O.encode(d, 1), b)
    # ties to even: 1 + 2^-8 is halfway between 1 and 1 + 2^-7; 1 + 3 * 2^-8 between 1 + 2^-7 and 1 + 2^-6
    v = np.zeros((1, 64), np.float32); v[0, :2] = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8
    assert O.decode(O.encode(v, 1), 1)[0, :2].tolist() == [1.0, 1 + 2.0 ** -6]


# ---------------------------------------------------------------------------------------------- the library's host-side codec
def test_weight_pack_holds_the_model_lines(lib):
    """wsi_prepack_conv (planes 3) runs the library's own fp6_encode / mx6_scale_byte on the host: the fragments of one (cout,
    line, tap) block, put back in line order, are the 128 bytes the model encodes for the same 32 values - fp16 plane, both
    fp6 planes and both scale bytes; the crafted lines (scale bump, ties, subnormals) among the weights."""
    rng = np.random.default_rng(5)
    cout, cin, k = 32, 64, 3
    w = (rng.standard_normal((cout, cin, k, k)) * 2.0 ** rng.integers(-12, 8, (cout, 1, k, k))).astype(np.float32)
    crafted = O.crafted_lines(3)
    crafted = crafted[np.abs(crafted).max(1) <= O.F16_MAX]                               # (the weight pack does not clamp)
    assert crafted.shape[0] >= 16
    w[:crafted.shape[0], :32, 1, 1] = crafted
    w[:crafted.shape[0], 32:, 0, 2] = crafted[::-1]
    out = np.zeros(lib.wsi_prepack_conv_bytes(cout, cin, k, 3), np.uint8)
    bias = np.zeros(cout, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.wsi_prepack_conv(p(w), None, None, None, None, 1e-5, cout, cin, k, 3, p(out), p(bias)) == 0
    blocks = out.reshape(cin // 32, 9, 4, 64, 16)                                        # [line][tap][frag][lane][16 B]
    got = np.zeros((cin // 32, 9, 32, 128), np.uint8)
    r = np.arange(32)
    for h in (0, 1):
        got[:, :, :, 16 * h:16 * h + 16] = blocks[:, :, 0, r + 32 * h]                   # fp16 positions 8h .. 8h + 7
        got[:, :, :, 32 + 16 * h:48 + 16 * h] = blocks[:, :, 1, r + 32 * h]              # positions 16 + 8h ..
    for plane, lanes in ((0, r + 32), (1, r)):                                           # lo6 plane: lanes h = 1; hi6: lanes h = 0
        got[:, :, :, 64 + 16 * plane:80 + 16 * plane] = blocks[:, :, 2, lanes]
        got[:, :, :, 96 + 16 * plane:112 + 16 * plane] = blocks[:, :, 3, lanes]
    want = O.encode(w.reshape(cout, cin // 32, 32, 9).transpose(1, 3, 0, 2), 3)          # [line][tap][cout][32 channels]
    assert O.diff_lines(got, want) is None, O.diff_lines(got, want)


# ---------------------------------------------------------------------------------------------- the model bites
def test_comparison_notices_a_wrong_codec():
    """On the crafted lines of the pack test: a hi6 scale byte off by one, two fp6 fields swapped and ties rounded away from zero
    are each reported by the comparison helper the GPU tests assert on."""
    x = O.crafted_lines(3)
    want = O.encode(x, 3)
    assert O.diff_lines(want, want.copy()) is None

    def noticed(bad):
        return O.diff_lines(bad, want) is not None
    bad = want.copy()
    bad[:, O.SCALE_HI] += (bad[:, O.SCALE_HI] != 0)
    assert noticed(bad) and 'bytes [120]' in O.diff_lines(bad, want)
    for where in (np.r_[64:80, 96:104], np.r_[80:96, 112:120]):                         # either plane
        bad = want.copy()
        f = O.unpack_fields(bad[:, where])
        f[:, [6, 7]] = f[:, [7, 6]]
        bad[:, where] = O.pack_fields(f)
        assert noticed(bad)
    bad = O.encode(x, 3, fp6_ties='away')
    assert noticed(bad)
    tie_lines = np.nonzero((bad != want).any(1))[0]
    assert tie_lines.size >= 2 and np.array_equal(bad[:, :64], want[:, :64]) and np.array_equal(bad[:, [104, 120]], want[:, [104, 120]])
    # the crafted lines hold the negative-zero code (a negative lo that rounds to zero keeps its sign bit): part of the pinned bytes
    assert (O.lo6_codes(want) == 0x20).any() and (O.hi6_codes(want) == 0x20).any()


# ---------------------------------------------------------------------------------------------- the conv test's exact sums
@pytest.mark.parametrize('planes', [1, 2, 3])
def test_conv_epilogue_inputs_sum_exactly(planes):
    """The premise of the conv epilogue test: with x, residual and bias on the 2^-14 grid (|value| < 4, times 2^k), decoded input +
    bias + decoded residual is exact in fp32 in every order of the three terms, so its expected line needs no tolerance."""
    rng = np.random.default_rng(planes)
    nch = O.CHANNELS[planes]
    for k in (-14, -6, 0, 5, 12):
        x = O.decode(O.encode(O.grid_values(rng, (400, nch), k), planes), planes)
        r = O.decode(O.encode(O.grid_values(rng, (400, nch), k), planes), planes)
        b = O.grid_values(rng, (1, nch), k)
        exact = x.astype(np.float64) + b.astype(np.float64) + r.astype(np.float64)
        for s in ((x + b) + r, (x + r) + b, (b + r) + x):
            assert s.dtype == np.float32 and np.array_equal(s.astype(np.float64), exact)
        for pair in (x + b, x + r, b + r):
            assert pair.dtype == np.float32
        assert np.array_equal((x + b).astype(np.float64), x.astype(np.float64) + b) and np.array_equal((b + r).astype(np.float64), r.astype(np.float64) + b)
        assert np.abs(exact).max() < O.F16_MAX
