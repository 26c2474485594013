"""Bit-exact NumPy model of the 128-byte activation lines of the padded-flat (PF) layout (test infrastructure only).

The three encodings (include/wsi_hip.h `planes`):

  planes 1  64 channels, bf16 (round to nearest even).
  planes 2  32 channels: x clamped to +-65504, hi = fp16(x) at bytes 0-63, lo = fp16(x - hi) at bytes 64-127.
  planes 3  32 channels: x clamped to +-65504, hi = fp16(x), lo = x - hi (fp32, exact).  Each of the two planes (lo, hi)
            is one MX block: an E8M0 scale byte s and 32 fp6 (e2m3) codes of value / 2^(s-127), round to nearest even,
            saturating at 7.5.  s is the smallest exponent that brings the block's largest magnitude to at most 7.75
            (half a top-binade step over fp6's largest value, 7.5), clamped to [1, 254]; 0 for an all-zero block,
            which decodes to zeros.  Bytes: [fp16 hi x32 | lo6 bytes 0-15 | hi6 bytes 0-15 | lo6 bytes 16-23, scale_lo,
            7 zero bytes | hi6 bytes 16-23, scale_hi, 7 zero bytes].  Channel c = 8g + 4h + i sits at fp16 position
            16h + 4g + i and at fp6 field 2(4g + i) + h; field f occupies bits 6f .. 6f+5 of its 192-bit plane.
            A reader takes x = f32(hi) + fp6(lo6 field) * 2^(scale_lo - 127); the hi6 plane is only ever an MFMA operand.

Everything here is vectorised over lines: `encode` / `decode` take (..., channels) / (..., 128) arrays.
"""
import numpy as np

F16_MAX = 65504.0
CHANNELS = {1: 64, 2: 32, 3: 32}            # channels per 128-byte line
BYTES_PER_CHANNEL = {1: 2, 2: 4, 3: 4}      # bytes per channel in a pixel record

# ---------------------------------------------------------------------------------------------- fp6 (e2m3)
# code = s eemmm: e = 0 -> m / 8 (subnormals), else (1 + m / 8) * 2^(e - 1); the magnitudes ascend with the 5 low bits
_M = np.arange(32)
FP6_MAGNITUDES = np.where(_M < 8, _M / 8.0, (1.0 + (_M & 7) / 8.0) * 2.0 ** ((_M >> 3) - 1.0))
FP6_TABLE = np.concatenate([FP6_MAGNITUDES, -FP6_MAGNITUDES]).astype(np.float32)      # value of each of the 64 codes
_FP6_MID = (FP6_MAGNITUDES[1:] + FP6_MAGNITUDES[:-1]) / 2.0


def fp6_value(code):
    return FP6_TABLE[np.asarray(code, np.uint8) & 63]


def fp6_encode(y, ties='even'):
    """Nearest fp6 code of y (any float array, no NaN): ties to the even code, magnitudes from 7.5 up (inf included) saturate
    to 7.5, the sign bit is y's (a negative value that rounds to zero gives 0x20).  ties='away' is a deliberately wrong
    rule that the model's own tests use to show that a comparison against this model notices it."""
    y = np.asarray(y, np.float64)
    a = np.abs(y)
    idx = np.searchsorted(_FP6_MID, a, side='left')                   # number of midpoints below a: a tie picks the lower code
    tie = (idx < 31) & (a == _FP6_MID[np.minimum(idx, 30)])
    idx = idx + (tie & (((idx & 1) == 1) if ties == 'even' else True))
    return (idx | np.where(np.signbit(y), 32, 0)).astype(np.uint8)


def scale_byte(amax):
    """E8M0 byte of a block whose largest magnitude is amax (float32 array)."""
    amax = np.abs(np.asarray(amax, np.float32)).astype(np.float64)
    with np.errstate(divide='ignore'):
        m, e = np.frexp(amax)                                         # amax = m * 2^e, m in [0.5, 1)
    s = 127 + (e - 1) - 2 + (2.0 * m > 1.9375)                         # 7.75 = 1.9375 * 2^2
    return np.where(amax == 0, 0, np.clip(s, 1, 254)).astype(np.uint8)


def scale_value(s):
    """2^(s - 127) as float64; 0 for s = 0."""
    s = np.asarray(s).astype(np.int64)
    return np.where(s == 0, 0.0, np.ldexp(1.0, s - 127))


# ---------------------------------------------------------------------------------------------- planes-3 line positions
_C = np.arange(32)
POS_OF_CHAN = 16 * ((_C >> 2) & 1) + 4 * (_C >> 3) + (_C & 3)          # channel 8g + 4h + i -> fp16 position 16h + 4g + i
CHAN_OF_POS = np.argsort(POS_OF_CHAN)
FIELD_OF_CHAN = 2 * (4 * (_C >> 3) + (_C & 3)) + ((_C >> 2) & 1)        # -> fp6 field 2(4g + i) + h
CHAN_OF_FIELD = np.argsort(FIELD_OF_CHAN)
FIELD_OF_POS = FIELD_OF_CHAN[CHAN_OF_POS]

_LO6 = np.r_[64:80, 96:104]                                            # byte offsets of the 24 bytes of each fp6 plane
_HI6 = np.r_[80:96, 112:120]
SCALE_LO, SCALE_HI = 104, 120                                          # dwords 26 / 30; dwords 27 / 31 stay zero
_BITS = np.arange(6, dtype=np.uint8)


def pack_fields(codes):
    """(..., 32) fp6 codes in FIELD order -> (..., 24) plane bytes (field f at bits 6f .. 6f + 5, little endian)."""
    codes = np.asarray(codes, np.uint8)
    bits = (codes[..., None] >> _BITS) & 1
    return np.packbits(bits.reshape(codes.shape[:-1] + (192,)), axis=-1, bitorder='little')


def unpack_fields(plane):
    """(..., 24) plane bytes -> (..., 32) fp6 codes in FIELD order."""
    plane = np.asarray(plane, np.uint8)
    bits = np.unpackbits(plane, axis=-1, bitorder='little').reshape(plane.shape[:-1] + (32, 6))
    return (bits << _BITS).sum(-1).astype(np.uint8)


def lo6_codes(lines):
    """fp6 codes of the lo6 plane of (..., 128) planes-3 lines, in CHANNEL order."""
    return unpack_fields(np.asarray(lines, np.uint8)[..., _LO6])[..., FIELD_OF_CHAN]


def hi6_codes(lines):
    return unpack_fields(np.asarray(lines, np.uint8)[..., _HI6])[..., FIELD_OF_CHAN]


# ---------------------------------------------------------------------------------------------- encode / decode
def _bf16_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)     # round to nearest even (inf stays inf; no NaN here)


def _f16_bytes(v16):
    return np.ascontiguousarray(v16, np.float16).view(np.uint8).reshape(v16.shape[:-1] + (2 * v16.shape[-1],))


def encode(values, planes, fp6_ties='even'):
    """(..., 64 | 32) float32 channel values -> (..., 128) uint8 line bytes."""
    v = np.ascontiguousarray(values, np.float32)
    assert v.shape[-1] == CHANNELS[planes]
    if planes == 1:
        b = _bf16_bits(v)
        return b.view(np.uint8).reshape(v.shape[:-1] + (128,))
    t = np.clip(v, np.float32(-F16_MAX), np.float32(F16_MAX))
    hi16 = t.astype(np.float16)
    hi = hi16.astype(np.float32)
    lo = t - hi                                                       # exact in fp32
    out = np.zeros(v.shape[:-1] + (128,), np.uint8)
    if planes == 2:
        out[..., :64] = _f16_bytes(hi16)
        out[..., 64:] = _f16_bytes(lo.astype(np.float16))
        return out
    out[..., :64] = _f16_bytes(hi16[..., CHAN_OF_POS])
    for plane, where, sbyte in ((lo, _LO6, SCALE_LO), (hi, _HI6, SCALE_HI)):
        s = scale_byte(np.abs(plane).max(-1))
        sv = scale_value(s)[..., None]
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(sv == 0, plane.astype(np.float64) * 0.0, plane.astype(np.float64) / sv)     # power-of-two scale: exact
        out[..., where] = pack_fields(fp6_encode(q, fp6_ties)[..., CHAN_OF_FIELD])
        out[..., sbyte] = s
    return out


def decode(lines, planes):
    """(..., 128) uint8 -> (..., 64 | 32) float32 channel values, with the readers' float32 arithmetic."""
    b = np.ascontiguousarray(lines, np.uint8)
    assert b.shape[-1] == 128
    if planes == 1:
        return (b.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    h = b[..., :64].copy().view(np.float16).astype(np.float32)
    if planes == 2:
        return h + b[..., 64:].copy().view(np.float16).astype(np.float32)
    sc = scale_value(b[..., SCALE_LO]).astype(np.float32)[..., None]   # 2^(s - 127): a float32 for every s in [1, 254]
    with np.errstate(over='ignore'):
        return h[..., POS_OF_CHAN] + fp6_value(lo6_codes(b)) * sc


def decode_hi6(lines):
    """The value the hi6 plane of planes-3 lines stands for: fp6(field) * 2^(scale_hi - 127), float64, channel order."""
    b = np.ascontiguousarray(lines, np.uint8)
    return fp6_value(hi6_codes(b)).astype(np.float64) * scale_value(b[..., SCALE_HI])[..., None]


def diff_lines(got, want):
    """None if two (..., 128) byte arrays are equal, else a one-line report of the first differing line (the helper the
    byte-for-byte tests assert on)."""
    got, want = np.asarray(got, np.uint8).reshape(-1, 128), np.asarray(want, np.uint8).reshape(-1, 128)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(1))[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    cols = np.nonzero(got[i] != want[i])[0]
    return '%d of %d lines differ; first: line %d, bytes %s\n  got  %s\n  want %s' % (
        bad.size, got.shape[0], i, cols.tolist(), got[i].tobytes().hex(), want[i].tobytes().hex())


# ---------------------------------------------------------------------------------------------- PF geometry
def pixel_index(n, y, x, h, w):
    """PF position of pixel (n, y, x) of an (h, w) map (wsi_pf_pixel_index): one zero column per row, one zero row per
    image, w + 2 guard pixels in front."""
    return (w + 2) + np.asarray(n, np.int64) * (h + 1) * (w + 1) + np.asarray(y, np.int64) * (w + 1) + x


def real_pixels(n, h, w):
    """PF positions of the n*h*w real pixels in (n, y, x) raster order."""
    nn, yy, xx = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing='ij')
    return pixel_index(nn, yy, xx, h, w).reshape(-1)


def real_lines(buf, n, c, h, w, planes):
    """The (n*h*w, lines, 128) bytes of the real pixels of a PF buffer (a copy, raster order)."""
    px = np.asarray(buf, np.uint8).reshape(-1, c * BYTES_PER_CHANNEL[planes])
    return px[real_pixels(n, h, w)].reshape(n * h * w, c // CHANNELS[planes], 128)


def set_real_lines(buf, lines, n, c, h, w, planes):
    """Write (n*h*w, lines, 128) bytes into the real pixels of a PF buffer, in place."""
    px = buf.reshape(-1, c * BYTES_PER_CHANNEL[planes])
    px[real_pixels(n, h, w)] = np.asarray(lines, np.uint8).reshape(n * h * w, -1)


def other_bytes(buf, n, c, h, w, planes):
    """Every byte of a PF buffer that belongs to no real pixel (guards, pad column / row, tile round-up), as one array."""
    px = np.asarray(buf, np.uint8).reshape(-1, c * BYTES_PER_CHANNEL[planes])
    mask = np.ones(px.shape[0], bool)
    mask[real_pixels(n, h, w)] = False
    return px[mask]


def to_lines(x, planes):
    """(n, c, h, w) values -> (n*h*w, lines, channels per line), the order `real_lines` uses."""
    n, c, h, w = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 3, 1)).reshape(n * h * w, c // CHANNELS[planes], CHANNELS[planes])


def from_lines(v, n, c, h, w):
    return np.ascontiguousarray(v.reshape(n, h, w, c).transpose(0, 3, 1, 2))


# ---------------------------------------------------------------------------------------------- crafted lines
def crafted_lines(planes):
    """(L, channels) float32: the edge-case lines the pack test plants among its random ones (L <= 32)."""
    nch = CHANNELS[planes]
    rng = np.random.default_rng(77)
    f = lambda *a: np.array(a, np.float32)
    L = []
    z = np.zeros(nch, np.float32)
    L.append(z.copy())                                                            # all zero
    v = z.copy(); v[13] = 0.3; L.append(v)                                        # one nonzero channel
    v = z.copy(); v[5] = -1.7e-3; L.append(v)
    v = rng.standard_normal(nch).astype(np.float32) * 100; v[0], v[9], v[31] = F16_MAX, -F16_MAX, F16_MAX; L.append(v)
    v = rng.standard_normal(nch).astype(np.float32); v[1], v[2], v[17], v[30] = 1e6, -1e6, np.inf, -np.inf; L.append(v)
    v = np.full(nch, 65520.0, np.float32); v[::2] = -65519.99; L.append(v)        # just past the clamp: fp16 would round to inf
    # hi block maximum with mantissa 0x780000 (1.9375 * 2^e): the last value below the scale's exponent bump ...
    v = (rng.uniform(-1, 1, nch) * 1.5).astype(np.float32).astype(np.float16).astype(np.float32); v[7] = -1.9375; L.append(v)
    v = v.copy(); v[7] = np.nextafter(np.float32(1.9375), np.float32(2)); L.append(v)    # input mantissa 0x780001: hi stays 0x780000
    v = v.copy(); v[7] = 1.9375 + 2.0 ** -10; L.append(v)                         # ... and the first fp16 above it (0x782000): bump
    v = (rng.uniform(-1, 1, nch) * 3e4).astype(np.float32); v[20] = 1.9375 * 2.0 ** 14; L.append(v)
    # lo block maximum with mantissa 0x780000 / 0x780001: hi = 1 (or 0), lo = x - hi
    v = np.ones(nch, np.float32) + (rng.integers(-20, 21, nch) * 2.0 ** -19).astype(np.float32); v[3] = 1 + 31 * 2.0 ** -19; L.append(v)
    v = (rng.integers(-8, 9, nch) * 0.125).astype(np.float32); v[11] = 1.9375 * 2.0 ** -27; L.append(v)           # |x| < 2^-25: hi = 0, lo = x
    v = v.copy(); v[11] = -np.nextafter(np.float32(1.9375 * 2.0 ** -27), np.float32(1)); L.append(v)      # 0x780001: bump
    # lo exactly halfway between two fp6 codes, both parities: hi = 1, scale_lo = 2^-14 (block maximum 7.25 * 2^-14)
    ties = f(0.0625, 0.1875, 0.3125, 0.9375, 1.0625, 1.9375, 2.125, 2.375, 3.875, 4.25, 4.75, 5.25, 7.25, -0.0625, -0.1875,
             -0.4375, -1.0625, -1.9375, -2.125, -2.375, -3.625, -3.875, 0.03125, -0.03125, 7.0, 6.0)
    v = np.ones(nch, np.float32); v[:ties.size] += ties * np.float32(2.0 ** -14); v[31] = 1 + 6 * 2.0 ** -14; L.append(v)
    v = (v - 1) * np.float32(2.0 ** -15); v[12] = 512.0; L.append(v)              # the same ties with hi = +-0 (|x| < 2^-25) beside a large hi block
    # hi in the fp16 subnormal range (below 2^-14), halfway cases of the fp16 rounding included
    v = (rng.standard_normal(nch) * 2.0 ** -17).astype(np.float32); v[4], v[5], v[6] = 2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -24; L.append(v)
    v = (rng.integers(-40, 41, nch) * 2.0 ** -24 + rng.integers(-1, 2, nch) * 2.0 ** -25).astype(np.float32); L.append(v)
    # lo in the fp16 subnormal range (planes 2: |x| < 2^-3), fp16 halfway cases of hi and of lo
    v = (rng.standard_normal(nch) * 2.0 ** -6).astype(np.float32); L.append(v)
    v = (1.0 + rng.integers(-3, 4, nch) * 2.0 ** -11 + rng.integers(-3, 4, nch) * 2.0 ** -25).astype(np.float32); L.append(v)
    v = (2.0 ** -5 * (1 + rng.integers(0, 1024, nch) * 2.0 ** -10) + rng.integers(-5, 6, nch) * 2.0 ** -25).astype(np.float32); L.append(v)
    out = np.stack(L)
    if planes == 1:                                                               # bf16 halfway cases, both parities
        v = (1.0 + rng.integers(0, 128, nch) * 2.0 ** -7 + rng.choice([-1, 1], nch) * 2.0 ** -8).astype(np.float32)
        out = np.concatenate([out, v[None], -v[None] * 2.0 ** 90])
    assert out.shape[0] <= 32 and not np.isnan(out).any()
    return out


def grid_values(rng, shape, k):
    """Random multiples of 2^-14 with |value| < 4 (zeros and both signs included), times 2^k, as float32: the exact-sum inputs of
    the conv epilogue test."""
    v = rng.integers(-(1 << 16) + 1, 1 << 16, shape).astype(np.float64)
    v[rng.random(shape) < 0.05] = 0.0
    return (v * 2.0 ** (k - 14)).astype(np.float32)
