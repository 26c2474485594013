"""The specification of the JPEG encode path (csrc/jpeg_enc_dev.h, csrc/jpeg_enc.hip, tiffwrite.py): libjpeg's default encode of
baseline JPEG restated in NumPy integers - jccolor's 16-bit fixed-point RGB -> YCbCr, jcsample's h2v1 / h2v2 box downsampling with
the alternating bias, jfdctint's islow FDCT (CONST_BITS 13, PASS1_BITS 2), jcdctmgr's quantisation, jchuff with the standard
(Annex K) Huffman tables, restart intervals.  tests/test_jpeg_enc_cpu.py holds it against Pillow byte for byte (quantised
coefficients and scan bytes); the GPU tests hold the kernels against it and against Pillow.

A tile is (h, w, 3) or (h, w) u8 with h and w multiples of 16, so every MCU is whole and libjpeg's edge handling never shows."""
import numpy as np

from jpeg_oracle import ZIGZAG, _F

SAMPLINGS = ((1, 1), (2, 1), (2, 2))                             # luma (hs, vs); Pillow's subsampling 0, 1, 2

# Annex K: the base quantisation tables, natural (row-major) order
STD_LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                       80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                       95, 98, 112, 100, 103, 99])
STD_CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99]
                        + [99] * 36)

# Annex K: (code counts of length 1..16, symbols) of DC luma, DC chroma, AC luma, AC chroma
STD_HUFF = (
    ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
     [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98,
      114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86,
      87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138,
      146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
      194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233,
      234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250]),
    ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
     [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114,
      209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85,
      86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136,
      137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184,
      185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232,
      233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250]),
)


def quality_tables(quality):
    """(luma, chroma) quantisation tables in natural order: jpeg_quality_scaling of the Annex K tables, force_baseline"""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t.astype(np.int64) * scale + 50) // 100, 1, 255) for t in (STD_LUMA_Q, STD_CHROMA_Q))


def encode_tables():
    """[{symbol: (code, length)}] of the four standard tables (DC luma, DC chroma, AC luma, AC chroma)"""
    out = []
    for counts, symbols in STD_HUFF:
        tab, code, k = {}, 0, 0
        for l in range(1, 17):
            for _ in range(counts[l - 1]):
                tab[symbols[k]] = (code, l)
                code += 1
                k += 1
            code <<= 1
        out.append(tab)
    return out


def rgb_to_ycc(rgb):
    """jccolor.c: 16 fractional bits -> (Y, Cb, Cr) int64 planes"""
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def downsample(p, hs, vs):
    """jcsample.c h2v1_downsample / h2v2_downsample: the bias alternates along the output row (0, 1, ... / 1, 2, ...)"""
    if hs == 1:
        return p
    x = np.arange(p.shape[1] // 2)
    if vs == 1:
        return (p[:, 0::2] + p[:, 1::2] + (x & 1)) >> 1
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + (x & 1)) >> 2


def _fdct_1d(d, first):
    """d: (..., 8) int64 -> (..., 8), one pass of jpeg_fdct_islow (first: the row pass)"""
    F = _F
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 11 if first else 15
    r = 1 << (sh - 1)
    o0, o4 = ((t10 + t11) << 2, (t10 - t11) << 2) if first else ((t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2)
    z1 = (t12 + t13) * F['f0_541']
    o2 = (z1 + t13 * F['f0_765'] + r) >> sh
    o6 = (z1 - t12 * F['f1_847'] + r) >> sh
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F['f1_175']
    t4, t5, t6, t7 = t4 * F['f0_298'], t5 * F['f2_053'], t6 * F['f3_072'], t7 * F['f1_501']
    z1, z2, z3, z4 = z1 * -F['f0_899'], z2 * -F['f2_562'], z3 * -F['f1_961'] + z5, z4 * -F['f0_390'] + z5
    o7, o5, o3, o1 = (t4 + z1 + z3 + r) >> sh, (t5 + z2 + z4 + r) >> sh, (t6 + z2 + z3 + r) >> sh, (t7 + z1 + z4 + r) >> sh
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], -1)


def fdct_islow(blocks):
    """(..., 8, 8) samples 0..255 -> (..., 8, 8): 8 x the DCT of (sample - 128)"""
    m = _fdct_1d(np.asarray(blocks, np.int64) - 128, True)
    return np.swapaxes(_fdct_1d(np.swapaxes(m, -1, -2), False), -1, -2)


def quantise(coef, q):
    """jcdctmgr.c: coef (..., 64) natural order, q (64,) natural order; round half away from zero over the divisor 8 q"""
    d = 8 * np.asarray(q, np.int64)
    return np.sign(coef) * ((np.abs(coef) + (d >> 1)) // d)


def coefficients(tile, qtables, sampling=(2, 2)):
    """[per component (block rows, block cols, 64)]: quantised coefficients in natural order.  qtables: (luma, chroma), natural order."""
    tile = np.asarray(tile)
    h, w = tile.shape[:2]
    assert h % 16 == 0 and w % 16 == 0 and tile.dtype == np.uint8
    if tile.ndim == 2:
        planes, tq = [tile.astype(np.int64)], [0]
    else:
        y, cb, cr = rgb_to_ycc(tile)
        planes, tq = [y, downsample(cb, *sampling), downsample(cr, *sampling)], [0, 1, 1]
    out = []
    for p, t in zip(planes, tq):
        b = p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)
        out.append(quantise(fdct_islow(b).reshape(b.shape[0], b.shape[1], 64), qtables[t]))
    return out


def mcu_order(coefs, sampling=(2, 2)):
    """the coefficients as the entropy stage consumes them: (MCUs, blocks per MCU, 64) int16, MCU by MCU, component by component
    (a luma MCU's blocks row by row), zigzag"""
    hs, vs = sampling if len(coefs) == 3 else (1, 1)
    mcuy, mcux = coefs[0].shape[0] // vs, coefs[0].shape[1] // hs
    parts = [coefs[0].reshape(mcuy, vs, mcux, hs, 64).transpose(0, 2, 1, 3, 4).reshape(mcuy * mcux, vs * hs, 64)]
    parts += [c.reshape(mcuy * mcux, 1, 64) for c in coefs[1:]]
    return np.concatenate(parts, 1)[..., ZIGZAG].astype(np.int16)


class _Bits:
    """jchuff.c's bit buffer: MSB first, every 0xFF byte followed by 0x00"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, size):
        self.acc = (self.acc << size) | code
        self.n += size
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def scan_bytes(mcus, ncomp, sampling=(2, 2), restart=0):
    """The entropy-coded scan of (MCUs, blocks per MCU, 64) zigzag coefficients: standard tables, `restart` MCUs per interval (0: none)."""
    tabs = encode_tables()
    hs, vs = sampling if ncomp == 3 else (1, 1)
    comp_of = [0] * (hs * vs) + [1, 2][:ncomp - 1]
    br, pred, rst = _Bits(), [0, 0, 0], 0
    for m, mcu in enumerate(np.asarray(mcus, np.int64)):
        if restart and m and m % restart == 0:
            br.flush()
            br.out += bytes([0xFF, 0xD0 + rst])
            rst, pred = (rst + 1) & 7, [0, 0, 0]
        for blk, c in zip(mcu, comp_of):
            dc, ac = tabs[min(c, 1)], tabs[2 + min(c, 1)]
            diff = int(blk[0]) - pred[c]
            pred[c] = int(blk[0])
            s = abs(diff).bit_length()
            br.put(*dc[s])
            if s:
                br.put((diff if diff >= 0 else diff - 1 + (1 << s)), s)
            run = 0
            for k in range(1, 64):
                v = int(blk[k])
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    br.put(*ac[0xF0])
                    run -= 16
                s = abs(v).bit_length()
                br.put(*ac[(run << 4) | s])
                br.put((v if v >= 0 else v - 1 + (1 << s)), s)
                run = 0
            if run:
                br.put(*ac[0])
    br.flush()
    return bytes(br.out)


def encode_tile(tile, qtables, sampling=(2, 2), restart=0):
    """(quantised coefficients per component, natural order; scan bytes) of one tile"""
    tile = np.asarray(tile)
    coefs = coefficients(tile, qtables, sampling)
    return coefs, scan_bytes(mcu_order(coefs, sampling), len(coefs), sampling, restart)
