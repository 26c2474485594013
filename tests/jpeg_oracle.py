"""The specification of the JPEG path (csrc/jpeg_dev.h, csrc/jpeg_walk.h, csrc/jpeg.hip): libjpeg's default decode of baseline
JPEG restated in NumPy integers - marker parse, Huffman decode, dequantise, jidctint's islow IDCT (CONST_BITS 13, PASS1_BITS 2),
jdsample's "fancy" h2v1 / h2v2 upsampling clamped at the component's real edges, jdcolor's 16-bit fixed-point YCbCr -> RGB.
tests/test_jpeg_cpu.py holds it against Pillow byte for byte; the GPU tests hold the kernels against it and against Pillow.

The status codes are include/wsi_hip.h's WSI_JPEG_*."""
import struct

import numpy as np

OK, PROGRESSIVE, ARITHMETIC, PRECISION, COMPONENTS, SAMPLING, MULTISCAN, MALFORMED, TABLE_CAPACITY, EMPTY = range(10)
BAD_CODE, COEF_OVERRUN, SHORT, EXHAUSTED, EXCESS, RANGE, GEOMETRY = range(16, 23)
STATUS_NAMES = {0: 'ok', 1: 'progressive', 2: 'arithmetic', 3: 'precision', 4: 'components', 5: 'sampling', 6: 'multiscan', 7: 'malformed',
                8: 'table_capacity', 9: 'empty', 16: 'bad_code', 17: 'coef_overrun', 18: 'short', 19: 'exhausted', 20: 'excess', 21: 'range',
                22: 'geometry'}

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])


class Unsupported(ValueError):
    def __init__(self, status):
        ValueError.__init__(self, STATUS_NAMES.get(status, str(status)))
        self.status = status


def segments(stream):
    """[(marker, body offset, body length)] up to and including SOS / EOI; raises Unsupported(MALFORMED) on a broken segment."""
    if stream[:2] != b'\xff\xd8':
        raise Unsupported(MALFORMED)
    out, i, n = [], 2, len(stream)
    while True:
        if i >= n or stream[i] != 0xFF:
            raise Unsupported(MALFORMED)
        while i < n and stream[i] == 0xFF:
            i += 1
        if i >= n:
            raise Unsupported(MALFORMED)
        mk = stream[i]
        i += 1
        if mk == 0xD9:
            out.append((mk, i, 0))
            return out
        if mk in (0, 1) or 0xD0 <= mk <= 0xD8 or i + 2 > n:
            raise Unsupported(MALFORMED)
        ln = struct.unpack('>H', stream[i:i + 2])[0]
        if ln < 2 or i + ln > n:
            raise Unsupported(MALFORMED)
        out.append((mk, i + 2, ln - 2))
        i += ln
        if mk == 0xDA:
            return out


def parse(stream, tables=None):
    """Header of one stream -> dict(width, height, ncomp, h, v, tq, td, ta, restart, scan_off, scan_len, qt {id: 64 zigzag values},
    huff {(class, id): (counts, symbols)}, own_tables, jfif, adobe, ids).  tables: the dict of a table blob (parse_tables)."""
    qt = dict(tables['qt']) if tables else {}
    huff = dict(tables['huff']) if tables else {}
    d = dict(qt=qt, huff=huff, restart=0, own_tables=False, jfif=False, adobe=None)
    sof = sos = False
    for mk, at, ln in segments(stream):
        body = stream[at:at + ln]
        if mk == 0xDB:
            j = 0
            while j < ln:
                prec, tid = body[j] >> 4, body[j] & 15
                j += 1
                if tid > 3 or prec > 1 or j + 64 * (prec + 1) > ln:
                    raise Unsupported(MALFORMED)
                qt[tid] = [int(v) for v in np.frombuffer(body[j:j + 64 * (prec + 1)], '>u2' if prec else 'u1')]
                j += 64 * (prec + 1)
            d['own_tables'] = True
        elif mk == 0xC4:
            j = 0
            while j < ln:
                cls, tid = body[j] >> 4, body[j] & 15
                counts = list(body[j + 1:j + 17])
                if cls > 1 or tid > 1 or len(counts) != 16 or j + 17 + sum(counts) > ln:
                    raise Unsupported(MALFORMED)
                huff[(cls, tid)] = (counts, list(body[j + 17:j + 17 + sum(counts)]))
                j += 17 + sum(counts)
            d['own_tables'] = True
        elif mk == 0xDD:
            d['restart'] = struct.unpack('>H', body)[0]
        elif mk == 0xE0 and body[:5] == b'JFIF\0':
            d['jfif'] = True
        elif mk == 0xEE and body[:5] == b'Adobe' and ln >= 12:
            d['adobe'] = body[11]
        elif 0xC0 <= mk <= 0xCF and mk not in (0xC4, 0xC8, 0xCC):
            if mk == 0xC2:
                raise Unsupported(PROGRESSIVE)
            if mk not in (0xC0, 0xC1):
                raise Unsupported(ARITHMETIC)
            prec, h, w, nc = struct.unpack('>BHHB', body[:6])
            if prec != 8:
                raise Unsupported(PRECISION)
            if nc not in (1, 3):
                raise Unsupported(COMPONENTS)
            comps = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(nc)]
            d.update(width=w, height=h, ncomp=nc, ids=[c[0] for c in comps], h=[c[1] for c in comps], v=[c[2] for c in comps],
                     tq=[c[3] for c in comps])
            if nc == 1:
                d['h'], d['v'] = [1], [1]
            elif (d['h'][0], d['v'][0]) not in ((1, 1), (2, 1), (2, 2)) or d['h'][1:] != [1, 1] or d['v'][1:] != [1, 1]:
                raise Unsupported(SAMPLING)
            sof = True
        elif mk == 0xDA:
            if not sof:
                raise Unsupported(MALFORMED)
            ns = body[0]
            if ns != d['ncomp']:
                raise Unsupported(MULTISCAN)
            d['td'] = [body[2 + 2 * c] >> 4 for c in range(ns)]
            d['ta'] = [body[2 + 2 * c] & 15 for c in range(ns)]
            if tuple(body[1 + 2 * ns:4 + 2 * ns]) != (0, 63, 0):
                raise Unsupported(MALFORMED)
            sos = True
            j = at + ln
            while True:
                j = stream.find(b'\xff', j)
                if j < 0 or j + 1 >= len(stream):
                    raise Unsupported(MALFORMED)
                if stream[j + 1] == 0 or 0xD0 <= stream[j + 1] <= 0xD7:
                    j += 2
                    continue
                break
            d['scan_off'], d['scan_len'] = at + ln, j - (at + ln)
            if stream[j + 1] != 0xD9:
                raise Unsupported(MULTISCAN)
    if not (sof and sos):
        raise Unsupported(MALFORMED)
    return d


def parse_tables(blob):
    qt, huff = {}, {}
    for mk, at, ln in segments(blob):
        if mk in (0xDB, 0xC4):
            d = parse(b'\xff\xd8' + b'\xff' + bytes([mk]) + struct.pack('>H', ln + 2) + blob[at:at + ln] + _NULL_FRAME)
            qt.update(d['qt'])
            huff.update(d['huff'])
    return dict(qt=qt, huff=huff)


# a minimal 1-component frame + scan, so that parse() can be reused for a lone table segment
_NULL_FRAME = (b'\xff\xc0' + struct.pack('>HBHHB', 11, 8, 8, 8, 1) + b'\x01\x11\x00' + b'\xff\xda' + struct.pack('>HB', 8, 1) + b'\x01\x00'
               + b'\x00\x3f\x00' + b'\xff\xd9')


def _code_table(counts, symbols):
    """{(length, code): symbol}"""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[(l, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return out


class _Bits:
    def __init__(self, data):
        # unstuff; a marker ends the segment (the caller splits at RSTn)
        self.bits = ''.join('{:08b}'.format(b) for b in data.replace(b'\xff\x00', b'\xff'))
        self.i = 0

    def get(self, n):
        if self.i + n > len(self.bits):
            raise Unsupported(EXHAUSTED)
        v = int(self.bits[self.i:self.i + n], 2) if n else 0
        self.i += n
        return v

    def symbol(self, table):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.get(1)
            if (l, code) in table:
                return table[(l, code)]
        raise Unsupported(BAD_CODE)


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def decode_coefficients(stream, tables=None):
    """(header dict, [per component (block rows, block cols, 64) int array]): dequantised coefficients in natural order."""
    d = parse(stream, tables)
    nc, hs, vs = d['ncomp'], d['h'][0], d['v'][0]
    mcux, mcuy = -(-d['width'] // (8 * hs)), -(-d['height'] // (8 * vs))
    coefs = [np.zeros((mcuy * d['v'][c], mcux * d['h'][c], 64), np.int64) for c in range(nc)]
    dc = [_code_table(*d['huff'][(0, d['td'][c])]) for c in range(nc)]
    ac = [_code_table(*d['huff'][(1, d['ta'][c])]) for c in range(nc)]
    q = [np.array(d['qt'][d['tq'][c]], np.int64) for c in range(nc)]
    data = stream[d['scan_off']:d['scan_off'] + d['scan_len']]
    intervals, j = [], 0
    if d['restart']:
        k = 0
        while True:
            m = data.find(bytes([0xFF, 0xD0 + (k & 7)]), j)
            # FF Dn can only be a marker: a data FF is followed by 00
            if m < 0:
                intervals.append(data[j:])
                break
            intervals.append(data[j:m])
            j, k = m + 2, k + 1
    else:
        intervals = [data]
    mcu = 0
    for seg in intervals:
        br, pred = _Bits(seg), [0] * nc
        for _ in range(d['restart'] or mcux * mcuy):
            if mcu >= mcux * mcuy:
                break
            my, mx = divmod(mcu, mcux)
            for c in range(nc):
                for by in range(d['v'][c]):
                    for bx in range(d['h'][c]):
                        blk = coefs[c][my * d['v'][c] + by, mx * d['h'][c] + bx]
                        s = br.symbol(dc[c])
                        pred[c] += _extend(br.get(s), s)
                        blk[0] = pred[c] * q[c][0]
                        k = 1
                        while k < 64:
                            rs = br.symbol(ac[c])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise Unsupported(COEF_OVERRUN)
                            blk[ZIGZAG[k]] = _extend(br.get(s), s) * q[c][k]
                            k += 1
            mcu += 1
    if mcu != mcux * mcuy:
        raise Unsupported(SHORT)
    return d, coefs


_F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
          f2_053=16819, f2_562=20995, f3_072=25172)


def _idct_1d(x, shift):
    """x: (..., 8) int64 -> (..., 8), one pass of jpeg_idct_islow descaled by `shift`"""
    F = _F
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * F['f0_541']
    tmp2 = z1 + z3 * -F['f1_847']
    tmp3 = z1 + z2 * F['f0_765']
    tmp0 = (x[..., 0] + x[..., 4]) << 13
    tmp1 = (x[..., 0] - x[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F['f1_175']
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F['f0_298'], tmp1 * F['f2_053'], tmp2 * F['f3_072'], tmp3 * F['f1_501']
    z1, z2, z3, z4 = z1 * -F['f0_899'], z2 * -F['f2_562'], z3 * -F['f1_961'] + z5, z4 * -F['f0_390'] + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([(tmp10 + tmp3 + r) >> shift, (tmp11 + tmp2 + r) >> shift, (tmp12 + tmp1 + r) >> shift, (tmp13 + tmp0 + r) >> shift,
                     (tmp13 - tmp0 + r) >> shift, (tmp12 - tmp1 + r) >> shift, (tmp11 - tmp2 + r) >> shift, (tmp10 - tmp3 + r) >> shift], -1)


def idct_islow(blocks):
    """(..., 64) dequantised coefficients -> (..., 8, 8) samples 0..255"""
    m = np.asarray(blocks, np.int64).reshape(blocks.shape[:-1] + (8, 8))
    m = np.swapaxes(_idct_1d(np.swapaxes(m, -1, -2), 11), -1, -2)          # pass 1: columns
    m = _idct_1d(m, 18)                                                      # pass 2: rows
    v = m & 1023                                                             # range_limit[x & RANGE_MASK]
    v = np.where(v < 512, v, v - 1024) + 128
    return np.clip(v, 0, 255)


def planes_of(d, coefs):
    """the component planes over whole MCUs"""
    out = []
    for c in range(d['ncomp']):
        s = idct_islow(coefs[c])                                             # (bh, bw, 8, 8)
        out.append(s.transpose(0, 2, 1, 3).reshape(s.shape[0] * 8, s.shape[1] * 8))
    return out


def upsample_fancy(p, hs, vs, width, height):
    """chroma plane -> (height, width): jdsample.c's h2v1 / h2v2 fancy upsampling over the component's real samples
    (ceil(width / hs) x ceil(height / vs)); replication where libjpeg falls back to it (at most 2 real columns)."""
    cw, ch = -(-width // hs), -(-height // vs)
    p = p[:ch, :cw].astype(np.int64)
    if hs == 1:
        return p[:height, :width]
    if cw <= 2:
        return np.repeat(np.repeat(p, vs, 0), 2, 1)[:height, :width]
    if vs == 1:
        out = np.zeros((ch, 2 * cw), np.int64)
        out[:, 0] = p[:, 0]
        out[:, 2::2] = (3 * p[:, 1:] + p[:, :-1] + 1) >> 2
        out[:, 1:-1:2] = (3 * p[:, :-1] + p[:, 1:] + 2) >> 2
        out[:, -1] = p[:, -1]
        return out[:height, :width]
    up = np.concatenate([p[:1], p[:-1]], 0)                                  # the row above, the first row repeated
    dn = np.concatenate([p[1:], p[-1:]], 0)
    out = np.zeros((2 * ch, 2 * cw), np.int64)
    for v, far in ((0, up), (1, dn)):
        cs = 3 * p + far
        o = out[v::2]
        o[:, 0] = (cs[:, 0] * 4 + 8) >> 4
        o[:, 2::2] = (cs[:, 1:] * 3 + cs[:, :-1] + 8) >> 4
        o[:, 1:-1:2] = (cs[:, :-1] * 3 + cs[:, 1:] + 7) >> 4
        o[:, -1] = (cs[:, -1] * 4 + 7) >> 4
    return out[:height, :width]


def ycc_to_rgb(y, cb, cr):
    """jdcolor.c: 16 fractional bits"""
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def libjpeg_transform(d):
    """libjpeg's own choice for a stand-alone stream (jdapimin.c default_decompress_parms)"""
    if d['ncomp'] != 3:
        return False
    if d['jfif']:
        return True
    if d['adobe'] is not None:
        return d['adobe'] != 0
    return d['ids'] != [ord('R'), ord('G'), ord('B')]


def decode(stream, tables=None, transform=None):
    """(height, width, 3) u8.  transform: True YCbCr -> RGB, False none (TIFF PhotometricInterpretation 6 / 2), None: libjpeg's rule
    for a stand-alone stream."""
    d, coefs = decode_coefficients(stream, tables)
    planes = planes_of(d, coefs)
    w, h = d['width'], d['height']
    y = planes[0][:h, :w].astype(np.int64)
    if d['ncomp'] == 1:
        return np.repeat(y[..., None], 3, -1).astype(np.uint8)
    c1 = upsample_fancy(planes[1], d['h'][0], d['v'][0], w, h)
    c2 = upsample_fancy(planes[2], d['h'][0], d['v'][0], w, h)
    if libjpeg_transform(d) if transform is None else transform:
        return ycc_to_rgb(y, c1, c2)
    return np.stack([y, c1, c2], -1).astype(np.uint8)
