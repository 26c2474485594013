"""Test fixtures of the JPEG path, made at test time: tile streams encoded by Pillow and tiled JPEG pyramids written by hand with
`struct` - classic TIFF or BigTIFF, either byte order, with or without a JPEGTables tag (Pillow's streamtype 1 = tables only,
2 = abbreviated), PhotometricInterpretation 6 (YCbCr) or 2 (RGB), optionally with the APP0 / APP14 markers stripped from the tile
streams, 0-byte tiles, progressive tiles and an uncompressed stripped directory (an SVS thumbnail) between the levels."""
import io
import struct

import numpy as np
from PIL import Image


def noise(h, w, seed, channels=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, channels) if channels > 1 else (h, w), dtype=np.uint8)


def he_like(h, w, seed, channels=3):
    """smooth pink / purple fields with blobs and a little noise; white background on the right edge"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    f = 0.5 + 0.5 * np.sin(xx / 9.0 + rng.uniform(0, 6)) * np.cos(yy / 7.0 + rng.uniform(0, 6))
    g = 0.5 + 0.5 * np.sin((xx + yy) / 13.0 + rng.uniform(0, 6))
    img = np.stack([235 - 90 * f - 20 * g, 170 - 110 * f + 30 * g, 215 - 60 * f - 25 * g], -1) + rng.normal(0, 5, (h, w, 3))
    img[:, w - max(1, w // 8):] = 243
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img if channels == 3 else img[..., 1]


def strip_app_markers(stream):
    """the stream without its APP0 (JFIF) and APP14 (Adobe) segments"""
    out, i = [stream[:2]], 2
    while stream[i] == 0xFF and stream[i + 1] != 0xDA:
        ln = struct.unpack('>H', stream[i + 2:i + 4])[0]
        if stream[i + 1] not in (0xE0, 0xEE):
            out.append(stream[i:i + 2 + ln])
        i += 2 + ln
    out.append(stream[i:])
    return b''.join(out)


def encode(arr, quality=75, subsampling=0, restart=0, rgb=False, streamtype=0, progressive=False, strip=False, optimize=False):
    """one JPEG stream of a (h, w, 3) or (h, w) u8 array.  rgb: the three planes are stored untransformed (Adobe transform 0).
    optimize: Huffman tables made for this image (libjpeg's optimize_coding) instead of the standard ones."""
    kw = dict(quality=quality, streamtype=streamtype)
    if arr.ndim == 3:
        kw['subsampling'] = subsampling
        if rgb:
            kw['keep_rgb'] = True
    if restart:
        kw['restart_marker_blocks'] = restart
    if progressive:
        kw['progressive'] = True
    if optimize:
        kw['optimize'] = True
    b = io.BytesIO()
    Image.fromarray(arr).save(b, 'JPEG', **kw)
    s = b.getvalue()
    return strip_app_markers(s) if strip and streamtype != 1 else s


def pad_to_tiles(level, tw, th):
    h, w = level.shape[:2]
    ph, pw = -(-h // th) * th, -(-w // tw) * tw
    return np.pad(level, ((0, ph - h), (0, pw - w)) + ((0, 0),) * (level.ndim - 2), mode='edge')


def pyramid(h, w, levels=3, seed=0, content=he_like):
    """levels of (h, w) / 2^k, each content of its own (nothing downstream needs them to be downsamples of each other)"""
    return [content(max(1, h >> k), max(1, w >> k), seed + k) for k in range(levels)]


def write_tiff(path, levels, tile=(64, 48), big=False, endian='<', jpegtables=True, photometric=6, quality=75, subsampling=2, restart=0,
               strip=False, empty=(), progressive=(), thumbnail=False, compression=7, optimize=False):
    """Write the pyramid; returns dict(streams=[per level [tile stream]], tables=[per level blob or None], frames=[Pillow frame index
    of each level]).  tile = (tile_w, tile_h); empty / progressive: sets of (level, tile index) written with byte count 0 / as a
    complete progressive stream; optimize: every tile stream carries Huffman tables of its own (use with jpegtables=False)."""
    tw, th = tile
    e = endian
    assert not (optimize and jpegtables), 'abbreviated streams carry no tables: optimised ones go with jpegtables=False'
    rgb = photometric == 2
    if rgb:
        subsampling = 0                                          # Pillow stores untransformed RGB at full resolution only
    off_t = 'Q' if big else 'I'
    out = bytearray()
    out += (b'II' if e == '<' else b'MM') + (struct.pack(e + 'HHHQ', 43, 8, 0, 0) if big else struct.pack(e + 'HI', 42, 0))
    first_ptr = 8 if big else 4                                  # where the first IFD's offset goes
    info = dict(streams=[], tables=[], frames=[])
    dirs = []                                                    # (entries, ) per IFD: [(tag, type, count, packed bytes)]

    def pack(fmt, *v):
        return struct.pack(e + fmt, *v)

    def blob(data):
        if len(out) & 1:
            out.append(0)
        at = len(out)
        out.extend(data)
        return at

    frame = 0
    for k, lv in enumerate(levels):
        h, w = lv.shape[:2]
        samples = 1 if lv.ndim == 2 else 3
        padded = pad_to_tiles(lv, tw, th)
        cols, rows = padded.shape[1] // tw, padded.shape[0] // th
        tables = encode(padded[:th, :tw], quality, subsampling, 0, rgb, 1) if jpegtables else None
        offs, cnts, streams = [], [], []
        for ty in range(rows):
            for tx in range(cols):
                idx = ty * cols + tx
                t = np.ascontiguousarray(padded[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw])
                if (k, idx) in empty:
                    s = b''
                elif (k, idx) in progressive:
                    s = encode(t, quality, subsampling, 0, rgb, 0, True, strip)
                else:
                    s = encode(t, quality, subsampling, restart, rgb, 2 if jpegtables else 0, False, strip, optimize)
                streams.append(s)
                offs.append(blob(s) if s else 0)
                cnts.append(len(s))
        info['streams'].append(streams)
        info['tables'].append(tables)
        info['frames'].append(frame)
        frame += 1
        n = len(offs)
        ent = [(256, 4, 1, pack('I', w)), (257, 4, 1, pack('I', h)), (258, 3, samples, pack('H' * samples, *([8] * samples))),
               (259, 3, 1, pack('H', compression)), (262, 3, 1, pack('H', (photometric if samples == 3 else 1))), (277, 3, 1, pack('H', samples)),
               (284, 3, 1, pack('H', 1)), (322, 4, 1, pack('I', tw)), (323, 4, 1, pack('I', th)),
               (324, 16 if big else 4, n, pack(off_t * n, *offs)), (325, 4, n, pack('I' * n, *cnts))]
        if tables:
            ent.append((347, 7, len(tables), tables))
        if samples == 3 and photometric == 6:
            ent.append((530, 3, 2, pack('HH', (1, 2, 2)[subsampling], (1, 1, 2)[subsampling])))
        dirs.append(ent)
        if thumbnail and k == 0:                                 # a stripped, uncompressed RGB image, as an SVS thumbnail is stripped
            th_img = np.ascontiguousarray(lv[::4, ::4] if lv.ndim == 3 else np.repeat(lv[::4, ::4, None], 3, 2))
            at = blob(th_img.tobytes())
            dirs.append([(256, 4, 1, pack('I', th_img.shape[1])), (257, 4, 1, pack('I', th_img.shape[0])), (258, 3, 3, pack('HHH', 8, 8, 8)),
                         (259, 3, 1, pack('H', 1)), (262, 3, 1, pack('H', 2)), (273, 16 if big else 4, 1, pack(off_t, at)), (277, 3, 1, pack('H', 3)),
                         (278, 4, 1, pack('I', th_img.shape[0])), (279, 4, 1, pack('I', th_img.nbytes)), (284, 3, 1, pack('H', 1))])
            frame += 1
    inline = 8 if big else 4
    ptr_at = first_ptr
    for ent in dirs:
        ent = sorted(ent, key=lambda t: t[0])
        fields = []
        for tag, typ, cnt, data in ent:
            if len(data) <= inline:
                val = bytes(data) + b'\0' * (inline - len(data))
            else:
                val = pack(off_t, blob(data))
            fields.append(pack('HH', tag, typ) + pack(off_t, cnt) + val)
        at = blob(b'')
        struct.pack_into(e + off_t, out, ptr_at, at)
        out += pack('Q' if big else 'H', len(fields)) + b''.join(fields)
        ptr_at = len(out)
        out += pack(off_t, 0)
    with open(path, 'wb') as f:
        f.write(out)
    return info


def pillow_levels(path, frames):
    """every level as Pillow's libtiff reads it: [(H, W, 3) u8]"""
    out = []
    with Image.open(path) as im:
        for k in frames:
            im.seek(k)
            out.append(np.asarray(im.convert('RGB')).copy())
    return out


# ------------------------------------------------------------------------------------------ streams made to fail in the decode loop
def _stuffed(bits):
    """a bit string, padded with ones to whole bytes, as scan data (FF -> FF 00)"""
    bits = bits + '1' * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b'\xff', b'\xff\x00')


def _scan_start(stream):
    i = 2
    while stream[i + 1] != 0xDA:
        i += 2 + struct.unpack('>H', stream[i + 2:i + 4])[0]
    return i + 2 + struct.unpack('>H', stream[i + 2:i + 4])[0]


def _code_of(stream, cls, symbol):
    """the bit string of `symbol` in the stream's Huffman table 0 of class cls (0 DC, 1 AC)"""
    import jpeg_oracle as O
    for (length, code), sym in O._code_table(*O.parse(stream)['huff'][(cls, 0)]).items():
        if sym == symbol:
            return format(code, '0%db' % length)
    raise KeyError(symbol)


def bad_scan_streams(subsampling=None):
    """{name: (stream, status)}: complete 16 x 16 greyscale streams (Pillow's header, the standard Huffman tables) that pass the marker
    walk and end the decode loop with the WSI_JPEG_* status given.  subsampling 0 / 1 / 2: three-component streams of that sub-sampling
    instead, for a colour batch - the first three only, which are damaged in the first luma block and do not depend on the MCU layout.
      exhausted   : the scan cut in the middle, EOI put back behind it
      bad_code    : sixteen 1-bits where a DC code is due (the standard DC table has no code of all ones)
      coef_overrun: DC category 0, three ZRL (coefficient 49), then run 15 / size 1: the run passes coefficient 63
      short       : restart markers after every MCU, the DRI segment patched to promise two MCUs per interval
      zrl_end     : status 0 - four blocks of DC category 0 and four ZRL each: the fourth ZRL passes coefficient 63 and ends the block, as
                    in libjpeg; every coefficient is zero"""
    colour = subsampling is not None
    g16 = encode(noise(16, 16, 6, 3), 75, subsampling) if colour else encode(noise(16, 16, 6, 1), 75)
    g16r = encode(noise(16, 16, 7, 1), 75, restart=1)
    s16 = _scan_start(g16)
    dc0, zrl, f1 = _code_of(g16, 0, 0), _code_of(g16, 1, 0xF0), _code_of(g16, 1, 0xF1)
    out = {}
    body = g16[s16:-2]
    out['exhausted'] = (g16[:s16] + body[:len(body) // 2].rstrip(b'\xff') + b'\xff\xd9', 19)
    out['bad_code'] = (g16[:s16] + b'\xff\x00\xff\x00' + b'\xff\xd9', 16)
    out['coef_overrun'] = (g16[:s16] + _stuffed(dc0 + zrl * 3 + f1 + '1') + b'\xff\xd9', 17)
    if colour:
        return out
    at = g16r.index(b'\xff\xdd\x00\x04')
    assert g16r[at + 4:at + 6] == b'\x00\x01'
    out['short'] = (g16r[:at + 4] + b'\x00\x02' + g16r[at + 6:], 18)
    out['zrl_end'] = (g16[:s16] + _stuffed((dc0 + zrl * 4) * 4) + b'\xff\xd9', 0)
    return out
