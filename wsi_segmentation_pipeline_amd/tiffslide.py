"""JPEG-tiled TIFF / SVS pyramids without OpenSlide (reference utils/dataset.py:171-185 reads every patch through OpenSlide).

`TiffSlide(path)` is pure Python over `mmap` + `struct` and has the slide surface the drivers use: level_count, level_dimensions,
level_downsamples, dimensions, name, read_region, device_level, close.  Classic TIFF and BigTIFF, both byte orders.  The pyramid
levels are the TILED IFDs in file order (stripped IFDs - an SVS thumbnail, label, macro - are skipped); compression 7 (JPEG), 8 bit,
1 or 3 samples, chunky.  Tile streams may be abbreviated (tables in tag 347 JPEGTables) or complete.  The colour transform follows
tag 262 as libtiff does - 6: YCbCr -> RGB, 2: none - whatever markers the streams carry.  A tile of byte count 0 is white.

read_region is the host path (Pillow decodes the tiles it touches); device_level goes through the GPU decode
(ingest.level_from_tiff, csrc/jpeg.hip)."""
import collections
import io
import mmap
import os
import struct
import threading

import numpy as np

# every TIFF 6.0 / BigTIFF field type has a size, so that a directory can be walked; rationals and floats (5, 10, 11, 12) are not decoded:
# no tag this reader uses has them
_TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 16: 8, 17: 8, 18: 8}
_TYPE_FMT = {1: 'B', 2: 'c', 3: 'H', 4: 'I', 6: 'b', 7: 'B', 8: 'h', 9: 'i', 16: 'Q', 17: 'q', 18: 'Q'}
T_WIDTH, T_LENGTH, T_BITS, T_COMPRESSION, T_PHOTOMETRIC, T_SAMPLES, T_PLANAR = 256, 257, 258, 259, 262, 277, 284
T_TILE_W, T_TILE_L, T_TILE_OFF, T_TILE_CNT, T_JPEGTABLES = 322, 323, 324, 325, 347


class TiffLevel:
    """One tiled IFD: geometry, the tile offsets / byte counts, the JPEGTables blob (or None), the photometric tag."""

    def __init__(self, width, height, tile_w, tile_h, samples, photometric, offsets, counts, tables):
        self.width, self.height, self.tile_w, self.tile_h = width, height, tile_w, tile_h
        self.samples, self.photometric, self.tables = samples, photometric, tables
        self.offsets, self.counts = np.asarray(offsets, np.uint64), np.asarray(counts, np.uint64)
        self.cols, self.rows = -(-width // tile_w), -(-height // tile_h)
        self.transform = 1 if photometric == 6 else 0


def _read_ifds(buf):
    """[{tag: tuple of values}] of every IFD in file order"""
    if len(buf) < 8 or buf[:2] not in (b'II', b'MM'):
        raise ValueError('not a TIFF file: byte-order mark %r' % (bytes(buf[:2]),))
    e = '<' if buf[:2] == b'II' else '>'
    magic = struct.unpack(e + 'H', buf[2:4])[0]
    if magic == 42:
        big, off = False, struct.unpack(e + 'I', buf[4:8])[0]
    elif magic == 43:
        big, off = True, struct.unpack(e + 'Q', buf[8:16])[0]
    else:
        raise ValueError('not a TIFF file: magic %d' % magic)
    ifds, seen = [], set()
    while off and off not in seen:
        seen.add(off)
        if big:
            n = struct.unpack(e + 'Q', buf[off:off + 8])[0]
            at, esz, inline = off + 8, 20, 8
        else:
            n = struct.unpack(e + 'H', buf[off:off + 2])[0]
            at, esz, inline = off + 2, 12, 4
        tags = {}
        for k in range(n):
            ent = buf[at + k * esz:at + (k + 1) * esz]
            if len(ent) < esz:
                raise ValueError('truncated TIFF directory at %d' % off)
            tag, typ = struct.unpack(e + 'HH', ent[:4])
            cnt = struct.unpack(e + ('Q' if big else 'I'), ent[4:4 + inline])[0]
            size = _TYPE_SIZE.get(typ)
            if size is None:
                continue
            if size * cnt <= inline:
                raw = ent[4 + inline:4 + inline + size * cnt]
            else:
                p = struct.unpack(e + ('Q' if big else 'I'), ent[4 + inline:4 + 2 * inline])[0]
                raw = buf[p:p + size * cnt]
                if len(raw) < size * cnt:
                    raise ValueError('TIFF tag %d points outside the file' % tag)
            if typ in (1, 7):
                tags[tag] = bytes(raw)
            elif typ in _TYPE_FMT:
                dt = np.dtype(e + {'B': 'u1', 'c': 'S1', 'H': 'u2', 'I': 'u4', 'b': 'i1', 'h': 'i2', 'i': 'i4', 'Q': 'u8', 'q': 'i8'}[_TYPE_FMT[typ]])
                tags[tag] = np.frombuffer(raw, dt)
        ifds.append(tags)
        nxt = at + n * esz
        off = struct.unpack(e + ('Q' if big else 'I'), buf[nxt:nxt + (8 if big else 4)])[0]
    return ifds


def _scalar(tags, tag, default=None):
    v = tags.get(tag)
    if v is None:
        return default
    return int(v[0])


class TiffSlide:
    def __init__(self, path, cache_tiles=64):
        self.path = str(path)
        self.name = os.path.basename(self.path)
        self._f = open(self.path, 'rb')
        self._map = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)
        try:
            self.levels = self._levels(_read_ifds(self._map))
        except Exception:
            self.close()
            raise
        if not self.levels:
            self.close()
            raise ValueError('%s holds no tiled image (tag 322 TileWidth missing in every directory)' % self.path)
        self.level_count = len(self.levels)
        self.level_dimensions = tuple((l.width, l.height) for l in self.levels)
        self.dimensions = self.level_dimensions[0]
        w0, h0 = self.dimensions
        self.level_downsamples = tuple((w0 / l.width + h0 / l.height) / 2.0 for l in self.levels)      # OpenSlide's rule
        self.decode_report = {}                                 # level -> {status name: tiles}, filled by device_level
        self._cache = collections.OrderedDict()
        self._cache_tiles = int(cache_tiles)
        self._lock = threading.Lock()                           # read_region is called from the ingestion ring's decoder threads
        self._dev = {}

    @staticmethod
    def _levels(ifds):
        out = []
        for tags in ifds:
            if T_TILE_W not in tags:
                continue                                        # stripped: thumbnail, label, macro
            for tag, ok, what in ((T_COMPRESSION, (7,), 'Compression'), (T_PLANAR, (1,), 'PlanarConfiguration'),
                                  (T_SAMPLES, (1, 3), 'SamplesPerPixel')):
                v = _scalar(tags, tag, 1)
                if v not in ok:
                    raise ValueError('unsupported TIFF: tag %d %s = %d (supported: %s)' % (tag, what, v, ', '.join(map(str, ok))))
            bits = tags.get(T_BITS)
            if bits is not None and any(int(b) != 8 for b in bits):
                raise ValueError('unsupported TIFF: tag %d BitsPerSample = %s (supported: 8)' % (T_BITS, list(map(int, bits))))
            samples = _scalar(tags, T_SAMPLES, 1)
            photometric = _scalar(tags, T_PHOTOMETRIC, 1 if samples == 1 else 2)
            if photometric not in ((0, 1) if samples == 1 else (2, 6)):
                raise ValueError('unsupported TIFF: tag %d PhotometricInterpretation = %d with %d samples' % (T_PHOTOMETRIC, photometric, samples))
            if T_TILE_OFF not in tags or T_TILE_CNT not in tags:
                raise ValueError('unsupported TIFF: tag %d TileOffsets or tag %d TileByteCounts missing' % (T_TILE_OFF, T_TILE_CNT))
            lv = TiffLevel(_scalar(tags, T_WIDTH), _scalar(tags, T_LENGTH), _scalar(tags, T_TILE_W), _scalar(tags, T_TILE_L), samples,
                           photometric, tags[T_TILE_OFF], tags[T_TILE_CNT], tags.get(T_JPEGTABLES))
            if min(lv.width, lv.height, lv.tile_w, lv.tile_h) <= 0 or len(lv.offsets) != lv.cols * lv.rows or len(lv.counts) != len(lv.offsets):
                raise ValueError('unsupported TIFF: %d tile offsets for a %d x %d grid' % (len(lv.offsets), lv.cols, lv.rows))
            out.append(lv)
        return out

    # ------------------------------------------------------------------------------------------------------------------ host path
    def tile_bytes(self, level, index):
        """the compressed stream of one tile (b'' for byte count 0)"""
        lv = self.levels[level]
        off, cnt = int(lv.offsets[index]), int(lv.counts[index])
        if off + cnt > len(self._map):
            raise ValueError('level %d tile %d lies outside the file' % (level, index))
        return self._map[off:off + cnt]

    def tile_stream(self, level, index):
        """a complete JPEG stream of one tile: the JPEGTables segments spliced in behind the tile's SOI"""
        lv = self.levels[level]
        data = self.tile_bytes(level, index)
        if lv.tables and len(lv.tables) > 4 and data[:2] == b'\xff\xd8':
            return data[:2] + lv.tables[2:-2] + data[2:]
        return data

    def decode_tile_host(self, level, index):
        """(tile_h, tile_w, 3) u8 through Pillow; the colour transform is the level's photometric tag, as libtiff sets it"""
        from PIL import Image
        lv = self.levels[level]
        data = self.tile_stream(level, index)
        if len(data) == 0:
            return np.full((lv.tile_h, lv.tile_w, 3), 255, np.uint8)
        try:
            im = Image.open(io.BytesIO(data))
            if im.mode == 'L':
                arr = np.array(im.convert('RGB'))
            else:
                # libjpeg's own choice would follow the JFIF / Adobe markers: restate the tag's transform in the stream
                arr = _decode_with_transform(data, lv.transform)
        except Exception as e:
            raise ValueError('level %d tile %d cannot be decoded: %s' % (level, index, e)) from e
        if arr.shape[0] < lv.tile_h or arr.shape[1] < lv.tile_w:
            raise ValueError('level %d tile %d is %d x %d, smaller than the %d x %d tile grid' % (level, index, arr.shape[1], arr.shape[0], lv.tile_w, lv.tile_h))
        return arr[:lv.tile_h, :lv.tile_w]

    def _tile(self, level, index):
        key = (level, index)
        with self._lock:
            t = self._cache.get(key)
            if t is not None:
                self._cache.move_to_end(key)
                return t
        t = self.decode_tile_host(level, index)                 # outside the lock: Pillow releases the GIL while it decodes
        with self._lock:
            self._cache[key] = t
            while len(self._cache) > self._cache_tiles:
                self._cache.popitem(last=False)
        return t

    def read_region(self, location, level, size):
        """(x, y) in level-0 pixels, size (w, h) at `level` -> PIL RGBA image; 0 with alpha 0 outside the level."""
        from PIL import Image
        lv = self.levels[level]
        ds = self.level_downsamples[level]
        x, y = int(location[0] // ds), int(location[1] // ds)
        w, h = int(size[0]), int(size[1])
        out = np.zeros((h, w, 4), np.uint8)
        y0, y1, x0, x1 = max(y, 0), min(y + h, lv.height), max(x, 0), min(x + w, lv.width)
        if y1 > y0 and x1 > x0:
            for ty in range(y0 // lv.tile_h, (y1 - 1) // lv.tile_h + 1):
                for tx in range(x0 // lv.tile_w, (x1 - 1) // lv.tile_w + 1):
                    t = self._tile(level, ty * lv.cols + tx)
                    ay0, ay1 = max(y0, ty * lv.tile_h), min(y1, (ty + 1) * lv.tile_h)
                    ax0, ax1 = max(x0, tx * lv.tile_w), min(x1, (tx + 1) * lv.tile_w)
                    out[ay0 - y:ay1 - y, ax0 - x:ax1 - x, :3] = t[ay0 - ty * lv.tile_h:ay1 - ty * lv.tile_h, ax0 - tx * lv.tile_w:ax1 - tx * lv.tile_w]
            out[y0 - y:y1 - y, x0 - x:x1 - x, 3] = 255
        return Image.fromarray(out, 'RGBA')

    # ---------------------------------------------------------------------------------------------------------------- device path
    def device_level(self, level, device):
        """(H, W, 3) u8 tensor of one level resident in HBM, decoded on the GPU; cached per (level, device)."""
        key = (level, str(device))
        if key not in self._dev:
            from . import ingest
            self._dev[key] = ingest.level_from_tiff(self, level, device)
        return self._dev[key]

    def close(self):
        self._dev = {}
        self._cache = collections.OrderedDict()
        if getattr(self, '_map', None) is not None:
            self._map.close()
            self._map = None
        if getattr(self, '_f', None) is not None:
            self._f.close()
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _set_adobe_transform(stream, transform):
    """The stream with its APP0 (JFIF) / APP14 (Adobe) segments replaced by one Adobe segment carrying `transform`: libjpeg then
    decodes three components as YCbCr (1) or as they are (0), which is what libtiff asks of it from the photometric tag."""
    out, i, n = [stream[:2]], 2, len(stream)
    out.append(b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00' + bytes([1 if transform else 0]))
    while i + 4 <= n and stream[i] == 0xFF:
        mk = stream[i + 1]
        ln = struct.unpack('>H', stream[i + 2:i + 4])[0]
        if mk == 0xDA:
            break
        if mk not in (0xE0, 0xEE):
            out.append(stream[i:i + 2 + ln])
        i += 2 + ln
    out.append(stream[i:])
    return b''.join(out)


def _decode_with_transform(stream, transform):
    from PIL import Image
    im = Image.open(io.BytesIO(_set_adobe_transform(bytes(stream), transform)))
    im.load()
    if im.mode != 'RGB':
        raise ValueError('mode %s' % im.mode)
    return np.array(im)
