"""Write JPEG-tiled pyramidal TIFF from levels resident in HBM: the mirror of tiffslide.py + ingest.level_from_tiff.

The tiles of a (H, W, 3) or (H, W) u8 CUDA tensor are encoded on the device (csrc/jpeg_enc.hip: colour, downsample, FDCT, quantise,
then a size pass and a write pass of the entropy stage); this module adds the markers and the container with `struct`, as the parser
reads them.  One tiled IFD per level in file order, compression 7, the tables once per level in tag 347 JPEGTables (SOI, DQT, DHT,
EOI), abbreviated tile streams (SOI, SOF0, [DRI], SOS, scan, EOI), PhotometricInterpretation 6 + YCbCrSubSampling for three
components, 1 for one, NewSubfileType 1 on the reduced levels.  Classic TIFF, BigTIFF where an offset passes 4 GiB or on request.
Tiles at the right and bottom edge are whole: a pixel outside the level repeats the nearest level pixel.  The scan bytes are
libjpeg's for the same pixels, tables and sampling (spec: tests/jpeg_enc_oracle.py), so TiffSlide, OpenSlide, QuPath and libtiff
read the file."""
import contextlib
import ctypes as C
import struct
import threading

import numpy as np

from . import native

SAMPLINGS = ((1, 1), (2, 1), (2, 2))
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
           57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
WORKSPACE_BYTES = 1 << 30                               # coefficient workspace of one batch: a 16 384^2 level in 256^2 tiles is one batch, and every tile a lane of one launch
_lock = threading.Lock()                                # one device write_pyramid at a time: the calls share the pinned slots
_pinned = {}                                            # (device index, slot) -> pinned host tensor, grown on demand and kept: pinning is slow


# ------------------------------------------------------------------------------------------------------------------ markers
def quality_tables(quality):
    """(luma, chroma) quantisation tables of a libjpeg quality, (64,) u8 in natural order (wsi_jenc_quality_tables)"""
    lib = native.load()
    lum, chrom = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    native.check(lib.wsi_jenc_quality_tables(int(quality), lum.ctypes.data_as(C.c_void_p), chrom.ctypes.data_as(C.c_void_p)), 'wsi_jenc_quality_tables')
    return lum, chrom


def std_huff(table):
    """(16 code counts, symbols) of standard table 0..3: DC luma, DC chroma, AC luma, AC chroma (wsi_jenc_std_huff)"""
    lib = native.load()
    counts, symbols, n = np.zeros(16, np.uint8), np.zeros(256, np.uint8), C.c_int(0)
    native.check(lib.wsi_jenc_std_huff(int(table), counts.ctypes.data_as(C.c_void_p), symbols.ctypes.data_as(C.c_void_p), C.byref(n)), 'wsi_jenc_std_huff')
    return bytes(counts), bytes(symbols[:n.value])


def _check_qtables(qtables):
    q = [np.asarray(t).reshape(64) for t in qtables]
    if len(q) != 2 or any(t.min() < 1 or t.max() > 255 for t in q):
        raise ValueError('qtables: two tables of 64 entries in 1..255, natural order')
    return [np.ascontiguousarray(t, np.uint8) for t in q]


def jpeg_tables(qtables, ncomp):
    """TIFF tag 347: SOI, one DQT per quantisation table, one DHT per Huffman table the components use, EOI"""
    ids = (0, 1) if ncomp == 3 else (0,)
    out = [b'\xff\xd8']
    for i in ids:
        out.append(b'\xff\xdb' + struct.pack('>HB', 67, i) + bytes(int(qtables[i][k]) for k in _ZIGZAG))
    for i in ids:                                               # libjpeg's order: DC 0, AC 0, DC 1, AC 1
        for cls in (0, 1):
            counts, symbols = std_huff(2 * cls + i)
            out.append(b'\xff\xc4' + struct.pack('>HB', 19 + len(symbols), (cls << 4) | i) + counts + symbols)
    out.append(b'\xff\xd9')
    return b''.join(out)


def tile_header(width, height, ncomp, sampling, restart=0):
    """what stands in front of a tile's scan in an abbreviated stream: SOI, SOF0, [DRI], SOS"""
    hs, vs = sampling if ncomp == 3 else (1, 1)
    comps = [(1, (hs << 4) | vs, 0), (2, 0x11, 1), (3, 0x11, 1)][:ncomp]
    out = b'\xff\xd8\xff\xc0' + struct.pack('>HBHHB', 8 + 3 * ncomp, 8, height, width, ncomp) + b''.join(bytes(c) for c in comps)
    if restart:
        out += b'\xff\xdd' + struct.pack('>HH', 4, restart)
    return out + b'\xff\xda' + struct.pack('>HB', 6 + 2 * ncomp, ncomp) + b''.join(bytes([c[0], (c[2] << 4) | c[2]]) for c in comps) + b'\x00\x3f\x00'


# ------------------------------------------------------------------------------------------------------------------ device encode
def _level_view(level):
    import torch
    if not isinstance(level, torch.Tensor) or not level.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError('the JPEG encode needs a GPU (it is a HIP kernel; there is no host path)')
        raise RuntimeError('the JPEG encode runs on a GPU tensor, not on %s' % (level.device if isinstance(level, torch.Tensor) else type(level).__name__))
    ncomp = 1 if level.dim() == 2 else 3
    if level.dtype != torch.uint8 or level.dim() not in (2, 3) or (level.dim() == 3 and level.shape[2] != 3) or level.shape[0] < 1 or level.shape[1] < 1:
        raise ValueError('a level is a (H, W, 3) or (H, W) uint8 tensor')
    if level.stride(1) != ncomp or (ncomp == 3 and level.stride(2) != 1) or level.stride(0) < level.shape[1] * ncomp:
        raise ValueError('a level must have dense rows (any pitch, any alignment)')
    return ncomp


def _geometry(tile, ncomp, subsampling):
    tw, th = int(tile[0]), int(tile[1])
    hs, vs = (int(subsampling[0]), int(subsampling[1])) if ncomp == 3 else (1, 1)
    tile_ws = native.load().wsi_jenc_workspace_bytes(tw, th, ncomp, hs, vs)
    if tile_ws == 0:
        raise ValueError('tile %s / sampling %s: sides are multiples of 16 in 16..4096, the luma sampling is 1x1, 2x1 or 2x2' % ((tw, th), (hs, vs)))
    return tw, th, hs, vs, tile_ws


class _DeviceEncoder:
    """The batches of one call: the coefficient workspace, two device and two pinned slots for the scan bytes, a copy stream.  While
    the device encodes batch k + 1, batch k's bytes come to the host on the copy stream and are handed to the caller."""

    def __init__(self, device, workspace_bytes):
        import torch
        self.torch, self.dev = torch, device
        self.budget = int(workspace_bytes)
        self.ws = None
        self.out = [None, None]
        index = device.index if device.index is not None else torch.cuda.current_device()
        self.keys = [(index, 0), (index, 1)]
        self.copy = torch.cuda.Stream(device)
        self.copied = [torch.cuda.Event(), torch.cuda.Event()]

    def _grow(self, t, size, pin=False):
        if t is not None and t.numel() >= size:
            return t
        size = max(size, 1 << 20)
        return self.torch.empty(size, dtype=self.torch.uint8).pin_memory() if pin else self.torch.empty(size, dtype=self.torch.uint8, device=self.dev)

    def _plan(self, levels, tile, subsampling):
        """[(geometry, [(level index, first cell, tiles)])]: the tiles of all levels in level order cut into batches of one geometry
        under the byte budget - the small levels of a pyramid share a batch, so their tiles are lanes of the same launches"""
        plan, pieces, geom, room = [], [], None, 0
        for li, level in enumerate(levels):
            g = _geometry(tile, _level_view(level), subsampling) + (_level_view(level),)
            if pieces and g != geom:
                plan.append((geom, pieces))
                pieces = []
            if not pieces:
                room = max(1, self.budget // g[4])
            geom = g
            first, tiles = 0, -(-int(level.shape[1]) // g[0]) * -(-int(level.shape[0]) // g[1])
            while first < tiles:
                n = min(room, tiles - first)
                pieces.append((li, first, n))
                first, room = first + n, room - n
                if room == 0:
                    plan.append((geom, pieces))
                    pieces, room = [], max(1, self.budget // g[4])
        if pieces:
            plan.append((geom, pieces))
        return plan

    def batches(self, levels, tile, qtables, subsampling, restart, to_host=True, lanes=0):
        """yields (level index, first cell, sizes (n,) uint32, offsets (n,) uint64, buffer) in level order, then cell order: tile i
        of the piece is buffer[offsets[i]:offsets[i] + sizes[i]].  to_host: the buffer is a pinned host array the caller must have
        consumed before it takes a piece of the batch after the next; else a device tensor of the batch's own."""
        from .engine import _ptr, _stream
        torch, lib = self.torch, native.load()
        q = _check_qtables(qtables)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        plan = self._plan(levels, tile, subsampling)
        pending = None
        with torch.cuda.device(self.dev):
            cur = torch.cuda.current_stream()
            self.ws = self._grow(self.ws, max(sum(pc[2] for pc in pieces) * g[4] for g, pieces in plan))
            for k, ((tw, th, hs, vs, tile_ws, ncomp), pieces) in enumerate(plan):
                n, s, at = sum(pc[2] for pc in pieces), k & 1, 0
                for li, first, cnt in pieces:
                    level = levels[li]
                    H, W = int(level.shape[0]), int(level.shape[1])
                    native.check(lib.wsi_jenc_transform(_ptr(level), level.stride(0), H, W, -(-W // tw), -(-H // th), first, cnt, tw, th, ncomp, hs, vs, p(q[0]),
                                                        p(q[1]), C.c_void_p(self.ws.data_ptr() + at * tile_ws), self.ws.numel() - at * tile_ws, _stream()),
                                 'wsi_jenc_transform')
                    at += cnt
                sizes_dev = torch.empty(n, dtype=torch.int32, device=self.dev)
                native.check(lib.wsi_jenc_entropy_size(_ptr(self.ws), self.ws.numel(), n, tw, th, ncomp, hs, vs, int(restart), _ptr(sizes_dev), int(lanes),
                                                       _stream()), 'wsi_jenc_entropy_size')
                sizes = sizes_dev.cpu().numpy().view(np.uint32)
                offsets = np.zeros(n, np.uint64)
                np.cumsum((sizes[:-1].astype(np.uint64) + 15) // 16 * 16, out=offsets[1:])
                total = int(offsets[-1]) + int(sizes[-1])
                ranges = torch.empty(12 * n + 8, dtype=torch.uint8, device=self.dev)
                # slot s last held batch k - 2: its copy was waited for and the caller has consumed it before asking for more
                out = self.out[s] = self._grow(self.out[s], total) if to_host else torch.empty(max(total, 1), dtype=torch.uint8, device=self.dev)
                native.check(lib.wsi_jenc_entropy_write(_ptr(self.ws), self.ws.numel(), n, tw, th, ncomp, hs, vs, int(restart), p(offsets), p(sizes),
                                                        _ptr(ranges), _ptr(out), out.numel(), int(lanes), _stream()), 'wsi_jenc_entropy_write')
                bounds = np.cumsum([0] + [pc[2] for pc in pieces])
                if not to_host:
                    cur.synchronize()                           # the write pass has read offsets / sizes (host arrays)
                    self.out[s] = None
                    view = out[:total]
                    for (li, first, cnt), a in zip(pieces, bounds):
                        yield li, first, sizes[a:a + cnt], offsets[a:a + cnt], view
                    continue
                pinned = _pinned[self.keys[s]] = self._grow(_pinned.get(self.keys[s]), total, pin=True)
                self.copy.wait_stream(cur)
                with torch.cuda.stream(self.copy):
                    pinned[:total].copy_(out[:total], non_blocking=True)
                    self.copied[s].record(self.copy)
                if pending is not None:                         # batch k - 1: its copy ran beside this batch's transform and size pass;
                    self.copied[1 - s].synchronize()            # the caller works on it beside this batch's write pass and copy
                    yield from pending
                host = pinned.numpy()[:total]
                pending = [(li, first, sizes[a:a + cnt], offsets[a:a + cnt], host) for (li, first, cnt), a in zip(pieces, bounds)]
            if pending is not None:
                self.copied[s].synchronize()
                yield from pending


def encode_level(level, tile=(256, 256), quality=75, subsampling=(2, 2), restart=0, qtables=None, workspace_bytes=WORKSPACE_BYTES, lanes=0):
    """Encode every tile of a resident level: (offsets (n,) uint64, sizes (n,) uint32, scan) - tile i (raster order of the level's tile
    grid) is scan[offsets[i]:offsets[i] + sizes[i]], scan a uint8 tensor on the level's device; every offset is a multiple of 16.
    tile = (tile_w, tile_h), multiples of 16; subsampling = the luma sampling (1, 1), (2, 1) or (2, 2) (ignored for a one-component
    level); restart: MCUs per restart interval; qtables: (luma, chroma) in natural order instead of `quality`'s.  The coefficient
    workspace of a batch stays under workspace_bytes.  RuntimeError without a GPU: the encode has no host path."""
    _level_view(level)
    import torch
    enc = _DeviceEncoder(level.device, workspace_bytes)
    q = qtables if qtables is not None else quality_tables(quality)
    offs, sizes, parts, base, last = [], [], [], 0, None
    for _, _, sz, off, buf in enc.batches([level], tile, q, subsampling, restart, to_host=False, lanes=lanes):
        if buf is not last and last is not None:
            base += parts[-1].numel()
        if buf is not last:
            pad = -buf.numel() % 16
            parts.append(buf if pad == 0 else torch.cat([buf, torch.zeros(pad, dtype=torch.uint8, device=buf.device)]))
            last = buf
        offs.append(off + np.uint64(base))
        sizes.append(sz)
    return np.concatenate(offs), np.concatenate(sizes), parts[0] if len(parts) == 1 else torch.cat(parts)


def downsample_level(level, factor):
    """(H // factor, W // factor[, 3]) box mean of a resident level, rounded half up (wsi_jenc_downsample); factor 2 or 4"""
    from .engine import _ptr, _stream
    import torch
    ncomp = _level_view(level)
    H, W = int(level.shape[0]), int(level.shape[1])
    if factor not in (2, 4) or H // factor < 1 or W // factor < 1:
        raise ValueError('downsample: factor 2 or 4 and a level of at least factor x factor pixels')
    with torch.cuda.device(level.device):
        out = torch.empty((H // factor, W // factor) + ((3,) if ncomp == 3 else ()), dtype=torch.uint8, device=level.device)
        native.check(native.load().wsi_jenc_downsample(_ptr(level), level.stride(0), H, W, ncomp, int(factor), _ptr(out), out.stride(0), _stream()),
                     'wsi_jenc_downsample')
    return out


# ------------------------------------------------------------------------------------------------------------------ container
def _ifd_entries(width, height, ncomp, tile, sampling, tables, offsets, counts, big, reduced, description, mpp):
    """[(tag, type, count, packed little-endian value bytes)] of one level, sorted by tag"""
    pk = lambda fmt, *v: struct.pack('<' + fmt, *v)
    n = len(offsets)
    ent = [(254, 4, 1, pk('I', 1 if reduced else 0)), (256, 4, 1, pk('I', width)), (257, 4, 1, pk('I', height)),
           (258, 3, ncomp, pk('H' * ncomp, *([8] * ncomp))), (259, 3, 1, pk('H', 7)), (262, 3, 1, pk('H', 6 if ncomp == 3 else 1)),
           (277, 3, 1, pk('H', ncomp)), (284, 3, 1, pk('H', 1)), (322, 4, 1, pk('I', tile[0])), (323, 4, 1, pk('I', tile[1])),
           (324, 16 if big else 4, n, pk(('Q' if big else 'I') * n, *offsets)), (325, 4, n, pk('I' * n, *counts)), (347, 7, len(tables), tables)]
    if description:
        text = description.encode('utf-8') + b'\0'
        ent.append((270, 2, len(text), text))
    if mpp:
        per_cm = 1e4 / float(mpp)                               # pixels per centimetre as a rational over 1000
        ent += [(282, 5, 1, pk('II', int(round(per_cm * 1000)), 1000)), (283, 5, 1, pk('II', int(round(per_cm * 1000)), 1000)), (296, 3, 1, pk('H', 3))]
    if ncomp == 3:
        ent.append((530, 3, 2, pk('HH', *sampling)))
    return sorted(ent, key=lambda t: t[0])


def _write_directories(f, dirs, big, at):
    """the IFD chain at file offset `at` (the file's end); returns the first IFD's offset"""
    off_t, inline = ('Q', 8) if big else ('I', 4)
    out, first, ptr_at = bytearray(), None, None

    def blob(data):
        if (at + len(out)) & 1:
            out.append(0)
        p = at + len(out)
        out.extend(data)
        return p
    for ent in dirs:
        fields = []
        for tag, typ, cnt, data in ent:
            val = bytes(data) + b'\0' * (inline - len(data)) if len(data) <= inline else struct.pack('<' + off_t, blob(data))
            fields.append(struct.pack('<HH' + off_t, tag, typ, cnt) + val)
        here = blob(b'')
        if first is None:
            first = here
        else:
            struct.pack_into('<' + off_t, out, ptr_at, here)
        out += struct.pack('<' + ('Q' if big else 'H'), len(fields)) + b''.join(fields)
        ptr_at = len(out)
        out += struct.pack('<' + off_t, 0)
    f.seek(at)
    f.write(out)
    return first, at + len(out)


def write_tiles(f, head, sizes, offs, buf, offsets, counts):
    """append one batch's tile streams - head, buf[offs[i]:offs[i] + sizes[i]], EOI - to the file at even offsets; their file offsets
    and byte counts are appended to the two lists"""
    for sz, o in zip(sizes.tolist(), offs.tolist()):
        offsets.append(f.tell())
        f.write(head)
        f.write(memoryview(buf[o:o + sz]))
        f.write(b'\xff\xd9')
        counts.append(len(head) + sz + 2)
        if f.tell() & 1:
            f.write(b'\0')


def write_pyramid(path, levels, tile=(256, 256), quality=75, subsampling=(2, 2), downsample=None, description=None, mpp=None, big=None,
                  restart=0, qtables=None, workspace_bytes=WORKSPACE_BYTES, encode=None):
    """Write `levels` as a JPEG-tiled pyramidal TIFF.  levels: a list of u8 CUDA tensors ((H, W, 3) or (H, W), level 0 first), or one
    tensor with downsample = 2 or 4: the further levels are box means of the one before (downsample_level) until both sides fit in
    one tile, which is the last level.  tile = (tile_w, tile_h); quality / qtables, subsampling, restart as in encode_level.
    description: tag 270 of level 0; mpp: microns per pixel of level 0 (tags 282 / 283 / 296 on every level).  big: None = BigTIFF
    only where the file needs it (an offset at or past 4 GiB), True / False = forced (False raises where it does not fit).
    encode: a stand-in for the device encode, `encode(level, tile, qtables, subsampling, restart)` yielding (first cell, sizes,
    offsets, buffer) batches as _DeviceEncoder.batches does (the CPU tests pass the NumPy spec).
    Returns dict(tiles, bytes, big, levels=[dict(width, height, tiles, bytes)])."""
    import torch
    if isinstance(levels, torch.Tensor) or isinstance(levels, np.ndarray):
        levels = [levels]
    levels = list(levels)
    if not levels:
        raise ValueError('write_pyramid needs at least one level')
    if downsample is not None:
        if len(levels) != 1 or downsample not in (2, 4):
            raise ValueError('downsample = 2 or 4 goes with ONE level: the others are made from it')
    q = _check_qtables(qtables if qtables is not None else quality_tables(quality))
    enc = None
    if encode is None:
        _level_view(levels[0])
        enc = _DeviceEncoder(levels[0].device, workspace_bytes)
    geoms = [_geometry(tile, 1 if levels[0].ndim == 2 else 3, subsampling)]
    if downsample is not None:                                  # all levels first: the small ones then share a batch of the encode
        tw, th = geoms[0][:2]
        while (levels[-1].shape[1] > tw or levels[-1].shape[0] > th) and min(levels[-1].shape[:2]) >= downsample:
            levels.append(downsample_level(levels[-1], downsample))
    geoms = [_geometry(tile, 1 if l.ndim == 2 else 3, subsampling) for l in levels]
    found = [([], []) for _ in levels]                          # per level: the file offsets and byte counts of its tiles
    heads = [tile_header(g[0], g[1], 1 if l.ndim == 2 else 3, g[2:4], restart) for g, l in zip(geoms, levels)]

    def pieces():
        if enc is not None:
            return enc.batches(levels, tile, q, subsampling, restart)
        return ((li, first, sizes, offs, buf) for li, (l, g) in enumerate(zip(levels, geoms)) for first, sizes, offs, buf in encode(l, g[:2], q, g[2:4], restart))
    with (_lock if enc is not None else contextlib.nullcontext()), open(path, 'wb') as f:
        f.write(b'\0' * 16)                                     # the header: 8 bytes of classic TIFF or 16 of BigTIFF, written last
        for li, first, sizes, offs, buf in pieces():
            if first != len(found[li][0]) or any(len(found[j][0]) == 0 for j in range(li)):
                raise RuntimeError('level %d: tiles out of order' % li)
            write_tiles(f, heads[li], sizes, offs, buf, *found[li])
        report = dict(tiles=0, bytes=0, levels=[])
        dirs = []
        for k, (level, g) in enumerate(zip(levels, geoms)):
            H, W, ncomp = int(level.shape[0]), int(level.shape[1]), 1 if level.ndim == 2 else 3
            offsets, counts = found[k]
            if len(offsets) != -(-W // g[0]) * -(-H // g[1]):
                raise RuntimeError('level %d: %d tiles encoded for a %d x %d level' % (k, len(offsets), W, H))
            dirs.append((W, H, ncomp, g[:2], g[2:4], jpeg_tables(q, ncomp), offsets, counts, k > 0,
                         description if k == 0 else None, mpp * int(levels[0].shape[1]) / W if mpp else None))
            report['levels'].append(dict(width=W, height=H, tiles=len(offsets), bytes=int(sum(counts))))
        end = f.tell()
        # every offset in the file is below `end` + the directories, which hold 12 bytes per tile and the tables: BigTIFF where that passes 4 GiB
        dir_bytes = sum(len(d[6]) * 12 + len(d[5]) + 400 for d in dirs) + (len(description.encode('utf-8')) if description else 0)
        need_big = end + dir_bytes >= 1 << 32
        if big is None:
            big = need_big
        elif not big and need_big:
            raise ValueError('the file needs BigTIFF: %d bytes' % (end + dir_bytes))
        first, size = _write_directories(f, [_ifd_entries(*d[:7], d[7], big, *d[8:]) for d in dirs], big, end)
        f.seek(0)
        f.write(b'II' + (struct.pack('<HHHQ', 43, 8, 0, first) if big else struct.pack('<HI', 42, first)))
    report['tiles'] = sum(l['tiles'] for l in report['levels'])
    report['bytes'] = size
    report['big'] = bool(big)
    return report


def save_slide(scan, path, levels=None, device='cuda', **kw):
    """Write the levels of a slide-like object (TiffSlide, ArraySlide, stain.StainedSlide: the normalised slide, ...) through its
    device_level(level, device); levels: the level numbers, all by default.  Keywords go to write_pyramid."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('save_slide needs a GPU (the JPEG encode is a HIP kernel; there is no host path)')
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('save_slide encodes on a GPU, not on %s' % dev)
    ks = list(range(scan.level_count)) if levels is None else list(levels)
    return write_pyramid(path, [scan.device_level(k, dev) for k in ks], **kw)
