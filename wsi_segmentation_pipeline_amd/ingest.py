"""Slide ingestion for the tile producer (reference utils/dataset.py:171-185): decoder threads fill
pinned host slots, the native ring (csrc/ingest.hip, wsi_ring_*) copies each band to the device and unpacks it into the
HBM-resident RGB level on a copy stream of its own; the compute stream only waits on a fence.  The decoder is whatever the
slide object provides (`read_region` of OpenSlide / ArraySlide / TiffSlide, or a raw band reader).  A TiffSlide has a second route
that does not decode on the host at all: level_from_tiff copies the compressed JPEG tiles and decodes them on the device
(csrc/jpeg.hip, wsi_jpeg_*).  Also the device side of `scan_resize != 1` (Pillow-exact bicubic tile resize, wsi_resample_*)."""
import collections
import ctypes as C
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import native
from .engine import _ptr, _require_gpu, _stream


class IngestRing:
    def __init__(self, slots=4, slot_bytes=64 << 20):
        self.lib = native.load()
        if not torch.cuda.is_available():
            raise RuntimeError('IngestRing needs a GPU (pinned slots + copy stream live in libwsi_hip)')
        self.slots, self.slot_bytes = int(slots), int(slot_bytes) & ~3
        h = C.c_void_p()
        native.check(self.lib.wsi_ring_create(C.byref(h), self.slots, self.slot_bytes), 'wsi_ring_create')
        self._h = h
        self.device_index = int(self.lib.wsi_ring_device(h))          # staging buffers + copy stream live on this device

    def close(self):
        if self._h is not None:
            self.lib.wsi_ring_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def slot_array(self, slot, shape):
        """numpy view of a pinned slot."""
        n = int(np.prod(shape))
        if n > self.slot_bytes:
            raise ValueError('band of %d bytes does not fit a %d-byte slot' % (n, self.slot_bytes))
        p = self.lib.wsi_ring_host_slot(self._h, slot)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n,)).reshape(shape)

    def upload_level(self, read_band, h, w, channels, device=None, out=None, workers=None, fence=True):
        """Fill an (h, w, 3) uint8 device level from `read_band(y0, rows, dst)` (dst: (rows, w, channels) pinned uint8 view the
        reader fills; called on worker threads, one band each).  Decode of band i+1.. overlaps the copy of band i.
        Returns the device tensor; with fence=True the current compute stream is ordered after the last copy."""
        dev = torch.device('cuda', self.device_index) if device is None else torch.device(device)
        if dev.type != 'cuda' or (dev.index if dev.index is not None else torch.cuda.current_device()) != self.device_index:
            raise ValueError('this ring stages for cuda:%d, not %s (one ring per device: default_ring(device))' % (self.device_index, dev))
        dev = torch.device('cuda', self.device_index)
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        _require_gpu(out, 'level')
        if out.device.index != self.device_index:
            raise ValueError('out lives on %s, the ring on cuda:%d' % (out.device, self.device_index))
        # `out` may be a block the caching allocator just recycled on the compute stream: the ring's copies must not overtake the
        # kernels still queued there that read its previous contents
        with torch.cuda.device(dev):
            native.check(self.lib.wsi_ring_acquire(self._h, _stream()), 'wsi_ring_acquire')
        if tuple(out.shape) != (h, w, 3) or not out.is_contiguous():
            raise ValueError('out must be a contiguous (h, w, 3) uint8 tensor')
        row_bytes = w * channels
        band = max(1, min(h, self.slot_bytes // row_bytes))
        if band * row_bytes > self.slot_bytes or (channels == 4 and row_bytes % 4):
            raise ValueError('slot too small for one row')
        nb = -(-h // band)
        pool = ThreadPoolExecutor(max_workers=min(workers or self.slots, self.slots))
        inflight = collections.deque()

        def decode(i, s):
            y0 = i * band
            rows = min(band, h - y0)
            read_band(y0, rows, self.slot_array(s, (rows, w, channels)))
            return y0, rows

        def submit(fut, s):
            y0, rows = fut.result()
            native.check(self.lib.wsi_ring_submit(self._h, s, rows, w, channels, row_bytes, out.data_ptr() + y0 * w * 3, w * 3), 'wsi_ring_submit')
        try:
            for i in range(nb):
                s = i % self.slots
                if len(inflight) == self.slots:
                    submit(*inflight.popleft())
                native.check(self.lib.wsi_ring_wait_slot(self._h, s), 'wsi_ring_wait_slot')
                inflight.append((pool.submit(decode, i, s), s))
            while inflight:
                submit(*inflight.popleft())
        finally:
            pool.shutdown(wait=True)
        if fence:
            with torch.cuda.device(dev):
                native.check(self.lib.wsi_ring_fence(self._h, _stream()), 'wsi_ring_fence')
        return out

    def drain(self):
        native.check(self.lib.wsi_ring_drain(self._h), 'wsi_ring_drain')


_default_rings = {}


def default_ring(device=None):
    """The process's ring of `device` (default: the current one) - one per device: staging buffers and copy stream are device
    resources."""
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _default_rings:
        with torch.cuda.device(idx):
            _default_rings[idx] = IngestRing()
    return _default_rings[idx]


def level_from_slide(scan, level, device, ring=None):
    """One pyramid level of an OpenSlide-like object (`read_region((x0, y0_level0), level, (w, rows))` -> RGBA PIL image) into
    HBM through the ring."""
    ring = ring or default_ring(device)
    w, h = scan.level_dimensions[level]
    ds = scan.level_downsamples[level]

    def read_band(y0, rows, dst):
        dst[...] = np.asarray(scan.read_region((0, int(y0 * ds)), level, (w, rows)))
    out = ring.upload_level(read_band, h, w, 4, device)
    return out


def level_from_array(arr, device, ring=None):
    """Host ndarray / memmap (h, w, 3|4) uint8 -> HBM through the ring (the band copy into the pinned slot is the "decode")."""
    ring = ring or default_ring(device)
    h, w, ch = arr.shape
    if ch == 4 and (w * 4) % 4 == 0:
        def read_band(y0, rows, dst):
            dst[...] = arr[y0:y0 + rows]
        return ring.upload_level(read_band, h, w, 4, device)

    def read_band3(y0, rows, dst):
        dst[...] = arr[y0:y0 + rows, :, :3]
    return ring.upload_level(read_band3, h, w, 3, device)


# ------------------------------------------------------------------------------------------ JPEG tiles, decoded on the device
JPEG_TABLE_SETS = 64                                   # capacity of the walk's table sets: the level's JPEGTables + tiles with tables of their own
JPEG_STAGE_BYTES = 64 << 20                            # compressed bytes of one batch (a larger single tile gets a batch of its own)


_jpeg_pinned = {}                                       # (device index, slot) -> pinned staging tensor, grown on demand and kept: pinning is slow
_jpeg_lock = threading.Lock()                           # one jpeg_decode_tiles at a time: the calls share the pinned slots


def _pinned_stage(index, slot, size):
    t = _jpeg_pinned.get((index, slot))
    if t is None or t.numel() < size:
        t = torch.empty(size, dtype=torch.uint8).pin_memory()
        _jpeg_pinned[(index, slot)] = t
    return t


def jpeg_parse_tables(blob):
    """(status, native.WsiJpegTables) of a table blob: TIFF tag 347, or the header of a complete stream (wsi_jpeg_parse_tables)."""
    lib = native.load()
    t = native.WsiJpegTables()
    data = np.frombuffer(bytes(blob), np.uint8)
    rc = lib.wsi_jpeg_parse_tables(data.ctypes.data_as(C.c_void_p), data.size, C.byref(t))
    if rc < 0:
        native.check(rc, 'wsi_jpeg_parse_tables')
    return rc, t


def jpeg_walk(buf, offsets, lengths, base=None, cap=JPEG_TABLE_SETS, sets=None, n_sets=0):
    """The marker walk over n streams of `buf` (uint8 ndarray): (records, sets, n_sets) - records a structured array of
    native.WsiJpegTile, sets a (cap,) structured array of native.WsiJpegTables (wsi_jpeg_walk).  sets / n_sets: carry on from an
    earlier walk."""
    lib = native.load()
    off = np.ascontiguousarray(offsets, np.uint64)
    ln = np.ascontiguousarray(lengths, np.uint32)
    if np.any(np.asarray(lengths, np.uint64) > 0xffffffff):
        raise ValueError('a tile stream of 4 GiB or more')
    rec = np.zeros(len(off), np.dtype(native.WsiJpegTile))
    if sets is None:
        sets = np.zeros(cap, np.dtype(native.WsiJpegTables))
    count = C.c_int(n_sets)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    native.check(lib.wsi_jpeg_walk(p(buf), buf.size, p(off), p(ln), len(off), C.byref(base) if base is not None else None, p(sets), len(sets),
                                   C.byref(count), p(rec)), 'wsi_jpeg_walk')
    return rec, sets, count.value


def _geometry(rec):
    return (int(rec['width']), int(rec['height']), int(rec['ncomp']), int(rec['h'][0]), int(rec['v'][0]))


def jpeg_stage(buf, rec, idx, cells, out=None):
    """The staging block of one batch - the records of tiles `idx` (scan_off rewritten to the block's data area), their grid cells
    (int32), padding to 16 bytes, the scan bytes of every tile at 4-byte steps - written into `out` (uint8 ndarray) or a new array.
    Returns (offset of the data area, bytes of scan data, the array)."""
    n, rec_size = len(idx), C.sizeof(native.WsiJpegTile)
    data_at = (n * (rec_size + 4) + 15) // 16 * 16
    tot = int(((rec['scan_len'][idx].astype(np.int64) + 3) // 4 * 4).sum())
    if out is None:
        out = np.zeros(data_at + tot, np.uint8)
    r = rec[idx].copy()
    at = 0
    for j, i in enumerate(idx):
        o, l = int(rec['scan_off'][i]), int(rec['scan_len'][i])
        out[data_at + at:data_at + at + l] = buf[o:o + l]
        r['scan_off'][j] = at
        at += (l + 3) // 4 * 4
    out[:n * rec_size] = r.view(np.uint8).reshape(-1)
    out[n * rec_size:n * (rec_size + 4)] = np.ascontiguousarray(np.asarray(cells)[idx], np.int32).view(np.uint8)
    return data_at, tot, out


def jpeg_decode_batch(stage, nbytes, n, sets_dev, n_sets, common_set, geometry, ws, status, transform, grid, level, lanes=0):
    """Entropy decode + reconstruct of one batch already on the device.  stage: device uint8 tensor holding n records, n grid cells
    (int32), padding to 16 bytes, then nbytes of scan data; status: n int32 on the device; level: a (H, W, 3) u8 view whose rows are
    dense (any pitch, any alignment); lanes: tiles per wave of the entropy kernel, 0 = the library's choice."""
    lib = native.load()
    w, h, nc, hs, vs = geometry
    rec_bytes = n * C.sizeof(native.WsiJpegTile)
    data_at = (rec_bytes + 4 * n + 15) // 16 * 16
    base = stage.data_ptr()
    native.check(lib.wsi_jpeg_entropy(C.c_void_p(base + data_at), nbytes, C.c_void_p(base), n, _ptr(sets_dev), n_sets, common_set, w, h, nc, hs, vs,
                                      _ptr(ws), ws.numel(), _ptr(status), int(lanes), _stream()), 'wsi_jpeg_entropy')
    H, W = level.shape[0], level.shape[1]
    if level.stride(2) != 1 or level.stride(1) != 3 or level.dtype != torch.uint8 or level.shape[2] != 3:
        raise ValueError('level must be a (H, W, 3) uint8 view with dense rows')
    native.check(lib.wsi_jpeg_reconstruct(_ptr(ws), ws.numel(), _ptr(status), C.c_void_p(base + rec_bytes), n, w, h, nc, hs, vs, int(transform),
                                          grid[0], grid[1], _ptr(level), level.stride(0), H, W, _stream()), 'wsi_jpeg_reconstruct')


def jpeg_decode_tiles(buf, rec, sets, n_sets, cells, grid, level, transform, workspace_bytes=1 << 30, stage_bytes=JPEG_STAGE_BYTES, lanes=0):
    """Decode the streams the walk accepted (rec['status'] == 0) into `level` on its device: tile i goes to grid cell cells[i] of
    grid = (cols, rows).  The compressed scan bytes of a batch go through pinned memory on a copy stream while the batch before it
    is decoded on the current stream; the coefficient workspace stays under workspace_bytes.  Tiles are grouped by frame geometry (a
    batch has one).  Returns the int32 status of every tile as a host array: the walk's where it was non-zero, else the kernel's."""
    _require_gpu(level, 'level')
    lib = native.load()
    dev = level.device
    status = rec['status'].astype(np.int32).copy()
    ok = np.nonzero(status == 0)[0]
    if len(ok) == 0:
        return status
    groups = {}
    for i in ok:
        groups.setdefault(_geometry(rec[i]), []).append(int(i))
    common_set = int(np.bincount(rec['table_set'][ok]).argmax())
    rec_size = C.sizeof(native.WsiJpegTile)
    with _jpeg_lock, torch.cuda.device(dev):
        cur = torch.cuda.current_stream()
        copy = torch.cuda.Stream()
        sets_dev = torch.from_numpy(sets[:n_sets].view(np.uint8).reshape(-1).copy()).to(dev)
        # the batches: whole tiles, at most `per` of them and at most stage_bytes of scan data
        batches = []
        for geom, idx in groups.items():
            tile_ws = lib.wsi_jpeg_workspace_bytes(*geom)
            if tile_ws == 0:
                status[idx] = native.JpegStatus.GEOMETRY
                continue
            per = max(1, int(workspace_bytes) // tile_ws)
            lens = (rec['scan_len'][idx].astype(np.int64) + 3) // 4 * 4
            a = 0
            while a < len(idx):
                b, tot = a, 0
                while b < len(idx) and b - a < per and (b == a or tot + lens[b] <= stage_bytes):
                    tot += int(lens[b])
                    b += 1
                batches.append((geom, idx[a:b], tot, tile_ws))
                a = b
        if not batches:
            return status
        stage_size = max((len(ix) * (rec_size + 4) + 15) // 16 * 16 + tot for _, ix, tot, _ in batches)
        ws = torch.empty(max(len(ix) * tw for _, ix, _, tw in batches), dtype=torch.uint8, device=dev)
        pinned = [_pinned_stage(dev.index if dev.index is not None else torch.cuda.current_device(), k, stage_size) for k in range(min(2, len(batches)))]
        staged = [torch.empty(stage_size, dtype=torch.uint8, device=dev) for _ in pinned]
        copied = [torch.cuda.Event() for _ in pinned]
        decoded = [torch.cuda.Event() for _ in pinned]
        outs = []
        for k, (geom, idx, tot, _) in enumerate(batches):
            s = k % len(pinned)
            n = len(idx)
            if k >= len(pinned):
                copied[s].synchronize()                        # the pinned slot's last copy has left it
            data_at, _, _ = jpeg_stage(buf, rec, idx, cells, pinned[s].numpy())
            if k >= len(pinned):
                copy.wait_event(decoded[s])                    # the device slot's last batch has been decoded
            with torch.cuda.stream(copy):
                staged[s][:data_at + tot].copy_(pinned[s][:data_at + tot], non_blocking=True)
                copied[s].record(copy)
            cur.wait_event(copied[s])
            st = torch.empty(n, dtype=torch.int32, device=dev)
            jpeg_decode_batch(staged[s], tot, n, sets_dev, n_sets, common_set, geom, ws, st, transform, grid, level, lanes)
            decoded[s].record(cur)
            outs.append((idx, st))
        for idx, st in outs:
            status[idx] = st.cpu().numpy()
        cur.synchronize()                                      # the pinned slots are free for the next call
    return status


def level_from_tiff(slide, level, device, workspace_bytes=1 << 30):
    """One level of a TiffSlide into HBM, decoded on the device (reference utils/dataset.py:171-185: OpenSlide's read_region).  The
    file is mapped, the marker walk fills one record per tile, the compressed bytes travel in batches and are decoded into the level.
    Tiles the device path does not take (the walk's status, or the kernel's) are decoded by Pillow on the host and copied in; a tile of
    byte count 0 is white.  slide.decode_report[level] = {status name: tiles}.  ValueError where Pillow cannot decode such a tile
    either."""
    if not torch.cuda.is_available():
        raise RuntimeError('level_from_tiff needs a GPU (the JPEG decode is a HIP kernel; the host path is TiffSlide.read_region)')
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('level_from_tiff decodes on a GPU, not on %s' % dev)
    lv = slide.levels[level]
    buf = np.frombuffer(slide._map, np.uint8)
    base = None
    if lv.tables:
        rc, base = jpeg_parse_tables(lv.tables)
        if rc:
            raise ValueError('level %d: tag 347 JPEGTables cannot be parsed (%s)' % (level, native.JpegStatus(rc).name))
    if np.any(lv.offsets + lv.counts > buf.size):
        raise ValueError('level %d: a tile lies outside the file' % level)
    rec, sets, n_sets = jpeg_walk(buf, lv.offsets, lv.counts, base)
    n = len(rec)
    # the device path stores whole frames at the cells of the level's tile grid: a frame that is not the tile goes to the host path
    odd = (rec['status'] == 0) & ((rec['width'] != lv.tile_w) | (rec['height'] != lv.tile_h) | (rec['ncomp'] != lv.samples))
    rec['status'][odd] = native.JpegStatus.GEOMETRY
    with torch.cuda.device(dev):
        if (rec['status'] == native.JpegStatus.EMPTY).any():
            out = torch.full((lv.height, lv.width, 3), 255, dtype=torch.uint8, device=dev)
        else:
            out = torch.empty((lv.height, lv.width, 3), dtype=torch.uint8, device=dev)
        status = jpeg_decode_tiles(buf, rec, sets, max(n_sets, 1), np.arange(n, dtype=np.int32), (lv.cols, lv.rows), out, lv.transform,
                                   workspace_bytes)
        report = {}
        for i in np.nonzero(status != 0)[0]:
            name = native.JpegStatus(int(status[i])).name.lower()
            report[name] = report.get(name, 0) + 1
            if status[i] == native.JpegStatus.EMPTY:
                continue
            t = slide.decode_tile_host(level, int(i))            # ValueError names level and tile
            y0, x0 = (int(i) // lv.cols) * lv.tile_h, (int(i) % lv.cols) * lv.tile_w
            hh, ww = min(lv.tile_h, lv.height - y0), min(lv.tile_w, lv.width - x0)
            out[y0:y0 + hh, x0:x0 + ww] = torch.from_numpy(np.ascontiguousarray(t[:hh, :ww])).to(dev)
        report['ok'] = int((status == 0).sum())
        slide.decode_report[level] = report
    return out


# ------------------------------------------------------------------------------------------ scan_resize != 1
_plans = {}


def _plan(lib, in_hw, out_hw, device):
    key = (tuple(in_hw), tuple(out_hw), str(device))
    if key not in _plans:
        h = C.c_void_p()
        with torch.cuda.device(device):
            native.check(lib.wsi_resample_plan_create(C.byref(h), in_hw[0], in_hw[1], out_hw[0], out_hw[1]), 'wsi_resample_plan_create')
        _plans[key] = h
    return _plans[key]


def resize_tiles_bicubic(level, tile_xy, in_hw, out_hw):
    """n tiles of in_hw at tile_xy (level pixels, (x, y)) of the (H,W,3) uint8 GPU level -> (n, out_h, out_w, 3) uint8, exactly
    PIL `Image.resize((out_w, out_h))` of each crop (reference utils/dataset.py:180-181)."""
    lib = native.load()
    _require_gpu(level, 'level')
    if level.dtype != torch.uint8 or level.dim() != 3 or level.shape[2] != 3 or not level.is_contiguous():
        raise ValueError('level must be a contiguous (H,W,3) uint8 tensor')
    xy = torch.as_tensor(tile_xy, dtype=torch.int32).to(level.device).contiguous()
    n = xy.shape[0]
    plan = _plan(lib, in_hw, out_hw, level.device)
    out = torch.empty((n, out_hw[0], out_hw[1], 3), dtype=torch.uint8, device=level.device)
    scratch = torch.empty(max(1, lib.wsi_resample_scratch_bytes(plan, n)), dtype=torch.uint8, device=level.device)
    native.check(lib.wsi_resample_tiles(plan, _ptr(level), level.stride(0), level.shape[0], level.shape[1], _ptr(xy), n, _ptr(out),
                                        _ptr(scratch), _stream()), 'wsi_resample_tiles')
    return out
