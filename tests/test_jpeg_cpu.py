"""CPU side of the JPEG path: the oracle against Pillow (0 differing bytes), TiffSlide against Pillow's libtiff, the marker walk of
the library against the oracle's parse, every status code, the C-ABI entries and their argument checks, and the walk plus the shared
per-tile decode loop as a stand-alone program under the host sanitizers."""
import ctypes as C
import io
import itertools
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_oracle as O                                        # noqa: E402
import tiff_fixture as TF                                      # noqa: E402
from wsi_segmentation_pipeline_amd import native                # noqa: E402
from wsi_segmentation_pipeline_amd.tiffslide import TiffSlide   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((48, 80), (37, 53), (64, 64))                          # (width, height)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


def _content(kind, h, w, seed, channels=3):
    return (TF.noise if kind == 'noise' else TF.he_like)(h, w, seed, channels)


def _matrix():
    """(name, stream): sub-sampling x quality x content x size, restart intervals, untransformed RGB, greyscale"""
    out, seed = [], 0
    for (w, h), ss, q, kind in itertools.product(SIZES, (0, 1, 2), (30, 75, 95), ('noise', 'he')):
        seed += 1
        out.append(('%dx%d ss%d q%d %s' % (w, h, ss, q, kind), TF.encode(_content(kind, h, w, seed), q, ss)))
    for (w, h), ss, kind in itertools.product(SIZES, (0, 1, 2), ('noise', 'he')):
        seed += 1
        out.append(('%dx%d ss%d restart %s' % (w, h, ss, kind), TF.encode(_content(kind, h, w, seed), 75, ss, restart=3)))
    for (w, h), kind in itertools.product(SIZES, ('noise', 'he')):
        seed += 1
        out.append(('%dx%d rgb %s' % (w, h, kind), TF.encode(_content(kind, h, w, seed), 75, 0, rgb=True)))
        out.append(('%dx%d rgb restart %s' % (w, h, kind), TF.encode(_content(kind, h, w, seed), 90, 0, restart=3, rgb=True)))
        out.append(('%dx%d grey %s' % (w, h, kind), TF.encode(_content(kind, h, w, seed, 1), 75)))
        out.append(('%dx%d grey restart %s' % (w, h, kind), TF.encode(_content(kind, h, w, seed, 1), 40, restart=2)))
    return out


@pytest.fixture(scope='module')
def matrix():
    return _matrix()


def test_oracle_equals_pillow(matrix):
    assert len(matrix) >= 93
    for name, s in matrix:
        ref = np.asarray(Image.open(io.BytesIO(s)).convert('RGB'))
        got = O.decode(s)
        assert got.shape == ref.shape and int((got != ref).sum()) == 0, name


# ------------------------------------------------------------------------------------------------------------------------ TiffSlide
VARIANTS = list(itertools.product((False, True), ('<', '>'), (True, False), (6, 2), (False, True)))   # big, endian, tables, photometric, strip


@pytest.fixture(scope='module')
def pyramid():
    return TF.pyramid(150, 200, 3, seed=1)


def _compose(slide, k, transform):
    """the level from the oracle's decode of every tile"""
    lv = slide.levels[k]
    tb = O.parse_tables(lv.tables) if lv.tables else None
    full = np.zeros((lv.rows * lv.tile_h, lv.cols * lv.tile_w, 3), np.uint8)
    for i in range(lv.rows * lv.cols):
        y, x = (i // lv.cols) * lv.tile_h, (i % lv.cols) * lv.tile_w
        data = bytes(slide.tile_bytes(k, i))
        full[y:y + lv.tile_h, x:x + lv.tile_w] = O.decode(data, tb, transform=transform) if data else 255
    return full[:lv.height, :lv.width]


@pytest.mark.parametrize('big,endian,tables,photometric,strip', VARIANTS)
def test_tiffslide_levels_equal_libtiff(tmp_path, pyramid, big, endian, tables, photometric, strip):
    path = str(tmp_path / 'p.tif')
    info = TF.write_tiff(path, pyramid, big=big, endian=endian, jpegtables=tables, photometric=photometric, strip=strip, thumbnail=True)
    try:
        ref = TF.pillow_levels(path, info['frames'])
    except Exception:
        ref = None                                              # a container Pillow does not open: the per-tile composition stands in
    s = TiffSlide(path)
    try:
        assert s.level_count == 3 and s.name == 'p.tif'          # the stripped directory is no level
        assert s.level_dimensions == tuple((l.shape[1], l.shape[0]) for l in pyramid) and s.dimensions == (200, 150)
        assert s.level_downsamples == tuple((200 / l.shape[1] + 150 / l.shape[0]) / 2 for l in pyramid)
        for k, (w, h) in enumerate(s.level_dimensions):
            got = np.asarray(s.read_region((0, 0), k, (w, h)))
            assert got.shape == (h, w, 4) and (got[..., 3] == 255).all()
            want = ref[k] if ref is not None else _compose(s, k, photometric == 6)
            assert int((got[..., :3] != want).sum()) == 0, k
            if ref is not None and k == 2:
                assert int((_compose(s, k, photometric == 6) != want).sum()) == 0
    finally:
        s.close()
    if not (big and endian == '>'):
        assert ref is not None                                  # Pillow opens every variant but big-endian BigTIFF


def test_read_region_offsets_border_and_empty_tile(tmp_path, pyramid):
    path = str(tmp_path / 'r.tif')
    TF.write_tiff(path, pyramid, tile=(64, 48), empty={(0, 5), (1, 0)})
    s = TiffSlide(path)
    full = [np.asarray(s.read_region((0, 0), k, s.level_dimensions[k]))[..., :3] for k in range(3)]
    assert (full[0][48:96, 64:128] == 255).all() and (full[1][:48, :64] == 255).all()          # tile 5 of a 4-column grid: row 1, column 1
    nonempty = _compose(s, 0, True)
    assert int((full[0] != nonempty).sum()) == 0
    for k, (x, y, w, h) in itertools.product(range(3), ((60, 40, 10, 20), (0, 0, 64, 48), (63, 47, 2, 2), (-7, -5, 30, 30), (30, 20, 400, 300))):
        ds = s.level_downsamples[k]
        img = np.asarray(s.read_region((int(x * ds) if x >= 0 else x * 4, int(y * ds) if y >= 0 else y * 4), k, (w, h)))
        lx, ly = (int(int(x * ds) // ds), int(int(y * ds) // ds)) if x >= 0 else (int((x * 4) // ds), int((y * 4) // ds))
        W, H = s.level_dimensions[k]
        want = np.zeros((h, w, 4), np.uint8)
        y0, y1, x0, x1 = max(ly, 0), min(ly + h, H), max(lx, 0), min(lx + w, W)
        if y1 > y0 and x1 > x0:
            want[y0 - ly:y1 - ly, x0 - lx:x1 - lx, :3] = full[k][y0:y1, x0:x1]
            want[y0 - ly:y1 - ly, x0 - lx:x1 - lx, 3] = 255
        assert np.array_equal(img, want), (k, x, y, w, h)
    s.close()


def test_photometric_rgb_without_markers_stays_untransformed(tmp_path):
    lv = [TF.he_like(96, 128, 3)]
    path = str(tmp_path / 'rgb.tif')
    info = TF.write_tiff(path, lv, photometric=2, strip=True, jpegtables=True)
    assert b'JFIF' not in info['streams'][0][0] and b'Adobe' not in info['streams'][0][0]
    s = TiffSlide(path)
    got = np.asarray(s.read_region((0, 0), 0, (128, 96)))[..., :3]
    s.close()
    assert int((got != TF.pillow_levels(path, info['frames'])[0]).sum()) == 0
    assert np.abs(got.astype(int) - lv[0]).mean() < 6           # the planes are R, G, B: a YCbCr -> RGB transform would be far off


@pytest.mark.parametrize('compression', (5, 33005, 33003))
def test_unsupported_compression_names_tag_and_value(tmp_path, compression):
    path = str(tmp_path / 'c.tif')
    TF.write_tiff(path, [TF.he_like(48, 64, 0)], compression=compression)
    with pytest.raises(ValueError, match=r'tag 259 .*%d' % compression):
        TiffSlide(path)


def test_open_slide_returns_tiffslide_without_openslide(tmp_path):
    try:
        import openslide                                       # noqa: F401
        pytest.skip('OpenSlide is importable: open_slide keeps using it')
    except ImportError:
        pass
    from utils import dataset as D
    path = str(tmp_path / 'case.svs')
    TF.write_tiff(path, TF.pyramid(96, 128, 2, seed=2))
    s = D.open_slide(path)
    assert isinstance(s, TiffSlide) and s.level_count == 2
    assert D.open_slide(s) is s
    s.close()


# ------------------------------------------------------------------------------------------------------------------ the marker walk
def _walk(lib, streams, tables=None, cap=64):
    from wsi_segmentation_pipeline_amd import ingest
    buf = np.frombuffer(b'\xaa' * 3 + b''.join(streams) + b'\xbb' * 5, np.uint8)
    lens = np.array([len(s) for s in streams], np.uint64)
    offs = 3 + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    base = None
    if tables is not None:
        rc, base = ingest.jpeg_parse_tables(tables)
        assert rc == 0
    rec, sets, n_sets = ingest.jpeg_walk(buf, offs, lens, base, cap)
    return rec, sets, n_sets, offs


def _huff_lookup(counts, symbols):
    look, code, k = np.zeros(512, np.uint16), 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            if l <= 9:
                look[code << (9 - l):(code + 1) << (9 - l)] = (l << 8) | symbols[k]
            code, k = code + 1, k + 1
        code <<= 1
    return look


def test_walk_records_equal_oracle_parse(lib, matrix):
    streams = [s for _, s in matrix]
    rec, sets, n_sets, offs = _walk(lib, streams)
    assert 1 <= n_sets <= 12                                    # a set per quality and colour layout, shared by content
    for (name, s), r, off in zip(matrix, rec, offs):
        d = O.parse(s)
        nc = d['ncomp']
        assert r['status'] == 0, name
        assert (r['scan_off'], r['scan_len']) == (off + d['scan_off'], d['scan_len']), name
        assert (r['width'], r['height'], r['ncomp'], r['restart']) == (d['width'], d['height'], nc, d['restart']), name
        for key in ('h', 'v', 'tq', 'td', 'ta'):
            assert list(r[key][:nc]) == d[key], (name, key)
        t = sets[r['table_set']]
        for c in range(nc):
            assert t['qt_present'][d['tq'][c]] and list(t['qt'][d['tq'][c]]) == d['qt'][d['tq'][c]], name
            for cls, tid in ((0, d['td'][c]), (1, d['ta'][c])):
                h = t['huff'][2 * cls + tid]
                counts, symbols = d['huff'][(cls, tid)]
                assert np.array_equal(h['look'], _huff_lookup(counts, symbols)), name
                assert bytes(h['huffval'][:len(symbols)]) == bytes(symbols) and h['maxcode'][17] == 0x7fffffff


def test_walk_table_sets_shared_and_own(lib):
    a = [TF.he_like(48, 64, k) for k in range(4)]
    tables = TF.encode(a[0], 75, 2, streamtype=1)
    abbreviated = [TF.encode(x, 75, 2, streamtype=2) for x in a]
    own90 = [TF.encode(x, 90, 2) for x in a[:2]]
    own75 = TF.encode(a[2], 75, 2)                              # complete, the same tables as the blob: shares its set
    rec, sets, n_sets, _ = _walk(lib, abbreviated[:2] + own90 + abbreviated[2:] + [own75], tables)
    assert (rec['status'] == 0).all() and n_sets == 2
    assert list(rec['table_set']) == [0, 0, 1, 1, 0, 0, 0]
    rec, sets, n_sets, _ = _walk(lib, [TF.encode(a[0], q, 2) for q in (50, 60, 70, 80)], None, cap=3)
    assert list(rec['status']) == [0, 0, 0, O.TABLE_CAPACITY] and n_sets == 3
    rec, _, _, _ = _walk(lib, abbreviated[:1], None)            # abbreviated with no tables anywhere
    assert rec['status'][0] == O.MALFORMED


def _patch(stream, marker, at, value):
    i = stream.index(bytes([0xFF, marker]))
    return stream[:i + at] + bytes([value]) + stream[i + at + 1:]


def test_walk_status_codes(lib):
    img = TF.he_like(32, 32, 9)
    good = TF.encode(img, 75, 2)
    cmyk = io.BytesIO()
    Image.fromarray(np.dstack([img, img[..., :1]]), 'CMYK').save(cmyk, 'JPEG')
    two_scans = good[:-2] + good[good.index(b'\xff\xda'):]
    cases = [
        (TF.encode(img, 75, 2, progressive=True), O.PROGRESSIVE),
        (_patch(good, 0xC0, 1, 0xC9), O.ARITHMETIC),
        (_patch(good, 0xC0, 4, 12), O.PRECISION),
        (cmyk.getvalue(), O.COMPONENTS),
        (_patch(good, 0xC0, 11, 0x12), O.SAMPLING),            # luma 1 x 2
        (_patch(good, 0xC0, 14, 0x21), O.SAMPLING),            # chroma 2 x 1
        (two_scans, O.MULTISCAN),
        (good[:len(good) // 2], O.MALFORMED),                   # the scan runs into the end
        (good[:30], O.MALFORMED),                               # a segment runs into the end
        (good[:-2], O.MALFORMED),                               # no EOI
        (b'\x00' + good[1:], O.MALFORMED),
        (b'', O.EMPTY),
        (good, O.OK),
    ]
    rec, _, _, _ = _walk(lib, [s for s, _ in cases])
    assert [int(v) for v in rec['status']] == [st for _, st in cases]
    for s, st in cases[:7]:
        with pytest.raises(O.Unsupported) as e:
            O.parse(s)
        assert e.value.status == st
    assert {int(m) for m in native.JpegStatus} == set(O.STATUS_NAMES)


def test_entries_declared_mirrored_and_checked(lib):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read(), flags=re.S)
    names = {'wsi_jpeg_tables_bytes', 'wsi_jpeg_tile_bytes', 'wsi_jpeg_parse_tables', 'wsi_jpeg_walk', 'wsi_jpeg_workspace_bytes',
             'wsi_jpeg_entropy', 'wsi_jpeg_reconstruct'}
    assert names == set(re.findall(r'\b(wsi_jpeg_[a-z0-9_]+)\s*\(', hdr)) == {n for n in native.SIGNATURES if n.startswith('wsi_jpeg_')}
    for n in names:
        assert hasattr(lib, n)
    for m in native.JpegStatus:
        assert int(re.search(r'WSI_JPEG_%s = (\d+)' % m.name, hdr).group(1)) == int(m)
    assert lib.wsi_jpeg_tables_bytes() == C.sizeof(native.WsiJpegTables) and lib.wsi_jpeg_tile_bytes() == C.sizeof(native.WsiJpegTile) == 48
    assert int(re.search(r'#define WSI_HIP_ABI_VERSION (\d+)', hdr).group(1)) == native.ABI_VERSION
    # workspace: int16 coefficients + u8 planes over whole MCUs, each rounded to 256 bytes
    assert lib.wsi_jpeg_workspace_bytes(240, 240, 3, 2, 1) == 2 * 240 * 240 * 2 + 2 * 240 * 240
    assert lib.wsi_jpeg_workspace_bytes(40, 56, 3, 2, 2) == (48 * 64 + 2 * 24 * 32) * 3
    assert lib.wsi_jpeg_workspace_bytes(8, 8, 1, 1, 1) == 512
    for bad in ((0, 8, 3, 1, 1), (8, 4097, 3, 1, 1), (8, 8, 2, 1, 1), (8, 8, 3, 1, 2), (8, 8, 1, 2, 1), (8, 8, 4, 1, 1)):
        assert lib.wsi_jpeg_workspace_bytes(*bad) == 0
    t = native.WsiJpegTables()
    blob = np.frombuffer(TF.encode(TF.he_like(8, 8, 0), streamtype=1), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.wsi_jpeg_parse_tables(p(blob), blob.size, C.byref(t)) == 0 and list(t.qt_present) == [1, 1, 0, 0] and list(t.huff_present) == [1] * 4
    assert lib.wsi_jpeg_parse_tables(None, 4, C.byref(t)) == -22 and lib.wsi_jpeg_parse_tables(p(blob), blob.size, None) == -22
    assert lib.wsi_jpeg_parse_tables(p(blob), 10, C.byref(t)) == O.MALFORMED
    off, ln = np.array([0], np.uint64), np.array([blob.size], np.uint32)
    rec, sets, cnt = np.zeros(1, np.dtype(native.WsiJpegTile)), np.zeros(2, np.dtype(native.WsiJpegTables)), C.c_int(0)
    walk = lambda *a: lib.wsi_jpeg_walk(*a)
    assert walk(p(blob), blob.size, p(off), p(ln), 1, None, p(sets), 2, C.byref(cnt), p(rec)) == 0
    assert walk(None, blob.size, p(off), p(ln), 1, None, p(sets), 2, C.byref(cnt), p(rec)) == -22
    assert walk(p(blob), blob.size, p(off), p(ln), 0, None, p(sets), 2, C.byref(cnt), p(rec)) == -22
    assert walk(p(blob), blob.size, p(off), p(ln), 1, None, p(sets), 0, C.byref(cnt), p(rec)) == -22
    assert walk(p(blob), blob.size - 1, p(off), p(ln), 1, None, p(sets), 2, C.byref(cnt), p(rec)) == -22       # a stream outside the buffer
    # device entries: every check comes before any device work, so they answer without a GPU.  Fake, aligned addresses.
    A = C.c_void_p(1 << 20)
    ws_bytes = lib.wsi_jpeg_workspace_bytes(64, 48, 3, 2, 2) * 4
    ent = lambda **k: lib.wsi_jpeg_entropy(k.get('bytes', A), 100, k.get('tiles', A), k.get('n', 4), k.get('sets', A), k.get('n_sets', 1), k.get('common', 0),
                                           k.get('w', 64), 48, 3, 2, 2, k.get('ws', A), k.get('ws_bytes', ws_bytes), k.get('status', A), k.get('lanes', 0), None)
    for k in (dict(bytes=None), dict(tiles=None), dict(sets=None), dict(ws=None), dict(status=None), dict(n=0), dict(n_sets=0), dict(common=1),
              dict(w=0), dict(ws=C.c_void_p((1 << 20) + 8)), dict(ws_bytes=ws_bytes - 1), dict(lanes=-1), dict(lanes=65)):
        assert ent(**k) == -22, k
    rcn = lambda **k: lib.wsi_jpeg_reconstruct(k.get('ws', A), k.get('ws_bytes', ws_bytes), k.get('status', A), k.get('cells', A), k.get('n', 4), 64, 48, 3, 2, 2,
                                               k.get('transform', 1), k.get('cols', 4), k.get('rows', 4), k.get('level', A), k.get('pitch', 600), k.get('H', 150),
                                               k.get('W', 200), None)
    for k in (dict(ws=None), dict(status=None), dict(cells=None), dict(level=None), dict(n=0), dict(ws=C.c_void_p((1 << 20) + 4)), dict(ws_bytes=16),
              dict(transform=2), dict(pitch=599), dict(H=0), dict(cols=0), dict(W=192), dict(H=144), dict(cols=5), dict(rows=5)):
        assert rcn(**k) == -22, k                                # W = 192 / H = 144: the grid's last column / row starts outside the level


def _resize_frame(stream, width, height):
    """the stream with the frame header's dimensions overwritten (the scan no longer fits them: for the walk alone)"""
    i = stream.index(b'\xff\xc0')
    return stream[:i + 5] + struct.pack('>HH', height, width) + stream[i + 9:]


def test_walk_and_workspace_stop_at_4096(lib):
    """MAX_DIM: the walk takes a frame of 4096 in either dimension and refuses 4097; wsi_jpeg_workspace_bytes answers 0 for it"""
    good = TF.encode(TF.he_like(16, 16, 3), 75, 2)
    assert _resize_frame(good, 16, 16) == good
    cases = [(4096, 16, O.OK), (16, 4096, O.OK), (4096, 4096, O.OK), (4097, 16, O.MALFORMED), (16, 4097, O.MALFORMED), (65535, 65535, O.MALFORMED)]
    rec, _, _, _ = _walk(lib, [_resize_frame(good, w, h) for w, h, _ in cases])
    assert [int(v) for v in rec['status']] == [st for _, _, st in cases]
    assert [(int(r['width']), int(r['height'])) for r in rec[:3]] == [c[:2] for c in cases[:3]]
    for ss, (hs, vs) in enumerate(((1, 1), (2, 1), (2, 2))):
        for w, h in ((4096, 16), (16, 4096)):
            mw, mh = -(-w // (8 * hs)) * 8 * hs, -(-h // (8 * vs)) * 8 * vs
            assert lib.wsi_jpeg_workspace_bytes(w, h, 3, hs, vs) == 3 * (mw * mh + 2 * (mw // hs) * (mh // vs))
        assert lib.wsi_jpeg_workspace_bytes(4097, 16, 3, hs, vs) == 0 and lib.wsi_jpeg_workspace_bytes(16, 4097, 3, hs, vs) == 0


def test_optimised_tables_fixture_and_walk(lib, tmp_path):
    """TF.encode / TF.write_tiff(optimize=True): off by default (every other stream keeps its bytes), the oracle equals Pillow on such
    streams, the walk keeps a set per stream and its slow-path tables (maxcode, valoffset, huffval) decode every code of more than 9
    bits to the oracle's symbol; the colour forms of the bad scan streams keep the header of a good one."""
    img = TF.noise(64, 48, 5)
    assert TF.encode(img, 90, 2) == TF.encode(img, 90, 2, optimize=False) != TF.encode(img, 90, 2, optimize=True)
    streams = [TF.encode(TF.noise(64, 48, 60 + k) if k % 2 else TF.he_like(64, 48, 60 + k), (75, 95)[k % 2], k % 3, restart=(0, 3)[k // 3], optimize=True)
               for k in range(6)]
    rec, sets, n_sets, _ = _walk(lib, streams)
    assert (rec['status'] == 0).all() and n_sets == 6 and list(rec['table_set']) == list(range(6))
    long_codes = 0
    for s, r in zip(streams, rec):
        d = O.parse(s)
        assert int((O.decode(s) != np.asarray(Image.open(io.BytesIO(s)).convert('RGB'))).sum()) == 0
        for (cls, tid), (counts, symbols) in d['huff'].items():
            h = sets[r['table_set']]['huff'][2 * cls + tid]
            assert np.array_equal(h['look'], _huff_lookup(counts, symbols))
            for (length, code), sym in O._code_table(counts, symbols).items():
                if length > 9:
                    long_codes += 1
                    assert h['look'][code >> (length - 9)] == 0                              # the look-up sends it to the slow path
                    assert h['maxcode'][length - 1] < (code >> 1) and code <= h['maxcode'][length]   # which stops at this length
                    assert h['huffval'][(code + h['valoffset'][length]) & 255] == sym
    assert long_codes > 0
    path = str(tmp_path / 'opt.tif')
    lv = TF.noise(96, 128, 8)
    info = TF.write_tiff(path, [lv], jpegtables=False, optimize=True)
    plain = TF.write_tiff(str(tmp_path / 'plain.tif'), [lv], jpegtables=False)
    assert all(a != b and len(a) < len(b) for a, b in zip(info['streams'][0], plain['streams'][0]))
    s = TiffSlide(path)
    assert int((np.asarray(s.read_region((0, 0), 0, (128, 96)))[..., :3] != TF.pillow_levels(path, info['frames'])[0]).sum()) == 0
    s.close()
    with pytest.raises(AssertionError):
        TF.write_tiff(path, [lv], optimize=True)                # abbreviated streams cannot carry tables of their own
    grey = TF.bad_scan_streams()
    assert list(grey) == ['exhausted', 'bad_code', 'coef_overrun', 'short', 'zrl_end']
    for ss in (0, 1, 2):
        bad = TF.bad_scan_streams(ss)
        assert list(bad) == ['exhausted', 'bad_code', 'coef_overrun'] and [v[1] for v in bad.values()] == [v[1] for v in list(grey.values())[:3]]
        rec, _, _, _ = _walk(lib, [v[0] for v in bad.values()])
        assert (rec['status'] == 0).all()                       # the damage is in the scan; the frame is a 16 x 16 colour tile's
        assert all((r['width'], r['height'], r['ncomp'], r['h'][0], r['v'][0]) == (16, 16, 3, (1, 2, 2)[ss], (1, 1, 2)[ss]) for r in rec)


# ------------------------------------------------------------------------------------------------ the decode loop under sanitizers
def _fixture_streams():
    """(tables or b'', stream) of every valid kind the fixtures make: complete and abbreviated, the three sub-samplings, grey, restart"""
    out = []
    for k, ((w, h), ss) in enumerate(itertools.product(((40, 56), (16, 16), (64, 48)), (0, 1, 2))):
        img = TF.he_like(h, w, 20 + k) if k % 2 else TF.noise(h, w, 20 + k)
        out.append((b'', TF.encode(img, (30, 75, 95)[k % 3], ss, restart=(0, 3)[k % 2])))
        out.append((TF.encode(img, 75, ss, streamtype=1), TF.encode(img, 75, ss, streamtype=2, strip=True)))
    out.append((b'', TF.encode(TF.he_like(37, 53, 40, 1), 75)))
    out.append((b'', TF.encode(TF.noise(24, 24, 41, 1), 50, restart=2)))
    return out


def sanitizer_corpus():
    """[(tables, stream, expected status or None, expects coefficients)]: every valid stream, each truncated at 16 evenly spaced
    lengths (bare, and with an EOI put back so that the decode loop and not the walk meets the cut), single bytes of the scan data and
    of the Huffman and quantisation tables overwritten (fixed seed), and the four streams built to fail in the loop."""
    rng = np.random.default_rng(1234)
    valid = _fixture_streams()
    cases = [(t, s, 0) for t, s in valid]
    for t, s in valid:
        for k in range(16):
            cut = 2 + (len(s) - 3) * k // 15
            cases.append((t, s[:cut], None))
            cases.append((t, s[:cut] + b'\xff\xd9', None))
    for n in range(320):
        t, s = valid[n % len(valid)]
        d = O.parse(s, O.parse_tables(t) if t else None)
        s2, t2 = bytearray(s), bytearray(t)
        if n % 4 != 3:
            s2[d['scan_off'] + int(rng.integers(0, d['scan_len']))] = int(rng.integers(0, 256))
        else:                                                   # inside a DHT (or, every other time, DQT) segment, of the stream or of the table blob
            tgt = t2 if t else s2
            i = bytes(tgt).index(b'\xff\xdb' if n % 8 == 7 else b'\xff\xc4')
            ln = struct.unpack('>H', bytes(tgt[i + 2:i + 4]))[0]
            tgt[i + 4 + int(rng.integers(0, ln - 2))] = int(rng.integers(0, 256))
        cases.append((bytes(t2), bytes(s2), None))
    cases += [(b'', s, st) for s, st in TF.bad_scan_streams().values()]
    cases += [(b'', s, st) for ss in (0, 1, 2) for s, st in TF.bad_scan_streams(ss).values()]      # their three-component forms
    return cases


@pytest.fixture(scope='module')
def sanitizer_run(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('san')
    exe = str(d / 'jpeg_san')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
           os.path.join(ROOT, 'tests', 'jpeg_san_main.cpp'), '-o', exe]
    if os.path.basename(cxx) == 'g++':
        cmd += ['-static-libasan', '-static-libubsan']          # the runtimes inside the program: nothing has to be preloaded or come first
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode:
        if re.search(r'cannot find .*(asan|ubsan)|libasan|libubsan', res.stdout):
            pytest.skip('the sanitizer runtime is not installed')
        raise AssertionError(res.stdout)
    cases = sanitizer_corpus()
    with open(d / 'corpus.bin', 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for t, s, _ in cases:
            f.write(struct.pack('<I', len(t)) + t + struct.pack('<I', len(s)) + s)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    res = subprocess.run([exe, str(d / 'corpus.bin'), str(d / 'results.bin')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0, res.stdout[-4000:]
    raw = open(d / 'results.bin', 'rb').read()
    results, at = [], 0
    for _ in cases:
        st, n = struct.unpack('<ii', raw[at:at + 8])
        results.append((st, np.frombuffer(raw, '<i2', n, at + 8)))
        at += 8 + 2 * n
    assert at == len(raw)
    return cases, results


def test_sanitized_decode_loop_has_a_status_for_every_case(sanitizer_run):
    cases, results = sanitizer_run
    assert len(results) == len(cases) >= 800
    known = set(O.STATUS_NAMES)
    seen = set()
    for (t, s, want), (st, coef) in zip(cases, results):
        assert st in known
        seen.add(st)
        if want is not None:
            assert st == want
    assert {O.OK, O.MALFORMED, O.BAD_CODE, O.COEF_OVERRUN, O.SHORT, O.EXHAUSTED} <= seen


def test_sanitized_decode_loop_equals_oracle_coefficients(sanitizer_run):
    """the coefficients of the shared decode loop (the entropy kernel's source, run on the host) equal the oracle's, stream by stream;
    a damaged stream that still decodes on both sides gives the same coefficients too"""
    cases, results = sanitizer_run
    checked = 0
    for (t, s, want), (st, coef) in zip(cases, results):
        if st != 0:
            continue
        try:
            d, ref = O.decode_coefficients(s, O.parse_tables(t) if t else None)
        except (O.Unsupported, KeyError, IndexError):
            assert want is None                                 # the oracle is stricter on a damaged table; never on a valid stream
            continue
        flat = np.concatenate([c.reshape(-1) for c in ref])
        if want == 0:
            assert np.array_equal(coef, flat)
            checked += 1
        elif np.abs(flat).max() <= 32767:
            assert np.array_equal(coef, flat)
    assert checked == len(_fixture_streams()) + 1                # + the stream whose ZRL ends its blocks
