"""CPU side of the JPEG encode path: the spec (tests/jpeg_enc_oracle.py) against Pillow - quantised coefficients and scan bytes, 0
differences - over a corpus that reaches the hard symbols, the library's quality tables against Pillow's, the C-ABI entries and
their argument checks, the container written by tiffwrite.write_pyramid with the spec standing in for the device encode (read back by
Pillow's libtiff and by TiffSlide), and the shared entropy loop as a stand-alone program under the host sanitizers."""
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
import jpeg_enc_oracle as E                                    # noqa: E402
import jpeg_oracle as O                                        # noqa: E402
import tiff_fixture as TF                                      # noqa: E402
from wsi_segmentation_pipeline_amd import native, tiffwrite as TW   # noqa: E402
from wsi_segmentation_pipeline_amd.tiffslide import TiffSlide   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ((16, 16), (64, 48), (32, 112))                         # (width, height)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


def _content(kind, h, w, seed, channels=3):
    return (TF.noise if kind == 'noise' else TF.he_like)(h, w, seed, channels)


def extreme_tile():
    """16 x 16 grey: a black block beside a white one (a DC difference of size 11 at quality 100), a 0 / 255 checkerboard (AC
    coefficients of size 10), a flat block"""
    t = np.zeros((16, 16), np.uint8)
    t[:8, 8:] = 255
    t[8:, :8] = ((np.add.outer(np.arange(8), np.arange(8)) & 1) * 255).astype(np.uint8)
    t[8:, 8:] = 77
    return t


def ff00_tail_seed():
    """the first seed whose 16 x 16 grey noise tile at quality 75 ends its scan in FF 00 (a stuffed last byte), or None"""
    for seed in range(400):
        s = TF.encode(TF.noise(16, 16, seed, 1), 75)
        d = O.parse(s)
        if s[d['scan_off']:d['scan_off'] + d['scan_len']].endswith(b'\xff\x00'):
            return seed
    return None


def _corpus():
    """[(name, image, quality, sampling index or None for grey, restart)]"""
    out, seed = [], 0
    for (w, h), ss, q, kind in itertools.product(SMALL, (0, 1, 2), (30, 75, 100), ('noise', 'he')):
        seed += 1
        out.append(('%dx%d ss%d q%d %s' % (w, h, ss, q, kind), _content(kind, h, w, seed), q, ss, 0))
    for (w, h), q, kind in itertools.product(SMALL, (30, 75, 100), ('noise', 'he')):
        seed += 1
        out.append(('%dx%d grey q%d %s' % (w, h, q, kind), _content(kind, h, w, seed, 1), q, None, 0))
    for (w, h), ss, kind in itertools.product(SMALL, (0, 1, 2), ('noise', 'he')):
        seed += 1
        hs = E.SAMPLINGS[ss][0]
        for r, what in ((1, 'every MCU'), (w // (8 * hs), 'every MCU row')):
            out.append(('%dx%d ss%d restart %s %s' % (w, h, ss, what, kind), _content(kind, h, w, seed), 70, ss, r))
    for (w, h) in SMALL:
        seed += 1
        out.append(('%dx%d grey restart' % (w, h), TF.noise(h, w, seed, 1), 80, None, w // 8))
    for ss, kind, q in ((0, 'he', 75), (1, 'he', 30), (2, 'he', 75), (2, 'noise', 100), (1, 'noise', 75), (None, 'he', 75), (2, 'he', 70)):
        seed += 1
        out.append(('256x256 ss%s q%d %s' % (ss, q, kind), _content(kind, 256, 256, seed, 1 if ss is None else 3), q, ss, 16 if q == 70 else 0))
    out.append(('white', np.full((64, 48, 3), 255, np.uint8), 75, 2, 0))
    out.append(('extreme', extreme_tile(), 100, None, 0))
    tail = ff00_tail_seed()
    if tail is not None:
        out.append(('ff00 tail', TF.noise(16, 16, tail, 1), 75, None, 0))
    return out


@pytest.fixture(scope='module')
def corpus():
    """(name, image, sampling, restart, Pillow's stream, its header dict, its scan bytes) per case"""
    out = []
    for name, img, q, ss, restart in _corpus():
        s = TF.encode(img, q, 0 if ss is None else ss, restart)
        d = O.parse(s)
        out.append((name, img, (1, 1) if ss is None else E.SAMPLINGS[ss], restart, s, d, s[d['scan_off']:d['scan_off'] + d['scan_len']]))
    return out


def test_spec_equals_pillow_coefficients_and_scan_bytes(corpus):
    assert len(corpus) >= 96
    coef_total = 0
    for name, img, sampling, restart, s, d, scan in corpus:
        assert d['restart'] == restart and (d['h'][0], d['v'][0]) == sampling, name
        qt = [np.asarray(Image.open(io.BytesIO(s)).quantization[i]) for i in range(2 if img.ndim == 3 else 1)]
        _, ref = O.decode_coefficients(s)
        coefs, got = E.encode_tile(img, (qt[0], qt[-1]), sampling, restart)
        for c in range(len(ref)):
            assert int((coefs[c] * qt[min(c, 1)] != ref[c]).sum()) == 0, name
            coef_total += ref[c].size
        assert got == scan, name
    assert coef_total > 1000000


def test_corpus_reaches_the_hard_symbols(corpus):
    """asserted on PILLOW's streams: byte stuffing, ZRL, a block that is EOB only, an AC coefficient of size 10 and a DC difference of
    size 11, a scan whose last byte is a stuffed FF"""
    stuffed = zrl = eob_only = big_ac = big_dc = tail = 0
    for name, img, sampling, restart, s, d, scan in corpus:
        stuffed += b'\xff\x00' in scan
        tail += scan.endswith(b'\xff\x00')
        if name.startswith('256'):
            continue                                            # the small streams reach every symbol; their coefficients are quick to walk
        qt = [np.asarray(d['qt'][t], np.int64) for t in d['tq']]
        _, ref = O.decode_coefficients(s)
        for c, blocks in enumerate(ref):
            v = (blocks // qt[c][O.ZIGZAG.argsort()]).reshape(-1, 64)[:, O.ZIGZAG]       # quantised, zigzag
            big_ac += int((np.abs(v[:, 1:]) >= 512).any())
            eob_only += int(((v[:, 1:] == 0).all(1) & (np.diff(v[:, 0], prepend=0) == 0)).any()) if not restart else 0
            for blk in v:
                nz = np.nonzero(blk[1:])[0]
                zrl += int(len(nz) > 0 and int(np.diff(np.concatenate([[-1], nz])).max()) > 16)
        if not restart and len(ref) == 1:
            dc = (ref[0][..., 0] // qt[0][0]).reshape(-1)
            big_dc += int((np.abs(np.diff(dc, prepend=0)) >= 1024).any())
    assert stuffed > 0 and zrl > 0 and eob_only > 0 and big_ac > 0 and big_dc > 0
    assert ff00_tail_seed() is not None and tail > 0            # found among the seeds: a real Pillow stream, nothing built by hand


def test_quality_tables_equal_pillow(lib):
    for q in (1, 25, 50, 75, 95, 100):
        im = Image.open(io.BytesIO(TF.encode(TF.he_like(16, 16, q), q, 2)))
        lum, chrom = TW.quality_tables(q)
        assert list(lum) == list(im.quantization[0]) and list(chrom) == list(im.quantization[1]), q
        assert all(np.array_equal(a, b) for a, b in zip((lum, chrom), E.quality_tables(q)))
    assert [list(t) for t in TW.quality_tables(0)] == [list(t) for t in TW.quality_tables(1)]
    assert [list(t) for t in TW.quality_tables(101)] == [list(t) for t in TW.quality_tables(100)] == [[1] * 64] * 2
    for k in range(4):
        counts, symbols = TW.std_huff(k)
        assert (list(counts), list(symbols)) == E.STD_HUFF[k]
    # the markers this module writes are the ones Pillow writes around the same scan
    img = TF.he_like(48, 64, 3)
    s, t = TF.encode(img, 60, 1, streamtype=2, strip=True), TF.encode(img, 60, 1, streamtype=1)
    d = O.parse(s, O.parse_tables(t))
    assert TW.tile_header(64, 48, 3, (2, 1)) == s[:d['scan_off']] and TW.jpeg_tables(TW.quality_tables(60), 3) == t
    g = TF.encode(img[..., 0], 60, streamtype=2, strip=True, restart=4)
    assert TW.tile_header(64, 48, 1, (2, 2), restart=4) == g[:O.parse(g, O.parse_tables(t))['scan_off']]
    # one component: libjpeg lists the chroma tables as well; this module writes the tables the component uses, with the same content
    ours, theirs = O.parse_tables(TW.jpeg_tables(TW.quality_tables(60), 1)), O.parse_tables(TF.encode(img[..., 0], 60, streamtype=1))
    assert set(ours['qt']) == {0} and set(ours['huff']) == {(0, 0), (1, 0)}
    assert ours['qt'][0] == theirs['qt'][0] and all(ours['huff'][k] == theirs['huff'][k] for k in ours['huff'])


def test_entries_declared_mirrored_and_checked(lib):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read(), flags=re.S)
    names = {'wsi_jenc_quality_tables', 'wsi_jenc_std_huff', 'wsi_jenc_workspace_bytes', 'wsi_jenc_transform', 'wsi_jenc_entropy_size',
             'wsi_jenc_entropy_write', 'wsi_jenc_downsample'}
    assert names == set(re.findall(r'\b(wsi_jenc_[a-z0-9_]+)\s*\(', hdr)) == {n for n in native.SIGNATURES if n.startswith('wsi_jenc_')}
    for n in names:
        assert hasattr(lib, n)
    assert {n for n in native.SIGNATURES if n.startswith('wsi_jpeg_')} == {
        'wsi_jpeg_tables_bytes', 'wsi_jpeg_tile_bytes', 'wsi_jpeg_parse_tables', 'wsi_jpeg_walk', 'wsi_jpeg_workspace_bytes', 'wsi_jpeg_entropy',
        'wsi_jpeg_reconstruct'}
    assert int(re.search(r'#define WSI_HIP_ABI_VERSION (\d+)', hdr).group(1)) == native.ABI_VERSION == lib.wsi_hip_abi_version() == 9
    # workspace: int16 coefficients over whole MCUs, rounded to 256 bytes
    ws = lib.wsi_jenc_workspace_bytes
    assert ws(256, 256, 3, 2, 2) == 256 * 256 * 3 and ws(256, 256, 3, 2, 1) == 256 * 256 * 4 and ws(64, 48, 3, 1, 1) == 64 * 48 * 6
    assert ws(16, 16, 1, 1, 1) == 512 and ws(4096, 16, 1, 1, 1) == 4096 * 32
    for bad in ((0, 16, 3, 1, 1), (8, 16, 3, 1, 1), (24, 16, 3, 1, 1), (16, 40, 3, 1, 1), (4112, 16, 3, 1, 1), (16, 4112, 1, 1, 1), (16, 16, 2, 1, 1),
                (16, 16, 4, 1, 1), (16, 16, 3, 1, 2), (16, 16, 3, 2, 4), (16, 16, 1, 2, 1), (16, 16, 1, 2, 2)):
        assert ws(*bad) == 0, bad
    # every check comes before any device work, so the device entries answer without a GPU.  Fake, aligned addresses.
    A, p = C.c_void_p(1 << 20), lambda a: a.ctypes.data_as(C.c_void_p)
    q, q0 = np.full(64, 9, np.uint8), np.full(64, 9, np.uint8)
    q0[17] = 0
    assert lib.wsi_jenc_quality_tables(50, None, p(q)) == -22 and lib.wsi_jenc_quality_tables(50, p(q.copy()), None) == -22
    cnt = C.c_int(0)
    sym = np.zeros(256, np.uint8)
    assert lib.wsi_jenc_std_huff(4, p(sym), p(sym), C.byref(cnt)) == -22 and lib.wsi_jenc_std_huff(-1, p(sym), p(sym), C.byref(cnt)) == -22
    assert lib.wsi_jenc_std_huff(0, None, p(sym), C.byref(cnt)) == -22 and lib.wsi_jenc_std_huff(0, p(sym), None, C.byref(cnt)) == -22
    assert lib.wsi_jenc_std_huff(0, p(sym), p(sym), None) == -22
    tile_ws = ws(64, 48, 3, 2, 2)

    def tr(**k):                                                # a 200 x 150 level in 64 x 48 tiles: a 4 x 4 grid
        return lib.wsi_jenc_transform(k.get('level', A), k.get('pitch', 600), k.get('H', 150), k.get('W', 200), k.get('cols', 4), k.get('rows', 4),
                                      k.get('first', 0), k.get('n', 16), k.get('tw', 64), k.get('th', 48), k.get('nc', 3), k.get('hs', 2), k.get('vs', 2),
                                      p(k.get('ql', q)) if k.get('ql', q) is not None else None, p(k.get('qc', q)) if k.get('qc', q) is not None else None,
                                      k.get('ws', A), k.get('ws_bytes', 16 * tile_ws), None)
    for k in (dict(level=None), dict(ql=None), dict(qc=None), dict(ws=None), dict(n=0), dict(n=-1), dict(tw=72), dict(th=40), dict(tw=8), dict(tw=4112),
              dict(nc=2), dict(nc=4), dict(hs=1, vs=2), dict(hs=4), dict(nc=1), dict(ql=q0), dict(qc=q0), dict(pitch=599), dict(H=0), dict(W=0),
              dict(cols=0), dict(rows=0), dict(W=192), dict(H=144), dict(cols=5), dict(rows=5), dict(first=-1), dict(first=1), dict(n=17, ws_bytes=17 * tile_ws),
              dict(ws=C.c_void_p((1 << 20) + 8)), dict(ws_bytes=16 * tile_ws - 1)):
        assert tr(**k) == -22, k                                 # nc=1 alone: one component with 2x2 sampling

    def sz(**k):
        return lib.wsi_jenc_entropy_size(k.get('ws', A), k.get('ws_bytes', 16 * tile_ws), k.get('n', 16), k.get('tw', 64), 48, k.get('nc', 3), k.get('hs', 2), 2,
                                         k.get('restart', 0), k.get('sizes', A), k.get('lanes', 0), None)
    for k in (dict(ws=None), dict(sizes=None), dict(n=0), dict(tw=60), dict(nc=2), dict(hs=1), dict(restart=-1), dict(restart=65536), dict(lanes=-1),
              dict(lanes=65), dict(ws=C.c_void_p((1 << 20) + 4)), dict(ws_bytes=15 * tile_ws)):
        assert sz(**k) == -22, k
    off, size = np.arange(16, dtype=np.uint64) * 1024, np.full(16, 1000, np.uint32)
    far, long_ = off.copy(), size.copy()
    far[15], long_[3] = 16 * 1024 - 999, 16 * 1024 - 3 * 1024 + 1

    def wr(**k):
        o, s = k.get('off', off), k.get('size', size)
        return lib.wsi_jenc_entropy_write(k.get('ws', A), k.get('ws_bytes', 16 * tile_ws), k.get('n', 16), k.get('tw', 64), 48, 3, 2, k.get('vs', 2),
                                          k.get('restart', 0), p(o) if o is not None else None, p(s) if s is not None else None, k.get('ranges', A),
                                          k.get('out', A), k.get('out_bytes', 16 * 1024), k.get('lanes', 0), None)
    for k in (dict(ws=None), dict(off=None), dict(size=None), dict(ranges=None), dict(out=None), dict(n=0), dict(tw=0), dict(vs=3), dict(restart=-1),
              dict(lanes=65), dict(ranges=C.c_void_p((1 << 20) + 4)), dict(ws_bytes=1), dict(off=far), dict(size=long_), dict(out_bytes=16 * 1024 - 25)):
        assert wr(**k) == -22, k                                 # the last three: a range that leaves the output

    def dn(**k):
        return lib.wsi_jenc_downsample(k.get('src', A), k.get('sp', 300), k.get('H', 50), k.get('W', 100), k.get('c', 3), k.get('f', 2), k.get('dst', A),
                                       k.get('dp', 150), None)
    for k in (dict(src=None), dict(dst=None), dict(H=0), dict(W=0), dict(c=2), dict(f=3), dict(f=1), dict(sp=299), dict(dp=149), dict(H=1), dict(W=3, f=4)):
        assert dn(**k) == -22, k


def test_gpu_path_refuses_a_cpu_process_loudly():
    import torch
    lv = torch.zeros((32, 32, 3), dtype=torch.uint8)            # a host tensor: refused with or without a GPU in the machine
    for call in (lambda: TW.encode_level(lv), lambda: TW.write_pyramid(os.devnull, [lv]), lambda: TW.downsample_level(lv, 2),
                 lambda: TW.save_slide(None, os.devnull, device='cpu')):
        with pytest.raises(RuntimeError, match='GPU'):
            call()


# ------------------------------------------------------------------------------------------------------------------------ container
def spec_encode(level, tile, qtables, sampling, restart):
    """the spec in place of the device encode: one batch per tile row, edge tiles padded by np.pad(mode='edge')"""
    tw, th = tile
    padded = TF.pad_to_tiles(np.asarray(level), tw, th)
    cols, rows = padded.shape[1] // tw, padded.shape[0] // th
    for ty in range(rows):
        scans = [E.encode_tile(padded[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw], qtables, sampling, restart)[1] for tx in range(cols)]
        sizes = np.array([len(s) for s in scans], np.uint32)
        offsets = np.zeros(cols, np.uint64)
        np.cumsum((sizes[:-1].astype(np.uint64) + 15) // 16 * 16, out=offsets[1:])
        buf = np.full(int(offsets[-1]) + int(sizes[-1]), 0xA5, np.uint8)
        for o, s in zip(offsets, scans):
            buf[int(o):int(o) + len(s)] = np.frombuffer(s, np.uint8)
        yield ty * cols, sizes, offsets, buf


def _pillow_roundtrip(level, tile, quality, ss):
    """the level as Pillow decodes Pillow-encoded tiles of it (edge tiles padded by np.pad(mode='edge'))"""
    tw, th = tile
    padded = TF.pad_to_tiles(level, tw, th)
    out = np.zeros(padded.shape[:2] + (3,), np.uint8)
    for y in range(0, padded.shape[0], th):
        for x in range(0, padded.shape[1], tw):
            s = TF.encode(np.ascontiguousarray(padded[y:y + th, x:x + tw]), quality, ss)
            out[y:y + th, x:x + tw] = np.asarray(Image.open(io.BytesIO(s)).convert('RGB'))
    return out[:level.shape[0], :level.shape[1]]


@pytest.mark.parametrize('big', (False, True))
@pytest.mark.parametrize('ss', (0, 1, 2))
def test_container_opens_in_pillow_and_tiffslide(tmp_path, big, ss):
    levels = [TF.he_like(150, 200, 1), TF.he_like(70, 50, 2), TF.noise(10, 7, 3)]
    path = str(tmp_path / 'w.tif')
    rep = TW.write_pyramid(path, levels, tile=(32, 32), quality=80, subsampling=E.SAMPLINGS[ss], big=big, description='spec', mpp=0.5, encode=spec_encode)
    assert rep['big'] == big and rep['bytes'] == os.path.getsize(path) and rep['tiles'] == 7 * 5 + 2 * 3 + 1
    assert [(l['width'], l['height'], l['tiles']) for l in rep['levels']] == [(200, 150, 35), (50, 70, 6), (7, 10, 1)]
    assert open(path, 'rb').read(4) == (b'II\x2b\x00' if big else b'II\x2a\x00')
    want = [_pillow_roundtrip(l, (32, 32), 80, ss) for l in levels]
    got = TF.pillow_levels(path, [0, 1, 2])
    s = TiffSlide(path)
    try:
        assert s.level_count == 3 and s.level_dimensions == ((200, 150), (50, 70), (7, 10))
        assert s.level_downsamples == tuple((200 / w + 150 / h) / 2 for w, h in s.level_dimensions)
        for k, (w, h) in enumerate(s.level_dimensions):
            assert int((got[k] != want[k]).sum()) == 0, k
            assert int((np.asarray(s.read_region((0, 0), k, (w, h)))[..., :3] != want[k]).sum()) == 0, k
            assert s.levels[k].tables == TW.jpeg_tables(TW.quality_tables(80), 3)
            # the tile streams are the ones Pillow writes for the padded tiles (abbreviated, APP markers stripped)
            padded = TF.pad_to_tiles(levels[k], 32, 32)
            for i in range(s.levels[k].cols * s.levels[k].rows):
                y, x = i // s.levels[k].cols * 32, i % s.levels[k].cols * 32
                assert bytes(s.tile_bytes(k, i)) == TF.encode(np.ascontiguousarray(padded[y:y + 32, x:x + 32]), 80, ss, streamtype=2, strip=True), (k, i)
    finally:
        s.close()
    with Image.open(path) as im:
        assert im.tag_v2[270] == 'spec' and im.tag_v2[254] == 0 and im.tag_v2[259] == 7 and im.tag_v2[262] == 6
        assert tuple(im.tag_v2[530]) == E.SAMPLINGS[ss] and abs(float(im.tag_v2[282]) - 20000.0) < 1e-6 and im.tag_v2[296] == 3
        im.seek(1)
        assert im.tag_v2[254] == 1 and 270 not in im.tag_v2 and abs(float(im.tag_v2[282]) - 5000.0) < 1e-6


def test_container_grey_restart_and_own_tables(tmp_path):
    levels = [TF.he_like(70, 50, 4, 1), TF.noise(10, 7, 5, 1)]
    path = str(tmp_path / 'g.tif')
    q = (np.arange(1, 65), np.full(64, 255))
    rep = TW.write_pyramid(path, levels, tile=(32, 16), qtables=q, restart=2, encode=spec_encode)
    assert not rep['big'] and rep['tiles'] == 2 * 5 + 1
    s = TiffSlide(path)
    try:
        assert s.level_dimensions == ((50, 70), (7, 10)) and s.levels[0].samples == 1 and s.levels[0].photometric == 1
        for k, lv in enumerate(levels):
            padded = TF.pad_to_tiles(lv, 32, 16)
            for i in range(s.levels[k].cols * s.levels[k].rows):
                y, x = i // s.levels[k].cols * 16, i % s.levels[k].cols * 32
                d, coefs = O.decode_coefficients(bytes(s.tile_stream(k, i)))
                assert d['restart'] == 2 and d['qt'][0] == [int(v) for v in q[0][O.ZIGZAG]]
                assert np.array_equal(coefs[0], E.coefficients(padded[y:y + 16, x:x + 32], q)[0] * q[0])
        got = TF.pillow_levels(path, [0, 1])
        for k in range(2):
            w, h = s.level_dimensions[k]
            assert int((got[k] != np.asarray(s.read_region((0, 0), k, (w, h)))[..., :3]).sum()) == 0
    finally:
        s.close()
    with pytest.raises(ValueError):
        TW.write_pyramid(path, levels, tile=(32, 24), encode=spec_encode)
    with pytest.raises(ValueError):
        TW.write_pyramid(path, levels, qtables=(np.zeros(64), np.ones(64)), encode=spec_encode)
    with pytest.raises(ValueError):
        TW.write_pyramid(path, levels, downsample=2, encode=spec_encode)


# ------------------------------------------------------------------------------------------------ the encode loop under sanitizers
def sanitizer_corpus():
    """[(width, height, ncomp, hs, vs, restart, (MCUs, blocks, 64) int16 zigzag coefficients)]: the spec's coefficients of real tiles in
    every sampling with and without restart intervals, and tiles made of all-zero, all-maximum (DC and AC at +-1023, the largest
    values a baseline code exists for), alternating-sign, single-last-coefficient and sparse long-run blocks"""
    rng = np.random.default_rng(77)
    cases = []
    for k, ((w, h), ss) in enumerate(itertools.product(((16, 16), (64, 48), (32, 112)), (None, 0, 1, 2))):
        samp = (1, 1) if ss is None else E.SAMPLINGS[ss]
        img = _content('he' if k % 2 else 'noise', h, w, 200 + k, 1 if ss is None else 3)
        coefs = E.coefficients(img, E.quality_tables((30, 75, 100)[k % 3]), samp)
        for restart in (0, 1, 3):
            cases.append((w, h, len(coefs), samp[0], samp[1], restart, E.mcu_order(coefs, samp)))
    for ncomp, (hs, vs) in ((1, (1, 1)), (3, (1, 1)), (3, (2, 1)), (3, (2, 2))):
        w, h = 32, 16
        mcus, bpm = (w // (8 * hs)) * (h // (8 * vs)), (hs * vs + 2 if ncomp == 3 else 1)
        shape = (mcus, bpm, 64)
        sign = np.where(np.arange(mcus * bpm * 64).reshape(shape) & 1, -1, 1)
        last = np.zeros(shape, np.int64)
        last[..., 63] = -1
        sparse = np.where(rng.random(shape) < 0.03, rng.integers(-1023, 1024, shape), 0)
        blocksign = np.where(np.arange(mcus * bpm).reshape(mcus, bpm, 1) & 1, -1, 1)
        for restart in (0, 2):
            for m in (np.zeros(shape, np.int64), np.full(shape, 1023), np.full(shape, -1023), 1023 * sign, 1023 * blocksign * np.ones(shape, np.int64),
                      last, sparse, rng.integers(-1023, 1024, shape)):
                cases.append((w, h, ncomp, hs, vs, restart, m.astype(np.int16)))
    return cases


@pytest.fixture(scope='module')
def sanitizer_run(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('jenc_san')
    exe = str(d / 'jenc_san')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer',
           os.path.join(ROOT, 'tests', 'jenc_san_main.cpp'), '-o', exe]
    if os.path.basename(cxx) == 'g++':
        cmd += ['-static-libasan', '-static-libubsan']          # the runtimes inside the program: nothing has to be preloaded or come first
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode:
        if re.search(r'cannot find .*(asan|ubsan)|libasan|libubsan', res.stdout):
            pytest.skip('the sanitizer runtime is not installed')
        raise AssertionError(res.stdout)
    cases = sanitizer_corpus()
    with open(d / 'corpus.bin', 'wb') as f:
        f.write(struct.pack('<I', len(cases) + 1))
        for w, h, nc, hs, vs, restart, m in cases:
            f.write(struct.pack('<6iI', w, h, nc, hs, vs, restart, m.size) + np.ascontiguousarray(m, '<i2').tobytes())
        f.write(struct.pack('<6iI', 24, 16, 1, 1, 1, 0, 0))     # a geometry the loop must refuse: status 1, nothing else
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    res = subprocess.run([exe, str(d / 'corpus.bin'), str(d / 'results.bin')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0, res.stdout[-4000:]
    raw = open(d / 'results.bin', 'rb').read()
    results, at = [], 0
    for _ in range(len(cases) + 1):
        st, n = struct.unpack('<iI', raw[at:at + 8])
        results.append((st, raw[at + 8:at + 8 + n]))
        at += 8 + n
    assert at == len(raw)
    return cases, results


def test_sanitized_encode_loop_equals_the_spec(sanitizer_run):
    """the size pass and the write pass of the shared loop (the entropy kernels' source, run on the host into buffers of exactly the
    size the size pass reported) give the spec's bytes, case by case"""
    cases, results = sanitizer_run
    assert len(cases) >= 90 and results[-1] == (1, b'')
    for (w, h, nc, hs, vs, restart, m), (st, scan) in zip(cases, results):
        assert st == 0
        assert scan == E.scan_bytes(m, nc, (hs, vs), restart), (w, h, nc, hs, vs, restart)
