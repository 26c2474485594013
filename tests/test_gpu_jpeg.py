"""GPU tests of the JPEG path (csrc/jpeg.hip, ingest.level_from_tiff, TiffSlide.device_level): tile batches against Pillow with 0
differing bytes, level assembly (clipped tiles, misaligned rows, guard bytes), batching, host fallback, bad data, and the drivers.

Frame sizes (width x height): 8 x 8 and 16 x 16 (a single MCU), 40 x 56 and 56 x 40 (no multiple of the 4:2:0 MCU: the upsampling edge
is at chroma column 20 / 28 and row 28 / 20, inside planes padded to 24 / 32), 48 x 64, 240 x 240 (Aperio's tile, 4:2:2).  A batch holds one geometry; every reference is decoded once by
Pillow.  The bad streams are the ones tests/test_jpeg_cpu.py has run through the same decode loop under the host sanitizers."""
import io
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_oracle as O
import tiff_fixture as TF
from wsi_segmentation_pipeline_amd import ingest, native
from wsi_segmentation_pipeline_amd.tiffslide import TiffSlide

pytestmark = pytest.mark.gpu
GUARD = 4096


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


def _pillow(stream):
    return np.asarray(Image.open(io.BytesIO(stream)).convert('RGB'))


def _decode_strip(dev, streams, tables=None, transform=None, **kw):
    """n streams of one frame size -> ((n, h, w, 3) u8, status): the tiles stacked in a one-column grid"""
    buf = np.frombuffer(b''.join(streams), np.uint8)
    lens = np.array([len(s) for s in streams], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    base = ingest.jpeg_parse_tables(tables)[1] if tables else None
    rec, sets, n_sets = ingest.jpeg_walk(buf, offs, lens, base)
    assert (rec['status'] == 0).all()
    w, h = int(rec['width'][0]), int(rec['height'][0])
    n = len(streams)
    if transform is None:
        transform = O.libjpeg_transform(O.parse(streams[0], O.parse_tables(tables) if tables else None))
    level = torch.full((n * h, w, 3), 7, dtype=torch.uint8, device=dev)
    status = ingest.jpeg_decode_tiles(buf, rec, sets, n_sets, np.arange(n, dtype=np.int32), (1, n), level, int(transform), **kw)
    return level.cpu().numpy().reshape(n, h, w, 3), status


SIZES = [(8, 8), (16, 16), (40, 56), (56, 40), (48, 64), (240, 240)]       # (width, height)
CASES = [(w, h, ss) for (w, h) in SIZES for ss in ((1,) if (w, h) == (240, 240) else (0, 1, 2))]


@pytest.mark.parametrize('w,h,ss', CASES, ids=lambda v: str(v))
def test_tile_batches_equal_pillow(dev, w, h, ss):
    """quality 30 / 75 / 95 x noise / H&E-like x (no restart, restart interval 3) in one batch; RGB and grey of the size in batches of
    their own"""
    streams = []
    for k, (q, kind, restart) in enumerate(itertools.product((30, 75, 95), ('noise', 'he'), (0, 3))):
        img = (TF.noise if kind == 'noise' else TF.he_like)(h, w, 100 + k)
        streams.append(TF.encode(img, q, ss, restart=restart))
    batches = [streams]
    if ss == 0 or (w, h) == (240, 240):
        batches.append([TF.encode(TF.he_like(h, w, 7), 75, 0, rgb=True), TF.encode(TF.noise(h, w, 8), 90, 0, rgb=True, restart=3)])
        batches.append([TF.encode(TF.he_like(h, w, 9, 1), 75), TF.encode(TF.noise(h, w, 10, 1), 30, restart=3)])
    for batch in batches:
        got, status = _decode_strip(dev, batch)
        assert (status == 0).all()
        for i, s in enumerate(batch):
            assert int((got[i] != _pillow(s)).sum()) == 0, i


@pytest.fixture(scope='module')
def tiles65():
    streams = [TF.encode(TF.he_like(64, 48, 200 + k) if k % 3 else TF.noise(64, 48, 200 + k), (30, 75, 95)[k % 3], 2, restart=(0, 3)[k % 2])
               for k in range(65)]
    return streams, np.stack([_pillow(s) for s in streams])


@pytest.mark.parametrize('lanes', (0, 7, 64))
@pytest.mark.parametrize('n', (1, 63, 64, 65))
def test_batch_sizes_around_a_wave(dev, tiles65, n, lanes):
    """lanes = tiles per wave of the entropy kernel (a workgroup is one wave).  64: the four sizes leave a wave partly filled, fill it
    and spill one tile into a second workgroup; 7: ragged last workgroups (63 = 9 x 7, 64 = 9 x 7 + 1, 65 = 9 x 7 + 2); 0: the library's
    choice, one tile per wave at these sizes."""
    streams, ref = tiles65
    got, status = _decode_strip(dev, streams[:n], lanes=lanes)
    assert (status == 0).all() and int((got != ref[:n]).sum()) == 0


def test_large_batch_fills_the_chip_with_several_lanes_per_wave(dev):
    """the library's own lane count: ceil(n / (4 x CUs)) tiles per wave.  n = 2 x 4 x CUs + 1 tiles of 16 x 16 gives three lanes per wave
    and a last workgroup that is not full; 24 different streams (sub-sampling 4:2:0, quality, content, restart) repeat through the batch,
    so neighbouring lanes of a wave run different streams."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    n = 2 * 4 * cus + 1
    kinds = [TF.encode((TF.noise if k % 2 else TF.he_like)(16, 16, 500 + k), (30, 75, 95)[k % 3], 2, restart=(0, 1, 3)[(k // 2) % 3]) for k in range(24)]
    ref = np.stack([_pillow(s) for s in kinds])
    order = (np.arange(n) * 7) % 24
    got, status = _decode_strip(dev, [kinds[i] for i in order])
    assert (status == 0).all() and int((got != ref[order]).sum()) == 0


def test_abbreviated_streams_with_tables_and_forced_transform(dev):
    """JPEGTables + abbreviated streams with their APP markers stripped: the transform is the caller's (the photometric tag), 1 and 0"""
    imgs = [TF.he_like(48, 64, 300 + k) for k in range(5)]
    for rgb in (False, True):
        tables = TF.encode(imgs[0], 75, 0 if rgb else 1, rgb=rgb, streamtype=1)
        streams = [TF.encode(im, 75, 0 if rgb else 1, rgb=rgb, streamtype=2, strip=True) for im in imgs]
        got, status = _decode_strip(dev, streams, tables, transform=0 if rgb else 1)
        ref = np.stack([O.decode(s, O.parse_tables(tables), transform=not rgb) for s in streams])
        assert (status == 0).all() and int((got != ref).sum()) == 0
        full = np.stack([_pillow(TF.encode(im, 75, 0 if rgb else 1, rgb=rgb)) for im in imgs])      # the complete streams hold the same scan
        assert int((got != full).sum()) == 0


def _offsets(streams):
    lens = np.array([len(s) for s in streams], np.uint64)
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64), lens


def longest_code(stream):
    """the longest Huffman code the stream's DHT segments define, in bits"""
    return max(l + 1 for counts, _ in O.parse(stream)['huff'].values() for l in range(16) if counts[l])


def test_optimised_huffman_tables_one_set_per_tile(dev):
    """48 complete 48 x 64 streams with Huffman tables made for each image (Pillow's optimize=True): the three sub-samplings x quality
    30 / 75 / 95 x noise / H&E-like x (no restart, restart interval 3), and quality 50 / 90 without restart.  The walk finds a table set
    per stream, so all but the common one are read from memory instead of LDS, and codes longer than the 9 look-up bits (up to 13 bits;
    33 of the 48 streams define one) take huff_decode's slow path."""
    combos = list(itertools.product((0, 1, 2), (30, 75, 95), ('noise', 'he'), (0, 3))) + list(itertools.product((0, 1, 2), (50, 90), ('noise', 'he'), (0,)))
    streams = [TF.encode((TF.noise if kind == 'noise' else TF.he_like)(64, 48, 700 + k), q, ss, restart=r, optimize=True)
               for k, (ss, q, kind, r) in enumerate(combos)]
    assert len(streams) == 48
    offs, lens = _offsets(streams)
    rec, sets, n_sets = ingest.jpeg_walk(np.frombuffer(b''.join(streams), np.uint8), offs, lens)
    longest = [longest_code(s) for s in streams]
    print('%d table sets for %d streams, longest code %d bits, %d streams with a code past %d bits' % (
        n_sets, len(streams), max(longest), sum(l > 9 for l in longest), 9))
    assert (rec['status'] == 0).all() and n_sets > 1 and len(set(rec['table_set'])) == n_sets and max(longest) > 9
    got, status = _decode_strip(dev, streams)
    assert (status == 0).all()
    for i, s in enumerate(streams):
        assert int((got[i] != _pillow(s)).sum()) == 0, (i, combos[i])


@pytest.mark.parametrize('w,h,ss', [(4096, 16, 0), (4096, 16, 1), (4096, 16, 2), (16, 4096, 0), (16, 4096, 1), (16, 4096, 2), (1032, 520, 2)],
                         ids=lambda v: str(v))
def test_frames_at_the_largest_dimension(dev, w, h, ss):
    """MAX_DIM = 4096 in either direction (769 pieces per row and a plane pitch of 4096 bytes; 512 block rows), and 1032 x 520, 4:2:0:
    no multiple of 16 in height, 66 x 130 + 2 x 33 x 65 = 12 870 blocks in one tile.  Two streams (H&E-like; noise with restart interval 3)
    stacked in a level that starts 0, 7 and 16 bytes past a 16-byte boundary inside guard bytes."""
    streams = [TF.encode(TF.he_like(h, w, 900 + ss), 75, ss), TF.encode(TF.noise(h, w, 910 + ss), 90, ss, restart=3)]
    ref = np.stack([_pillow(s) for s in streams]).reshape(2 * h, w, 3)
    buf = np.frombuffer(b''.join(streams), np.uint8)
    rec, sets, n_sets = ingest.jpeg_walk(buf, *_offsets(streams))
    assert (rec['status'] == 0).all() and (int(rec['width'][0]), int(rec['height'][0])) == (w, h)
    nbytes = 2 * h * w * 3
    for shift in (0, 7, 16):
        whole = torch.full((2 * GUARD + nbytes + 32,), 0x5A, dtype=torch.uint8, device=dev)
        view = whole[GUARD + shift:GUARD + shift + nbytes].view(2 * h, w, 3)
        status = ingest.jpeg_decode_tiles(buf, rec, sets, n_sets, np.arange(2, dtype=np.int32), (1, 2), view, 1)
        host = whole.cpu().numpy()
        assert (status == 0).all()
        assert int((host[GUARD + shift:GUARD + shift + nbytes].reshape(2 * h, w, 3) != ref).sum()) == 0, shift
        assert (host[:GUARD + shift] == 0x5A).all() and (host[GUARD + shift + nbytes:] == 0x5A).all(), shift


def test_second_store_launch_past_65535_tiles(dev):
    """65 537 tiles of 16 x 16, 4:2:0, in one jpeg_decode_batch: wsi_jpeg_reconstruct launches store_kernel once per 65 535 tiles, so
    tiles 65 535 and 65 536 run with tile0 = 65 535.  The 24 streams of the large-batch test repeat in the order (i * 7) % 24; tile i goes
    to cell perm[i] of a 256 x 257 grid (a seeded permutation of its first 65 537 cells), so a tile that takes another's status, planes or
    cell lands in the wrong place.  Tiles 0 and 65 536 are streams that fail in the decode loop: their status is reported and their
    cells keep the fill byte, as do the 255 cells no tile is sent to.  (Were the second launch to read the status of tiles 0 and 1, tile
    65 535 would be left out and the failed tile 65 536 stored.)"""
    lib = native.load()
    n, cols, rows, fill = 65537, 256, 257, 0x5A
    kinds = [TF.encode((TF.noise if k % 2 else TF.he_like)(16, 16, 500 + k), (30, 75, 95)[k % 3], 2, restart=(0, 1, 3)[(k // 2) % 3]) for k in range(24)]
    bad = TF.bad_scan_streams(2)
    kinds += [bad['exhausted'][0], bad['bad_code'][0]]
    ref = np.stack([_pillow(s) for s in kinds[:24]])
    order = (np.arange(n) * 7) % 24
    order[0], order[65536] = 24, 25
    want_status = np.zeros(n, np.int32)
    want_status[0], want_status[65536] = bad['exhausted'][1], bad['bad_code'][1]
    assert bad['exhausted'][1] == O.EXHAUSTED and bad['bad_code'][1] == O.BAD_CODE
    offs, lens = _offsets(kinds)                                # the 26 streams once; the records name them over and over
    buf = np.frombuffer(b''.join(kinds), np.uint8)
    rec, sets, n_sets = ingest.jpeg_walk(buf, offs[order], lens[order])
    assert (rec['status'] == 0).all() and len(rec) == n
    geom = (16, 16, 3, 2, 2)
    assert all(ingest._geometry(rec[i]) == geom for i in (0, 1, 65535, 65536))
    cells = np.random.default_rng(65537).permutation(n).astype(np.int32)
    data_at, tot, stage = ingest.jpeg_stage(buf, rec, np.arange(n), cells)
    tile_ws = lib.wsi_jpeg_workspace_bytes(*geom)
    assert tile_ws == 1280
    ws = torch.empty(n * tile_ws, dtype=torch.uint8, device=dev)
    H, W = rows * 16, cols * 16
    lvl_whole = torch.full((2 * GUARD + H * W * 3,), fill, dtype=torch.uint8, device=dev)
    level = lvl_whole[GUARD:GUARD + H * W * 3].view(H, W, 3)
    status = torch.full((n + 2,), -1, dtype=torch.int32, device=dev)
    sets_dev = torch.from_numpy(sets[:n_sets].view(np.uint8).reshape(-1).copy()).to(dev)
    common = int(np.bincount(rec['table_set']).argmax())
    ingest.jpeg_decode_batch(torch.from_numpy(stage).to(dev), tot, n, sets_dev, n_sets, common, geom, ws, status[1:n + 1], 1, (cols, rows), level)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert st[0] == -1 and st[-1] == -1 and np.array_equal(st[1:-1], want_status)
    host = lvl_whole.cpu().numpy()
    assert (host[:GUARD] == fill).all() and (host[-GUARD:] == fill).all()
    got = host[GUARD:-GUARD].reshape(rows, 16, cols, 16, 3).transpose(0, 2, 1, 3, 4).reshape(rows * cols, 16, 16, 3)     # by cell
    want = np.full_like(got, fill)
    good = want_status == 0
    want[cells[good]] = ref[order[good]]
    wrong = np.nonzero((got != want).reshape(rows * cols, -1).any(1))[0]
    assert wrong.size == 0, 'cells %s differ (tiles %s)' % (wrong[:8], [int(np.nonzero(cells == c)[0][0]) if c in cells else None for c in wrong[:8]])
    assert int((got != want).sum()) == 0


# ------------------------------------------------------------------------------------------------------------------ level assembly
@pytest.fixture(scope='module')
def pyramid_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('jpeg') / 'pyr.tif')
    levels = TF.pyramid(150, 200, 3, seed=11)
    info = TF.write_tiff(path, levels, tile=(64, 48), subsampling=2)
    return path, info, TF.pillow_levels(path, info['frames'])


def test_level_clipped_misaligned_inside_guards(dev, pyramid_file):
    """150 x 200 of 64 x 48 tiles: clipped on both axes, rows of 600 bytes, the level at an odd address inside a larger buffer"""
    path, info, ref = pyramid_file
    s = TiffSlide(path)
    lv = s.levels[0]
    buf = np.frombuffer(s._map, np.uint8)
    rec, sets, n_sets = ingest.jpeg_walk(buf, lv.offsets, lv.counts, ingest.jpeg_parse_tables(lv.tables)[1])
    for shift in (0, 7, 16):
        whole = torch.full((2 * GUARD + 150 * 600 + 32,), 0x5A, dtype=torch.uint8, device=dev)
        view = whole[GUARD + shift:GUARD + shift + 150 * 600].view(150, 200, 3)
        status = ingest.jpeg_decode_tiles(buf, rec, sets, n_sets, np.arange(16, dtype=np.int32), (4, 4), view, 1)
        host = whole.cpu().numpy()
        assert (status == 0).all()
        assert int((host[GUARD + shift:GUARD + shift + 150 * 600].reshape(150, 200, 3) != ref[0]).sum()) == 0, shift
        assert (host[:GUARD + shift] == 0x5A).all() and (host[GUARD + shift + 150 * 600:] == 0x5A).all(), shift
    del buf
    s.close()


def test_pyramid_levels_equal_libtiff_any_batching(dev, pyramid_file):
    path, info, ref = pyramid_file
    s = TiffSlide(path)
    for k in range(3):
        got = s.device_level(k, dev)
        assert got.shape == ref[k].shape and got.dtype == torch.uint8 and s.device_level(k, dev) is got
        assert int((got.cpu().numpy() != ref[k]).sum()) == 0, k
        assert s.decode_report[k] == {'ok': len(info['streams'][k])}
    tile_ws = native.load().wsi_jpeg_workspace_bytes(64, 48, 3, 2, 2)
    small = ingest.level_from_tiff(s, 0, dev, workspace_bytes=5 * tile_ws)                  # 16 tiles: batches of 5, 5, 5, 1
    assert torch.equal(small, s.device_level(0, dev))
    one = ingest.level_from_tiff(s, 0, dev, workspace_bytes=1)                              # a tile per batch
    assert torch.equal(one, small)
    ring = ingest.level_from_slide(s, 0, dev)                                               # the host path through the ring, unchanged
    assert torch.equal(ring, small)
    s.close()


def test_fallback_progressive_and_empty_tiles(dev, tmp_path):
    levels = TF.pyramid(150, 200, 2, seed=12)
    path = str(tmp_path / 'fb.tif')
    TF.write_tiff(path, levels, tile=(64, 48), subsampling=1, progressive={(0, 6)}, empty={(0, 9), (1, 0)})
    s = TiffSlide(path)
    want = np.asarray(s.read_region((0, 0), 0, (200, 150)))[..., :3]                        # the host path, held against libtiff on the CPU
    assert (want[96:144, 64:128] == 255).all()                                              # tile 9: row 2, column 1
    got = s.device_level(0, dev).cpu().numpy()
    assert int((got != want).sum()) == 0
    assert s.decode_report[0] == {'ok': 14, 'progressive': 1, 'empty': 1}
    prog = _pillow(bytes(s.tile_bytes(0, 6)))
    assert int((got[48:96, 128:192] != prog).sum()) == 0
    assert int((s.device_level(1, dev).cpu().numpy() != np.asarray(s.read_region((0, 0), 1, (100, 75)))[..., :3]).sum()) == 0
    assert s.decode_report[1] == {'ok': 3, 'empty': 1}
    s.close()
    # a tile neither path decodes: the error names level and tile
    raw = bytearray(open(path, 'rb').read())
    s = TiffSlide(path)
    off, cnt = int(s.levels[0].offsets[3]), int(s.levels[0].counts[3])
    s.close()
    raw[off + cnt // 2:off + cnt] = b'\x00' * (cnt - cnt // 2)
    bad = str(tmp_path / 'bad.tif')
    open(bad, 'wb').write(raw)
    s = TiffSlide(bad)
    with pytest.raises(ValueError, match='level 0 tile 3'):
        s.device_level(0, dev)
    s.close()


def test_level_with_more_table_sets_than_the_walk_keeps(dev, tmp_path):
    """a level of 70 tiles without JPEGTables, every tile with optimised tables of its own: the walk keeps JPEG_TABLE_SETS = 64 sets and
    turns the tiles that would need more away with TABLE_CAPACITY; level_from_tiff decodes those on the host.  The split is the walk's
    (two tiles may share a set), the level is libtiff's byte for byte."""
    lv = TF.he_like(330, 630, 41)
    lv[:, 540:] = TF.noise(330, 90, 42)                         # he_like's white right edge would give the last column one set
    path = str(tmp_path / 'own_tables.tif')
    info = TF.write_tiff(path, [lv], tile=(64, 48), jpegtables=False, optimize=True, subsampling=2)
    assert len(info['streams'][0]) == 70 and b'\xff\xc4' in info['streams'][0][0]
    ref = TF.pillow_levels(path, info['frames'])[0]
    s = TiffSlide(path)
    l0 = s.levels[0]
    assert not l0.tables
    rec, sets, n_sets = ingest.jpeg_walk(np.frombuffer(s._map, np.uint8), l0.offsets, l0.counts, None)
    n_ok, n_cap = int((rec['status'] == 0).sum()), int((rec['status'] == O.TABLE_CAPACITY).sum())
    print('%d tiles: %d table sets, %d tiles accepted, %d refused for capacity, longest code %d bits' % (
        len(rec), n_sets, n_ok, n_cap, max(longest_code(t) for t in info['streams'][0])))
    assert n_sets == ingest.JPEG_TABLE_SETS == 64 and n_cap > 0 and n_ok + n_cap == 70 and n_ok >= 64
    got = s.device_level(0, dev)
    assert got.shape == ref.shape and int((got.cpu().numpy() != ref).sum()) == 0
    assert s.decode_report[0] == {'ok': n_ok, 'table_capacity': n_cap}
    s.close()


def test_bad_tiles_report_status_and_touch_nothing_else(dev):
    """four valid 16 x 16 grey tiles (the last one ends its blocks with a ZRL past coefficient 63, as libjpeg allows) and the four streams
    made to fail in the decode loop, in one batch, four lanes to a wave: the bad tiles report their
    status, the valid ones are exact, the guards around the workspace and the level stay as they were, and so do the bad tiles' cells"""
    lib = native.load()
    bad = TF.bad_scan_streams()
    names = ['exhausted', 'bad_code', 'coef_overrun', 'short']
    good = [TF.encode(TF.noise(16, 16, 400 + k, 1), (30, 75, 95)[k], restart=(0, 2)[k % 2]) for k in range(3)]
    streams = [good[0], bad[names[0]][0], good[1], bad[names[1]][0], bad[names[2]][0], good[2], bad[names[3]][0], bad['zrl_end'][0]]
    want_status = [0, bad[names[0]][1], 0, bad[names[1]][1], bad[names[2]][1], 0, bad[names[3]][1], 0]
    assert [bad[k][1] for k in names] == [O.EXHAUSTED, O.BAD_CODE, O.COEF_OVERRUN, O.SHORT] and bad['zrl_end'][1] == 0
    buf = np.frombuffer(b''.join(streams), np.uint8)
    lens = np.array([len(s) for s in streams], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    rec, sets, n_sets = ingest.jpeg_walk(buf, offs, lens)
    assert (rec['status'] == 0).all()                           # the walk passes all eight: the damage is in the scan
    n = 8
    data_at, tot, stage = ingest.jpeg_stage(buf, rec, list(range(n)), np.arange(n, dtype=np.int32))
    tile_ws = lib.wsi_jpeg_workspace_bytes(16, 16, 1, 1, 1)
    ws_whole = torch.full((2 * GUARD + n * tile_ws,), 0xC3, dtype=torch.uint8, device=dev)
    lvl_whole = torch.full((2 * GUARD + n * 16 * 16 * 3,), 0x5A, dtype=torch.uint8, device=dev)
    ws = ws_whole[GUARD:GUARD + n * tile_ws]
    level = lvl_whole[GUARD:GUARD + n * 768].view(n * 16, 16, 3)
    status = torch.full((n + 2,), -1, dtype=torch.int32, device=dev)
    sets_dev = torch.from_numpy(sets[:n_sets].view(np.uint8).reshape(-1).copy()).to(dev)
    ingest.jpeg_decode_batch(torch.from_numpy(stage).to(dev), tot, n, sets_dev, n_sets, 0, (16, 16, 1, 1, 1), ws, status[1:n + 1], 1, (1, n), level, lanes=4)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert st[0] == -1 and st[-1] == -1 and list(st[1:-1]) == want_status
    host = lvl_whole.cpu().numpy()
    tiles = host[GUARD:GUARD + n * 768].reshape(n, 16, 16, 3)
    for i, s in enumerate(streams):
        if want_status[i] == 0:
            assert int((tiles[i] != _pillow(s)).sum()) == 0, i
        else:
            assert (tiles[i] == 0x5A).all(), i
    assert (host[:GUARD] == 0x5A).all() and (host[-GUARD:] == 0x5A).all()
    wsh = ws_whole.cpu().numpy()
    assert (wsh[:GUARD] == 0xC3).all() and (wsh[-GUARD:] == 0xC3).all()


# --------------------------------------------------------------------------------------------------------------------- the drivers
def _args(monkeypatch, tmp_path):
    import myargs
    for k, v in (('scan_level', 0), ('scan_resize', 1), ('num_classes', 4), ('class_probs', [0., 0., 0., 0.]), ('tile_w', 64), ('tile_h', 64),
                 ('tile_stride_w', 64), ('tile_stride_h', 64), ('val_save_pth', str(tmp_path / 'out')), ('wsi_mask_pth', str(tmp_path / 'nomask'))):
        monkeypatch.setattr(myargs.args, k, v)


@pytest.fixture(scope='module')
def he_slide(tmp_path_factory):
    """a 512 x 512 H&E-like slide with levels at 1, 4 and 16 as a tiled JPEG TIFF, and the same pyramid as Pillow's libtiff decodes it"""
    import stain_oracle as SO
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    l0 = SO.shifted_he(31, 1, 512)[0]
    path = str(tmp_path_factory.mktemp('slide') / 'case.svs')
    info = TF.write_tiff(path, [l0, l0[::4, ::4], l0[::16, ::16]], tile=(128, 128), subsampling=1, quality=85, thumbnail=True)
    decoded = TF.pillow_levels(path, info['frames'])
    arr = ArraySlide(decoded, [1.0, 4.0, 16.0])
    arr.name = 'case.svs'
    return path, arr


def test_dataset_and_iterator_equal_array_slide(dev, he_slide, tmp_path, monkeypatch):
    import utils.dataset as ds
    _args(monkeypatch, tmp_path)
    path, arr = he_slide
    tiff = TiffSlide(path)
    assert tiff.level_downsamples == (1.0, 4.0, 16.0)
    params = {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}
    a = ds.Dataset_wsis({'case.svs': tiff}, params, bs=8)
    b = ds.Dataset_wsis({'case.svs': arr}, params, bs=8)
    ia, ib = a.wsis['case.svs']['iterator'], b.wsis['case.svs']['iterator']
    assert a.wsis['case.svs']['scan'] is tiff and np.array_equal(a.wsis['case.svs']['mask'], b.wsis['case.svs']['mask'])
    assert len(ia.dataset) == len(ib.dataset) > 8 and np.array_equal(ia.dataset.tile_xy, ib.dataset.tile_xy)
    batches = 0
    for (xa, ya, ima), (xb, yb, imb) in zip(ia, ib):
        assert torch.equal(xa, xb) and torch.equal(ya, yb) and torch.equal(ima, imb)
        batches += 1
    assert batches == len(ia) == len(ib)
    item_a, item_b = ia.dataset[3], ib.dataset[3]                                           # single-item access: the host path
    assert item_a[:2] == item_b[:2] and torch.equal(item_a[2], item_b[2])
    tiff.close()


def test_predict_tumorbed_and_stain_equal_array_slide(dev, he_slide, tmp_path, monkeypatch):
    import resnets_shift
    import utils.dataset as ds
    import utils.eval as val
    from models.models import Classifier
    from wsi_segmentation_pipeline_amd import stain
    from wsi_segmentation_pipeline_amd import synthetic as W
    _args(monkeypatch, tmp_path)
    path, arr = he_slide
    net = resnets_shift.resnet18(False)
    net.load_state_dict(W.make_resnet18_state_dict(11, with_fc=False), strict=False)
    head = Classifier(512, 4)
    head.load_state_dict(W.make_head_state_dict(22, 'classifier'))
    model = val.SlideClassifierModel(net, head).to(dev)
    params = {'ph': 64, 'pw': 64, 'sh': 64, 'sw': 64}

    def run(scan, **kw):
        dataset = ds.Dataset_wsis({'case.svs': scan}, params, bs=16, **kw)
        res = val.predict_tumorbed(model, dataset, 1, mode='cls', save=False)['case.svs']
        return res['logits'].cpu().numpy(), np.asarray(res['heatmap']), np.asarray(res['classes'])
    tiff = TiffSlide(path)
    for kw in ({}, {'stain': stain.Normalizer('macenko')}):
        got, want = run(tiff, **kw), run(arr, **kw)
        for x, y in zip(got, want):
            assert x.shape == y.shape and np.array_equal(x, y)
    norm = stain.Normalizer('macenko')
    sa, sb = stain.StainedSlide(tiff, norm), stain.StainedSlide(arr, norm)
    assert torch.equal(sa.device_level(0, dev), sb.device_level(0, dev)) and sa.stain_error is None
    tiff.close()
