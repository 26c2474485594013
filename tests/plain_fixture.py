"""Inputs and expected values for the tests that send the plain grid-stride kernels (csrc/proposals.hip, postproc.hip,
slide_ops.hip, ingest.hip) past one launch, one LDS round of SLIC centres and one round of scan block sums.

The constants restate launch caps of the HIP sources; tests/test_plain_strides_cpu.py reads the sources and fails when one of
them moves, so that a later change of a cap cannot put these tests back inside a single launch.  Every size below is an
expression of these constants or is asserted against them there.  Expected values come from the oracles (oracle/*, NumPy)
only; each is computed once per process, shared, and handed out read-only."""
import functools

import numpy as np

from oracle import postprocess_oracle as PPO
from oracle import proposals_oracle as PO
from oracle import resize_oracle as RO
from oracle import wsi_oracle as WO

# ------------------------------------------------------------------------------------------ caps (elements of one launch)
BLOCK = 256                      # threads per workgroup of every kernel here: dim3(256), stride gridDim.x * 256
CAP_16384 = 16384 * 256          # grid_for of postproc.hip, slide_ops.hip and ingest.hip: `g > 16384 ? 16384`
CAP_PROPOSALS = 8192 * 256       # grid_for of proposals.hip: `g > 8192 ? 8192`
CAP_LAB = 2048 * 256             # wsi_lab_mask_dispatch: `grid_for(npix) > 2048 ? 2048` (lab_a_kernel, lab_thresh_kernel)
CAP_SLIC_SUM = 4096 * 256        # wsi_slic_dispatch: slic_sum_kernel at `g1 > 4096 ? 4096`
CAP_COUNTS = 1024 * 256          # iou / score counts and exponent span: `grid_for(n) > 1024 ? 1024` (not exercised here)
SLIC_LDS_ROUND = 1024            # slic_assign_kernel: `for (int k0 = 0; k0 < K; k0 += 1024)`, `__shared__ double sg[1024 * 6]`
SLIC_MAXK = 2048                 # `#define SLIC_MAXK 2048`
SCAN_BLOCK = 1024                # scan_block_kernel: `blockIdx.x * 1024`; readers index block_sums[i >> 10]
SCAN_ROUND = 256 * 1024          # scan_sums_kernel: 256 block sums per round (`b0 += 256`), each of SCAN_BLOCK flags


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ------------------------------------------------------------------------------------------ bicubic resample (ingest.hip)
RESAMPLE_IN = (64, 64)
RESAMPLE_LEVEL_HW = (200, 220)
# 16 tile origins (x, y) on the 200 x 220 level; the first six hang over the top-left, right, bottom, bottom-right, left and
# top edges and read black there
RESAMPLE_ORIGINS = np.array([[-20, -30], [180, 50], [40, 170], [190, 180], [-10, 100], [70, -9], [0, 0], [156, 136], [13, 29],
                             [35, 7], [100, 20], [3, 60], [90, 90], [150, 10], [60, 130], [121, 77]], np.int32)
# (tiles, output size): both passes past the cap; width only (no vertical pass: the horizontal kernel writes the output)
RESAMPLE_CASES = {'both_passes': (2200, (48, 40)), 'width_only': (1700, (64, 40))}


def resample_elements(case):
    """(elements of the horizontal pass, elements of the vertical pass or 0 when the plan has none)."""
    n, (th, tw) = RESAMPLE_CASES[case]
    return n * RESAMPLE_IN[0] * tw, (n * th * tw if th != RESAMPLE_IN[0] else 0)


@functools.lru_cache(None)
def resample_level():
    rng = np.random.default_rng(41)
    h, w = RESAMPLE_LEVEL_HW
    level = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    level[: h // 4] = 255
    return _frozen(level)


@functools.lru_cache(None)
def resample_expected(case):
    """The 16 expected tiles (16, th, tw, 3) of the case, one per origin."""
    _, out_hw = RESAMPLE_CASES[case]
    level = resample_level()
    ph, pw = RESAMPLE_IN
    return _frozen(np.stack([RO.resize_bicubic_u8(WO.read_tile(level, int(x), int(y), pw, ph), out_hw) for x, y in RESAMPLE_ORIGINS]))


def resample_origin_of(case):
    """Which of the 16 origins each of the case's tiles uses."""
    return np.arange(RESAMPLE_CASES[case][0]) % len(RESAMPLE_ORIGINS)


# ------------------------------------------------------------------------------------------ tile gather (slide_ops.hip)
GATHER_TILES, GATHER_HW = 70, (256, 256)
GATHER_LEVEL_HW = (300, 400)
GATHER_ORIGINS = np.array([[0, 0], [7, 13], [400 - 256, 300 - 256], [390 - 200, 290 - 200], [-5, -3]], np.int32)   # the last two: partly outside


@functools.lru_cache(None)
def gather_level():
    return _frozen(np.random.default_rng(42).integers(0, 256, GATHER_LEVEL_HW + (3,), dtype=np.uint8))


@functools.lru_cache(None)
def gather_expected():
    """The 5 expected normalised tiles (5, 3, 256, 256) float32, one per origin."""
    from oracle.resnet_oracle import normalize_u8
    level = gather_level()
    ph, pw = GATHER_HW
    return _frozen(np.stack([normalize_u8(WO.read_tile(level, int(x), int(y), pw, ph).transpose(2, 0, 1)[None])[0].numpy()
                             for x, y in GATHER_ORIGINS]))


# ------------------------------------------------------------------------------------------ resize / argmax (postproc.hip)
RESIZE_SRC, RESIZE_DST = (2, 132, 126), (2100, 2000)
ARGMAX_TAIL = 5000                                   # ties and NaNs live in the last ARGMAX_TAIL pixels


@functools.lru_cache(None)
def resize_input():
    return _frozen(np.random.default_rng(43).standard_normal(RESIZE_SRC))


@functools.lru_cache(None)
def resize_expected():
    return _frozen(PPO.resize_bilinear(resize_input(), RESIZE_DST))


@functools.lru_cache(None)
def argmax_input():
    """(2, 2100, 2000) float64: the resized map, with ties, NaNs in either and in both channels and signed zeros in its last
    ARGMAX_TAIL pixels."""
    x = resize_expected().copy().reshape(RESIZE_SRC[0], -1)
    hw = x.shape[1]
    t = hw - ARGMAX_TAIL
    x[1, t:t + 1500] = x[0, t:t + 1500]                                  # ties -> first maximum
    x[0, t + 1500:t + 2200] = np.nan                                     # NaN wins, like np.argmax
    x[1, t + 2200:t + 2900] = np.nan
    x[:, t + 2900:t + 3300] = np.nan
    x[0, t + 3300:t + 3600], x[1, t + 3300:t + 3600] = 0.0, -0.0
    x[0, t + 3600:t + 3900], x[1, t + 3600:t + 3900] = -0.0, 0.0
    return _frozen(x.reshape((RESIZE_SRC[0],) + RESIZE_DST))


@functools.lru_cache(None)
def argmax_expected():
    return _frozen(np.argmax(argmax_input(), 0).astype(np.uint8))


# ------------------------------------------------------------------------------------------ paint (slide_ops.hip)
PAINT_HW = (2100, 2100)
PAINT_RECTS = ((0, 1200, 0, 1500), (600, 1800, 500, 2000), (1500, 2100, 1000, 2100))   # (y0, y1, x0, x1): overlapping pairwise
PAINT_CLASSES = np.array([1, 2, 3, 1], np.uint8)
PAINT_TAIL = 10000                                   # the last region repaints pixels among the map's final PAINT_TAIL


@functools.lru_cache(None)
def paint_case():
    """(index lists, expected int64 label map): three rectangles as tuples of index arrays, then one flat index array."""
    h, w = PAINT_HW
    lists = []
    for y0, y1, x0, x1 in PAINT_RECTS:
        yy, xx = np.mgrid[y0:y1, x0:x1]
        lists.append((yy.ravel(), xx.ravel()))
    rng = np.random.default_rng(44)
    npix = h * w
    lists.append(np.concatenate((rng.integers(0, npix, 50000), np.arange(npix - 7000, npix - 100, 3))).astype(np.int64))
    ref = np.zeros(PAINT_HW, np.int64)
    for idx, c in zip(lists, PAINT_CLASSES):                              # the reference's sequential loop: the last region wins
        if isinstance(idx, tuple):
            ref[idx] = c
        else:
            ref.reshape(-1)[idx] = c
    return lists, _frozen(ref)


def paint_entries():
    return sum(len(i[0]) if isinstance(i, tuple) else len(i) for i in paint_case()[0])


# ------------------------------------------------------------------------------------------ HSV / Lab masks (proposals.hip)
HSV_HW = (1500, 1420)
HSV_MU = (0.1, 0.5)
LAB_HW = (600, 900)
LAB_MU = (0.1, 0.5)
LAB_BLOCK = (545, 598, 200, 700)                      # the purple block (y0, y1, x0, x1): inside the last 60 rows


@functools.lru_cache(None)
def hsv_image():
    """Random image; white, black and grey (delta == 0) rows at the top and again inside the last 22 rows, all of which lie past
    CAP_PROPOSALS pixels."""
    rng = np.random.default_rng(45)
    h, w = HSV_HW
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[:40] = 255
    img[40:60] = 0
    img[60:80] = rng.integers(0, 256, (20, w, 1), dtype=np.uint8)
    img[h - 22:h - 18] = 255
    img[h - 18:h - 12] = 0
    img[h - 12:h - 6] = rng.integers(0, 256, (6, w, 1), dtype=np.uint8)
    return _frozen(img)


def hsv_special_rows():
    h = HSV_HW[0]
    return {'white': (h - 22, h - 18), 'black': (h - 18, h - 12), 'grey': (h - 12, h - 6)}


@functools.lru_cache(None)
def hsv_expected(mu):
    return _frozen(WO.find_nuclei_hsv(hsv_image(), mu))


@functools.lru_cache(None)
def lab_image():
    from tests.test_proposals_oracle import _thumb
    img = _thumb(0, LAB_HW)
    y0, y1, x0, x1 = LAB_BLOCK
    img[y0:y1, x0:x1] = (180, 60, 150)                                    # purple: high a
    return _frozen(img)


@functools.lru_cache(None)
def lab_expected(mu):
    return _frozen(WO.find_nuclei_lab(lab_image(), mu))


# ------------------------------------------------------------------------------------------ SLIC (proposals.hip)
SLIC_ROUND2 = dict(seed=9, hw=(72, 96), n_segments=1300, sigma=1.0, max_iter=3)       # more than SLIC_LDS_ROUND centres
SLIC_SUMS = dict(seed=10, hw=(1030, 1040), n_segments=60, sigma=2.0, max_iter=2)      # more than CAP_SLIC_SUM pixels
SLIC_TOO_MANY = dict(hw=(100, 100), n_segments=2500)                                  # a grid of more than SLIC_MAXK centres
SLIC_COMPACTNESS = 20.0


@functools.lru_cache(None)
def slic_image(name):
    from tests.test_proposals_oracle import _thumb
    case = {'round2': SLIC_ROUND2, 'sums': SLIC_SUMS}[name]
    return _frozen(_thumb(case['seed'], case['hw']))


def slic_centres(case):
    return len(PO.slic_setup(case['hw'][0], case['hw'][1], case['n_segments'])[0])


@functools.lru_cache(None)
def slic_expected(name):
    case = {'round2': SLIC_ROUND2, 'sums': SLIC_SUMS}[name]
    return _frozen(PO.slic_labels(slic_image(name), case['n_segments'], SLIC_COMPACTNESS, case['sigma'], case['max_iter']))


# ------------------------------------------------------------------------------------------ scan under wsi_cc (proposals.hip)
# isolated pixels (every second row and column): each is its own component under 8-connectivity.  (shape, cleared share):
# one-row masks with 1023 / 1024 / 1025 set pixels, whole and thinned; 256 and 257 block sums; three rounds of the sums kernel.
# The 257th block of (512, 513) lies in the last, odd row and is empty (a zero block sum behind a full round); (511, 514) has
# 257 blocks too and set pixels in the last one.
CC_ISOLATED = [((1, 2045), 0.0), ((1, 2047), 0.0), ((1, 2049), 0.0), ((1, 2045), 0.03), ((1, 2047), 0.03), ((1, 2049), 0.03),
               ((512, 512), 0.03), ((513, 512), 0.03), ((512, 513), 0.03), ((700, 800), 0.03), ((511, 514), 0.03)]
CC_GAPPED_ROWS = (SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1)


def isolated_mask(shape, clear, seed=46):
    """m[::2, ::2] = 1, then `clear` of the set pixels removed by a seeded generator, so the per-block counts are irregular."""
    m = np.zeros(shape, np.uint8)
    m[::2, ::2] = 1
    if clear:
        rng = np.random.default_rng(seed + shape[0] * 7919 + shape[1])
        ys, xs = np.nonzero(m)
        drop = rng.random(len(ys)) < clear
        m[ys[drop], xs[drop]] = 0
    return m


def isolated_labels(m):
    """Labels of a mask without two 8-adjacent set pixels: raster rank of each set pixel."""
    return (np.cumsum(m.ravel(), dtype=np.int64).reshape(m.shape) * m).astype(np.int32)


def gapped_row(n):
    """One row of n ones with a gap every third pixel: components are the pairs (3k, 3k + 1), so with n around SCAN_BLOCK the
    pair rooted at 1023 has its other pixel in the next scan block."""
    m = np.ones((1, n), np.uint8)
    m[0, 2::3] = 0
    return m


def row_labels(m):
    """Labels of a one-row mask: number of run starts up to each set pixel."""
    r = m[0] != 0
    starts = r & ~np.concatenate(([False], r[:-1]))
    return (np.cumsum(starts) * r).astype(np.int32)[None]


def scan_blocks(n):
    return (n + SCAN_BLOCK - 1) // SCAN_BLOCK


# ------------------------------------------------------------------------------------------ scan under wsi_tile_grid
TILE_GRID = dict(iw=16700, ih=16700, ph=256, pw=256, sh=32, sw=32, m=0.0625)
TILE_GRID_BLOCK = 48                                  # mask block edge in level-2 pixels (three mask windows of 16)


def tile_grid_candidates():
    g = TILE_GRID
    ny, nx = len(range(1, g['ih'] - 1 - g['ph'], g['sh'])), len(range(1, g['iw'] - 1 - g['pw'], g['sw']))
    return ny * nx + ny + nx


@functools.lru_cache(None)
def tile_grid_mask():
    """Block-structured level-2 mask: blocks of TILE_GRID_BLOCK pixels switched on with probability 0.45, half filled inside."""
    g = TILE_GRID
    rng = np.random.default_rng(47)
    mh, mw = int(g['ih'] * g['m']), int(g['iw'] * g['m'])
    b = TILE_GRID_BLOCK
    coarse = rng.random((mh // b + 1, mw // b + 1)) < 0.45
    return _frozen((np.kron(coarse, np.ones((b, b), bool))[:mh, :mw] & (rng.random((mh, mw)) < 0.5)).astype(np.uint8))


@functools.lru_cache(None)
def tile_grid_expected(masked):
    g = TILE_GRID
    mk = tile_grid_mask() if masked else None
    return _frozen(np.array(WO.tile_grid(g['iw'], g['ih'], g['ph'], g['pw'], g['sh'], g['sw'], mk, g['m']), np.int32).reshape(-1, 2))


# ------------------------------------------------------------------------------------------ degenerate hulls, one-point contour
def _points(shape, pts):
    m = np.zeros(shape, np.uint8)
    for y, x in pts:
        m[y, x] = 1
    return m


# name -> (map, hull pixels of the oracle)
DEGENERATE_HULLS = {
    'row_two_pixels': (_points((1, 300), [(0, 27), (0, 272)]), 246),
    'column_two_pixels': (_points((300, 1), [(8, 0), (291, 0)]), 284),
    'one_by_one': (_points((1, 1), [(0, 0)]), 1),
    'first_corner': (_points((40, 50), [(0, 0)]), 1),
    'last_corner': (_points((40, 50), [(39, 49)]), 1),
    'diagonal_pair': (_points((40, 50), [(2, 3), (30, 44)]), 42),
    'anti_diagonal_corners': (_points((40, 50), [(0, 49), (39, 0)]), 50),
}
ONE_POINT_CONTOUR = np.array([[3.5, -7.25]])
ONE_POINT_NUMS = (1, 3)
