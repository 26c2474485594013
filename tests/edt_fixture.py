"""Maps for the distance transform's tests (tests/test_edt_cpu.py, tests/test_gpu_edt.py): seeded random maps over the densities at
which the nearest feature is next door or far away, and the shapes at which the kernels of csrc/edt.hip take another path.  NumPy only."""
import numpy as np

BAND = 64                                # csrc/edt_dev.h wsi_edt::BAND: rows of one band of the column pass
TILE_W = 256                             # csrc/edt.hip TILE_W: columns of one workgroup of the column pass, and of one lane round of the row pass
ROW_ROUND = 256 * 8                      # csrc/edt.hip THREADS * ROW_VEC: g values the row pass fetches per round of its lanes
DENSITIES = (0.001, 0.01, 0.05, 0.2, 0.5, 0.9)


def random_map(h, w, density, seed):
    """bytes 1 .. 255 at `density` of the pixels, 0 elsewhere"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((h, w)) < density, rng.integers(1, 256, (h, w)), 0).astype(np.uint8)


def random_cases(n, seed=5, max_h=40, max_w=40):
    """n seeded cases {name, m, invert}: every density in turn, both invert settings, sizes 1 .. max each way; case 0 is the empty
    map, case 1 the all-feature map"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        h, w = int(rng.integers(1, max_h + 1)), int(rng.integers(1, max_w + 1))
        density = DENSITIES[k % len(DENSITIES)]
        m = random_map(h, w, density, seed * 1000 + k)
        if k == 0:
            m[:] = 0
        elif k == 1:
            m[:] = 255
        out.append(dict(name='random%d' % k, m=m, invert=bool((k // len(DENSITIES)) % 2), density=density))
    return out


def far_end_row(w=32768):
    m = np.zeros((1, w), np.uint8)
    m[0, -1] = 1
    return m


def far_end_column(h=32768):
    m = np.zeros((h, 1), np.uint8)
    m[-1, 0] = 1
    return m


def largest_sum_row(w=32768):
    """a hand-made row of the g plane: g[0] = 32767, every other column without a feature, so out[w - 1] = 2 * 32767^2 at w = 32768"""
    g = np.full(w, 0xFFFF, np.uint16)
    g[0] = 32767
    return g


def corners(h, w):
    m = np.zeros((h, w), np.uint8)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 7
    return m


def disc(h, w, cy, cx, r):
    y, x = np.mgrid[0:h, 0:w]
    return ((y - cy) ** 2 + (x - cx) ** 2 <= r * r).astype(np.uint8)
