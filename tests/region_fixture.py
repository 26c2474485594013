"""Class maps for the region tables' tests (tests/test_regions_cpu.py, tests/test_gpu_regions.py, tests/regions_san_main.cpp's corpus):
the shapes at which the kernels of csrc/regions.hip take another path or the union-find has the most to do.  NumPy only; blobs, noise,
checkerboard, nested rings and the serpentine come from contour_fixture."""
import numpy as np

import contour_fixture as CF

CHUNK = 1024                             # csrc/regions_dev.h CHUNK: pixels of a row one workgroup walks; items of one scan chunk
SCAN_SPAN = 256 * 4                      # csrc/map_kernels.h SUMS_TILE: chunk sums the one scanning workgroup takes in one step of its loop
SCAN_SECOND = CHUNK * 256                # a run count of 256 scan chunks: the rank stage's scan over more than one chunk of runs


def combs(h, w, label=1):
    """U shapes side by side, ten columns each: four arms on columns 0, 2, 4, 6 that join only in the last row, three empty columns
    between two combs.  Every arm is a region of its own until the very end, so a comb's root changes late."""
    x = np.arange(w)
    m = np.zeros((h, w), np.uint8)
    m[:, (x % 10 < 7) & (x % 2 == 0)] = label
    m[h - 1, x % 10 < 7] = label
    return m


def run_count_map(n_runs, w, label=1):
    """a map with exactly n_runs runs: single pixels on every second column of every second row (no two touch, not even by a corner at
    connectivity 8), so there are as many regions as runs"""
    per_row = (w + 1) // 2
    rows = -(-n_runs // per_row)
    m = np.zeros((2 * rows - 1 if rows else 1, w), np.uint8)
    left = n_runs
    for k in range(rows):
        take = min(left, per_row)
        m[2 * k, 0:2 * take:2] = label
        left -= take
    return m


def spiral(n, label=1):
    """a 1-pixel-wide square spiral in an n x n map, turns 2 pixels apart: one region whose runs are united along a chain as long as
    the map allows"""
    m = np.zeros((n, n), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = label
    while True:
        moved = False
        while True:
            ny, nx = y + dy, x + dx
            ay, ax = ny + dy, nx + dx                            # the pixel after the next: stop before touching an earlier turn
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx] or (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
                break
            y, x = ny, nx
            m[y, x] = label
            moved = True
        if not moved:
            return m
        dy, dx = dx, -dy                                        # turn right


def long_run_map(w, x0, x1, h=3):
    """one run [x0, x1) in the middle row of h rows, a second class to its right"""
    m = np.zeros((h, w), np.uint8)
    m[h // 2, x0:x1] = 1
    m[h // 2, x1:min(w, x1 + 3)] = 2
    return m


def random_cases(n, seed=23):
    """n seeded cases {name, m, classes, connectivity, weight}: blobby and noisy maps of 1 - 4 labels up to 24 x 31, class subsets that
    include 0, both connectivities, a random weight map on every other case"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        h, w = int(rng.integers(1, 25)), int(rng.integers(1, 32))
        labels = int(rng.integers(1, 5))
        m = CF.blob_map(h, w, labels, seed * 1000 + k, radius=1 + k % 3) if k % 2 else CF.noise_map(h, w, labels, seed * 1000 + k)
        classes = None if k % 3 == 0 else sorted({int(c) for c in rng.integers(0, labels + 1, int(rng.integers(1, labels + 2)))})
        weight = rng.integers(0, 256, (h, w)).astype(np.uint8) if k % 2 == 0 else None
        out.append(dict(name='random%d' % k, m=m, classes=classes, connectivity=4 if k % 4 < 2 else 8, weight=weight))
    return out


def shape_cases():
    """the named shapes, small enough for the brute-force definition"""
    return [dict(name='checkerboard', m=CF.checkerboard(9, 11, 1, 2)), dict(name='rings', m=CF.nested_rings(7)), dict(name='serpentine', m=CF.serpentine(9, 8)),
            dict(name='combs', m=combs(7, 23)), dict(name='spiral', m=spiral(13)), dict(name='runs', m=run_count_map(37, 9)),
            dict(name='long run', m=long_run_map(40, 3, 33))]
