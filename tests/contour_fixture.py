"""Label maps for the boundary tracer's tests (tests/test_contours_cpu.py, tests/test_gpu_contours.py): seeded random maps and the
shapes at which the kernels of csrc/contour.hip take another path.  NumPy only."""
import numpy as np

SCAN_CHUNK = 1024                        # csrc/map_kernels.h CHUNK: items (corners, edges) of one workgroup
SCAN_SPAN = 256 * 4                      # csrc/map_kernels.h SUMS_TILE: chunk sums the one scanning workgroup takes in one step of its loop
SCAN_SECOND = SCAN_CHUNK * 256           # an edge count of 256 scan chunks: a scan over many chunks, a quarter of the scanning workgroup's step
SCAN_STEP = SCAN_CHUNK * SCAN_SPAN       # items the scanning workgroup covers in one step of its loop


def noise_map(h, w, labels, seed):
    return np.random.default_rng(seed).integers(0, labels + 1, (h, w)).astype(np.uint8)


def blob_map(h, w, labels, seed, radius=3):
    """smooth blobs: box-filtered noise per label, the strongest label wins where it clears a threshold"""
    rng = np.random.default_rng(seed)
    k = 2 * radius + 1
    best, out = np.full((h, w), -1.0), np.zeros((h, w), np.uint8)
    for l in range(1, labels + 1):
        f = np.pad(rng.random((h, w)), radius, mode='wrap')
        c = np.cumsum(np.cumsum(np.pad(f, ((1, 0), (1, 0))), 0), 1)
        s = (c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]) / (k * k)
        take = s > best
        best[take], out[take] = s[take], l
    out[best < 0.5 + 0.15 / k] = 0
    return out


def checkerboard(h, w, a=1, b=0):
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x + y) % 2 == 0, a, b).astype(np.uint8)


def nested_rings(n, cycle=(1, 0, 2, 3)):
    """2 n - 1 pixels square, Chebyshev distance from the border picks the label: every ring encloses the next"""
    s = 2 * n - 1
    y, x = np.mgrid[0:s, 0:s]
    d = np.minimum(np.minimum(x, y), np.minimum(s - 1 - x, s - 1 - y))
    return np.asarray(cycle, np.uint8)[d % len(cycle)]


def serpentine(h, w, label=1):
    """one 1-pixel-wide path: full rows 0, 2, 4, ... joined alternately at the right and the left end.  One loop of 2 * pixels + 2 edges."""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = label
    for k, y in enumerate(range(1, h - 1, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = label
    return m


def serpentine_edges(h, w):
    rows = (h + 1) // 2
    return 2 * (rows * w + (rows - 1)) + 2


def row_loop(edges):
    """a 1 x m row of one label: one loop of 2 m + 2 edges"""
    assert edges % 2 == 0 and edges >= 4
    return np.ones((1, (edges - 2) // 2), np.uint8)


def edge_count_map(target, h, w):
    """a map with exactly `target` boundary edges (even, >= 4): isolated pixels of 4 edges on a checkerboard below row 2 and, where
    target = 2 mod 4, one domino of 6 edges in row 0"""
    assert target % 2 == 0 and target >= 4
    m = np.zeros((h, w), np.uint8)
    if target % 4 == 2:
        m[0, 0:2] = 2
        target -= 6
    ys, xs = np.nonzero(checkerboard(h - 2, w))
    assert target // 4 <= len(ys)
    m[ys[:target // 4] + 2, xs[:target // 4]] = 1
    return m


def isolated_pixels(h, w, label=1):
    """single pixels at even (x, y): no two touch, not even at a corner, so every pixel is a loop of 4 edges of its own"""
    m = np.zeros((h, w), np.uint8)
    m[0::2, 0::2] = label
    return m


def isolated_pixels_trace(h, w, step=(2, 2), origin=(0, 0), label=1):
    """what the spec gives for isolated_pixels(h, w), in closed form -> dict(vertices, first, count, edges, label, area2): the loops in
    raster order of their pixels, each from its top-left corner east, south, west (the spec's start and sense), area2 = 2"""
    ys, xs = np.nonzero(isolated_pixels(h, w, label))           # raster order: ascending smallest key
    n = len(ys)
    corners = np.stack((xs, ys), 1)[:, None, :] + np.asarray(((0, 0), (1, 0), (1, 1), (0, 1)))[None]
    s, o = np.asarray(step, np.int64), np.asarray(origin, np.int64)
    four = np.full(n, 4, np.int32)
    return dict(vertices=(o + corners.reshape(-1, 2) * s - s // 2).astype(np.int32), first=(4 * np.arange(n)).astype(np.int32), count=four, edges=four,
                label=np.full(n, label, np.int32), area2=np.full(n, 2, np.int64))


def sparse_rectangles(h, w):
    """a handful of small rectangles of three labels in an otherwise empty map: in the first rows, round row 1023, in the middle and in
    the last rows (the last one ends in the map's last row and column)"""
    m = np.zeros((h, w), np.uint8)
    for k, (y, x, rh, rw) in enumerate(((0, 3, 2, 5), (1019, 100, 9, 4), (h // 2, w // 2, 3, 3), (h // 3, w - 9, 4, 6), (h - 3, 40, 2, 7), (h - 2, w - 4, 2, 4))):
        m[max(0, min(y, h - rh)):max(0, min(y, h - rh)) + rh, x:x + rw] = 1 + k % 3
    return m


def random_cases(n, seed=11):
    """n seeded cases {m, classes, step, origin, bounds}: blobby and noisy maps of 1 - 4 labels up to 24 x 31, partial class sets (0
    included), steps 2 - 5, negative origins, and bounds that clamp the last column and row"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        h, w = int(rng.integers(1, 25)), int(rng.integers(1, 32))
        labels = int(rng.integers(1, 5))
        m = blob_map(h, w, labels, seed * 1000 + k, radius=1 + k % 3) if k % 2 else noise_map(h, w, labels, seed * 1000 + k)
        sx, sy = int(rng.integers(2, 6)), int(rng.integers(2, 6))
        classes = None if k % 3 == 0 else sorted({int(c) for c in rng.integers(0, labels + 1, int(rng.integers(1, labels + 2)))})
        if k % 4 == 3:                                          # clamped: the origin is 0 and the slide ends inside the last pixel's cell
            origin = (0, 0)
            bounds = ((w - 1) * sx + int(rng.integers(1, sx + 1)), (h - 1) * sy + int(rng.integers(1, sy + 1)))
        else:
            origin, bounds = (int(rng.integers(-7, 8)), int(rng.integers(-7, 8))), None
        out.append(dict(name='random%d' % k, m=m, classes=classes, step=(sx, sy), origin=origin, bounds=bounds))
    return out


def traced_part(m, table):
    return np.where(np.asarray(table, bool)[m], m, 0).astype(np.uint8)
