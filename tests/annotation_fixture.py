"""Small annotation files in the two XML formats the pipeline reads, written from plain lists - the writer of the annotation tests and of
tools/gen_golden_annotations.py (which records what the reference's readers make of the same files) - and the seeded polygons the
CPU and GPU tests share."""
import xml.etree.ElementTree as ET

import numpy as np

# (label text, where it goes: 'Value' attribute or the region's own 'Text', vertices)
IMAGESCOPE_REGIONS = [
    ('Benign', 'Value', [(10, 12), (200, 20), (180, 170), (30, 150)]),
    ('Carcinoma in situ', 'Value', [(300, 40), (420, 60), (400, 200), (310, 180), (280, 100)]),
    ('Carcinoma invasive', 'Text', [(100, 250), (350, 260), (330, 420), (220, 300), (120, 400)]),
    ('INVASIVE carcinoma', 'Value', [(50, 50), (60, 50), (60, 60)]),
    ('benign (in situ nearby)', 'Text', [(440, 300), (500, 300), (500, 380), (440, 380)]),
]

# (type, description, vertices as the text of the file: floats are truncated by the reader)
SEDEEN_GRAPHICS = [
    ('polygon', 'IDC', ['20.7,30.2', '400.9,35.0', '380.1,300.5', '40.0,280.99']),
    ('polygon', 'DCIS', ['500,100', '720,120', '700,330', '480,310']),
    ('polygon', 'no DCIS', ['100,400', '330,410', '320,600', '90,590']),
    ('polygon', 'benign', ['600,400', '790,400', '1200,640', '600,700']),          # leaves the 800 x 640 image: clamped
    ('polygon', 'UDH', ['10,10', '60,10', '60,300', '10,300']),                     # 50 wide: rejected by the 100-pixel rule
    ('polygon', 'cellularity 40', ['200,200', '400,200', '400,400', '200,400']),    # class 0: skipped
    ('point', 'i', ['300,300']),
    ('ellipse', 'invasive', ['100,100', '300,300']),
    ('text', 'DCIS', ['10,600']),
    ('polygon', 'TB 1', ['5,5', '795,8', '790,630', '8,620']),
    ('polyline', ' t b two', ['50,50', '300,60', '280,290', '60,270']),
    ('rectangle', 'I', ['420,450', '560,450', '560,600', '420,600']),
    ('polygon', 'Normal', ['0,0', '200,0', '200,200']),
]

LABEL_STRINGS = ['i', 'I', ' i ', 'IDC', 'idc 2', 'ILC', 'invasive', 'Invasive Carcinoma', 'DCIS', 'dcis', 'D C I S', 'no DCIS', 'No dcis', 'nodcis',
                 'no  DCIS here', 'UDH', 'udh ', 'benign', 'Benign 3', 'TB', 'TB 1', 'tb2', 't b', 'cellularity 40', 'Cellularity', 'cellularity idc',
                 'normal', 'Normal tissue', 'normal dcis', '', ' ', 'x', 'in', 'ii', 'milc', 'stroma', 'fat', 'DCIS + invasive', 'benign dcis',
                 'udh benign', 'Tumor Bed', 'tumorbed tb']


def write_imagescope(path, regions=IMAGESCOPE_REGIONS, mpp=0.467):
    root = ET.Element('Annotations', MicronsPerPixel='%.6f' % mpp)
    ann = ET.SubElement(root, 'Annotation', Id='1')
    ET.SubElement(ann, 'Attributes')
    regs = ET.SubElement(ann, 'Regions')
    for k, (text, where, verts) in enumerate(regions):
        r = ET.SubElement(regs, 'Region', Id=str(k + 1), LengthMicrons='%.3f' % (11.5 * (k + 1)), AreaMicrons='%.3f' % (101.25 * (k + 1)),
                          **({'Text': text} if where == 'Text' else {'Text': ''}))
        attrs = ET.SubElement(r, 'Attributes')
        if where == 'Value':
            ET.SubElement(attrs, 'Attribute', Name='label', Value=text)
        vs = ET.SubElement(r, 'Vertices')
        for x, y in verts:
            ET.SubElement(vs, 'Vertex', X=str(x), Y=str(y))
    ET.ElementTree(root).write(str(path))


def write_sedeen(path, graphics=SEDEEN_GRAPHICS):
    root = ET.Element('session', software='Sedeen Viewer')
    image = ET.SubElement(root, 'image', identifier='case')
    for tag in ('dimensions', 'pixel-size', 'transform'):
        ET.SubElement(image, tag)
    overlays = ET.SubElement(image, 'overlays')
    for k, (kind, description, points) in enumerate(graphics):
        g = ET.SubElement(overlays, 'graphic', type=kind, name='Region %d' % k, description=description)
        ET.SubElement(g, 'pen', color='#ff0000ff')
        ET.SubElement(g, 'font')
        pl = ET.SubElement(g, 'point-list')
        for p in points:
            ET.SubElement(pl, 'point').text = p
    ET.ElementTree(root).write(str(path))


def random_polygons(n=200, seed=5, lo=-10, hi=75, vmin=3, vmax=12):
    """n seeded polygons of vmin .. vmax - 1 vertices with coordinates in [lo, hi): many are self-intersecting"""
    rng = np.random.default_rng(seed)
    return [rng.integers(lo, hi, (int(rng.integers(vmin, vmax)), 2)) for _ in range(n)]


# ------------------------------------------------------------------------------------------------------------- rasteriser corpus
LIMIT = 1 << 29
SHAPES = {                                                       # on a 64 x 48 map at step 1
    'triangle': [(5, 4), (58, 11), (23, 44)],
    'rectangle': [(8, 6), (50, 6), (50, 40), (8, 40)],            # horizontal edges on scanlines: all four sides are covered
    'bow-tie': [(4, 4), (60, 44), (60, 4), (4, 44)],
    'pentagram': [(32, 2), (45, 45), (8, 17), (56, 17), (19, 45)],
    'spike same way': [(10, 5), (30, 20), (12, 40), (5, 40), (5, 5)],           # (30, 20) sits on a scanline between a falling and a falling edge
    'spike opposite ways': [(5, 30), (20, 10), (35, 30), (50, 10), (60, 30), (60, 45), (5, 45)],      # local extrema on scanlines
    'repeated and collinear': [(6, 6), (6, 6), (30, 6), (40, 6), (40, 6), (40, 20), (40, 30), (23, 30), (6, 30), (6, 18)],
    'one vertex': [(17, 9)],
    'two vertices': [(3, 40), (43, 10)],
    'two vertices, horizontal': [(9, 21), (33, 21)],
    'outside left': [(-40, 5), (-5, 10), (-20, 40)],
    'outside right': [(70, 5), (100, 10), (80, 40)],
    'outside above': [(5, -30), (50, -20), (30, -2)],
    'outside below': [(5, 50), (50, 60), (30, 90)],
    'partly outside': [(-25, -12), (40, -7), (75, 30), (20, 60), (-9, 22)],
    'encloses the map': [(-5, -5), (70, -8), (66, 55), (-3, 50)],
}
STEPS = ((1, 1), (4, 4), (16, 16), (3, 5))
ORIGINS = ((0, 0), (7, -3), (-40, -40))


def case(name, coords, labels, size=(64, 48), step=(1, 1), origin=(0, 0), fill=0):
    return {'name': name, 'coords': [np.asarray(c, np.int64).reshape(-1, 2) for c in coords], 'labels': [int(l) for l in labels],
            'size': size, 'step': step, 'origin': origin, 'fill': fill}


def shape_cases():
    """every shape under every step and origin, its vertices on the sampled lattice (scaled by the step, moved by the origin) and off it"""
    out = []
    for step in STEPS:
        for origin in ORIGINS:
            for off in ((0, 0), (1, 2)):
                for name, v in SHAPES.items():
                    vv = np.asarray(v, np.int64) * step + origin + off
                    out.append(case('%s, step %s, origin %s, offset %s' % (name, step, origin, off), [vv], [3], step=step, origin=origin))
    return out


def star(n, centre, r0, r1, seed):
    """a star-shaped polygon of n distinct-angle integer vertices around `centre`, radii in [r0, r1]"""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.random(n)) * 2 * np.pi
    rad = rng.uniform(r0, r1, n)
    return np.stack((centre[0] + np.rint(rad * np.cos(ang)), centre[1] + np.rint(rad * np.sin(ang))), 1).astype(np.int64)


def painter_cases():
    four = [[(5, 5), (40, 5), (40, 30), (5, 30)], [(20, 10), (60, 14), (50, 40)], [(10, 20), (55, 25), (30, 46), (12, 44)], [(25, 12), (45, 12), (45, 35), (25, 35)]]
    rng = np.random.default_rng(11)
    many = random_polygons(300, seed=12)
    return [case('four overlapping, the last one erasing', four, [1, 2, 3, 0]),
            case('300 random polygons', many, rng.integers(0, 4, 300)),
            case('painted over a map of 7s', four[:3], [1, 2, 0], fill=7),
            case('no polygon over a map of 7s', [], [], fill=7),
            case('no polygon', [], [])]


def chunk_cases(edge_chunk):
    """polygons whose edge counts sit around the kernel's staging chunk; every edge reaches the map, so the LDS slots fill up"""
    out = []
    for n in (edge_chunk - 1, edge_chunk, edge_chunk + 1, 3 * edge_chunk + 7):
        out.append(case('%d edges' % n, [star(n, (300, 200), 60, 290, n), [(0, 0), (600, 0), (0, 400)]], [2, 1], size=(150, 100), step=(4, 4)))
    return out


def geometry_cases():
    """widths around the 16-byte piece and the tile, heights around the tile, several tiles both ways"""
    out = []
    for k, (w, h) in enumerate([(1, 1), (15, 1), (16, 31), (17, 32), (255, 33), (257, 3), (1, 40), (1000, 70)]):
        polys = [star(int(n), (w * 0.5 + dx, h * 0.5 + dy), 0.1 * max(w, h), 0.7 * max(w, h) + 2, 100 * k + j)
                 for j, (n, dx, dy) in enumerate([(7, 0, 0), (23, w * 0.3, -h * 0.2), (5, -w * 0.4, h * 0.3), (40, 0, 0)])]
        out.append(case('%d x %d' % (w, h), polys, [1, 2, 3, 2], size=(w, h)))
    return out


def large_cases():
    """a thin triangle across the whole coordinate range, sampled at both ends: a 32-bit product gives other bytes"""
    L = LIMIT
    tri = [(-L, -L), (L, L - 40), (L - 40, L)]
    fat = [(-L, -L + 9), (L, -L), (L, L), (-L + 5, L)]
    out = []
    for origin, step in (((L - 1000, L - 1000), (1, 1)), ((L - 1000, L - 1000), (8, 15)), ((-L, -L), (1, 1)), ((-L, -L), (16, 16)),
                         ((-L, L - 63), (1 << 24, 1))):
        out.append(case('thin triangle, origin %s, step %s' % (origin, step), [fat, tri], [1, 2], size=(64, 64), step=step, origin=origin))
    return out


def all_cases(edge_chunk):
    return shape_cases() + painter_cases() + chunk_cases(edge_chunk) + geometry_cases() + large_cases()
