#!/usr/bin/env python3
"""Write tests/golden/annotation_parse.json: what the REFERENCE's own annotation readers make of two small XML files and of a list of
label strings.  Run from the repository root, where the reference tree is present:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_annotations.py

The reference's utils.read_xml (readXML) and utils.read_xml_sunnybrook (readXML, readXML_TB, class_dictionary, mapToClass) are imported
read-only behind the stub finder for absent packages of oracle/gen_golden.py (cv2 and skimage are imported by those modules and never
executed here).  The XML files come from the writer of the tests (tests/annotation_fixture.py).  Only recorded results are written:
coordinates, labels and classes - no program text."""
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import annotation_fixture as AF                      # noqa: E402
from oracle import gen_golden as G                   # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as d:
        isc, sed = os.path.join(d, 'imagescope.xml'), os.path.join(d, 'sedeen.session.xml')
        AF.write_imagescope(isc)
        AF.write_sedeen(sed)
        with G.reference_utils():
            import importlib
            rx = importlib.import_module('utils.read_xml')
            rs = importlib.import_module('utils.read_xml_sunnybrook')
            assert os.path.abspath(rx.__file__).startswith(G.REF) and os.path.abspath(rs.__file__).startswith(G.REF)
            coords, labels, length, area, mpp = rx.readXML(isc)
            s_coords, s_labels = rs.readXML(sed)
            t_coords, t_labels = rs.readXML_TB(sed)
            out = {
                'imagescope': {'coords': coords, 'labels': labels, 'length': length, 'area': area, 'mpp': mpp},
                'sedeen': {'coords': [[list(p) for p in c] for c in s_coords], 'labels': s_labels},
                'sedeen_tb': {'coords': [[list(p) for p in c] for c in t_coords], 'labels': t_labels},
                'class_dictionary': [[s, rs.class_dictionary(s)] for s in AF.LABEL_STRINGS],
                'mapToClass': [[s, list(rs.mapToClass(s))] for s in AF.LABEL_STRINGS],
            }
    path = os.path.join(ROOT, 'tests', 'golden', 'annotation_parse.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s: %d + %d + %d polygons, %d label strings' % (path, len(coords), len(s_coords), len(t_coords), len(AF.LABEL_STRINGS)))


if __name__ == '__main__':
    main()
