"""Drop-in for the reference's ``utils.read_xml_sunnybrook`` (Sunnybrook / Sedeen annotations,
reference utils/read_xml_sunnybrook.py:14-223) with the reference's names and signatures.

One deviation, stated: the reference draws each polygon's OUTLINE 8 pixels wide on the full-resolution canvas (cv2.polylines), keeps
every 8th pixel (every 2nd for the tumour bed), closes with a 10 x 10 box and fills the holes - a roundabout polygon fill whose cv2 line
drawing cannot be reproduced here.  This module fills the polygons directly, on the GPU, with the exact rule of
wsi_segmentation_pipeline_amd.annotations at the same sampling step (8 for getGT, 2 for getTB).  fillImage's two rules are kept: a
coordinate above the image size is clamped to size - 1, and a polygon whose box is not more than 100 in both directions is rejected.
Neither cv2 nor skimage nor scipy is imported."""
import os

import numpy as np
from PIL import Image

from utils.read_xml import one_hot_resize_argmax, sampled_labels
from wsi_segmentation_pipeline_amd import annotations as A

class_dictionary = A.class_dictionary


def findAnnotatedFiles(root_dir):
    """the xml files that have been annotated and padded properly"""
    return [os.path.join(path, f) for path, subdirs, files in os.walk(root_dir) for f in files if f.endswith('padded.session.xml')]


def mapToClass(label):
    """red is 'benign', green is 'in situ' and blue is 'invasive', the rest is black"""
    return {0: (0, 0, 0), 1: (255, 0, 0), 2: (0, 255, 0), 3: (0, 0, 255)}[class_dictionary(label)]


def readXML(filename):
    """(coords, descriptions) of the graphics of a class other than 0 and a type other than point / ellipse / text"""
    return A.read_sedeen(filename)


def readXML_TB(filename):
    """(coords, descriptions) of the graphics whose description contains `tb`"""
    return A.read_sedeen_tb(filename)


def _filled(coords, descriptions, scan, sample):
    coords, classes = A.sedeen_polygons(coords, [class_dictionary(d) for d in descriptions], scan.level_dimensions[0])
    return sampled_labels(coords, classes, scan, sample).cpu().numpy()


def getGT(xmlpath, scan, level):
    """Host integer (H, W) class map at `level`: the polygons filled at every 8th pixel, then - where that map has not the level's
    size - the reference's one-hot Image.resize and argmax over (0, R, G, B)."""
    gt = _filled(*readXML(xmlpath), scan, 8)
    if (gt.shape[1], gt.shape[0]) == tuple(scan.level_dimensions[level]):
        return gt.astype(np.int64)
    return one_hot_resize_argmax(gt, scan.level_dimensions[level])


def getTB(xmlpath, scan, level):
    """RGB PIL image at the level's size: the union of the `tb` graphics, filled at every 2nd pixel"""
    coords, labels = readXML_TB(xmlpath)
    tb = _filled(coords, ['benign' for _ in labels], scan, 2)
    return Image.fromarray((tb > 0).astype(np.uint8) * 255).convert('RGB').resize(scan.level_dimensions[level])
