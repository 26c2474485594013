"""Drop-in for the reference's ``utils.read_xml`` (BACH / Aperio ImageScope annotations, reference utils/read_xml.py:15-106)
with the reference's names and signatures.  The polygons are filled on the GPU at the sampled lattice points
(wsi_segmentation_pipeline_amd.annotations.rasterize) instead of by cv2.fillPoly on a full-resolution canvas; the coverage rule is
this project's own exact integer rule (tests/annotations_oracle.py), not cv2's.  Neither cv2 nor skimage is imported."""
import os

import numpy as np
from PIL import Image

from wsi_segmentation_pipeline_amd import annotations as A

COLORS = [(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)]      # red is 'benign', green is 'in situ' and blue is 'invasive'


def findExtension(directory, extension='.xml'):
    return sorted(f for f in os.listdir(directory) if f.endswith(extension))


def readXML(filename):
    """(coords, labels 1 / 2 / 3, lengths, areas, microns per pixel); an unknown label is a ValueError naming the region"""
    return A.read_imagescope(filename)


def one_hot_resize_argmax(labels, size):
    """The reference's way from a sampled label map to a level of another size (:88-91): the (R, G, B) one-hot image of classes
    1 / 2 / 3 through Image.resize (the installed Pillow's default filter) to size = (w, h), then argmax over (0, R, G, B)."""
    rgb = np.stack([(labels == k).astype(np.uint8) * 255 for k in (1, 2, 3)], -1)
    gt = np.asarray(Image.fromarray(rgb).convert('RGB').resize(tuple(size)))
    gt = np.concatenate((np.zeros((gt.shape[0], gt.shape[1], 1)), gt), axis=-1)
    return np.argmax(gt, axis=-1)


def sampled_labels(coords, labels, scan, sample):
    """every sample-th pixel of the full-resolution label canvas, (ceil(H0 / sample), ceil(W0 / sample)) u8 on the GPU"""
    w0, h0 = scan.level_dimensions[0]
    return A.rasterize(coords, labels, (-(-int(w0) // sample), -(-int(h0) // sample)), sample)


def getGT(xmlpath, scan, level):
    """Host integer (H, W) class map at `level`, as the reference makes it: every 4 ** level-th pixel of the label canvas; where that
    map already has the level's size it is the answer, otherwise it goes through one_hot_resize_argmax."""
    coords, labels = readXML(xmlpath)[:2]
    gt = sampled_labels(coords, labels, scan, 4 ** level).cpu().numpy()
    if (gt.shape[1], gt.shape[0]) == tuple(scan.level_dimensions[level]):
        return gt.astype(np.int64)
    return one_hot_resize_argmax(gt, scan.level_dimensions[level])


def getTB(gt, scan, level):
    """RGB PIL image at the level's size of the tumour bed of a class map with 1 = benign, 2 = dcis, 3 = invasive: the convex hull
    (taken on the GPU) of the malignant classes.  Like the reference it zeroes the benign pixels of `gt` in place."""
    import torch
    gt[gt == 1] = 0
    tb = A.tumor_bed_map(torch.from_numpy(np.ascontiguousarray(gt > 0).astype(np.uint8) * 2).cuda())
    return Image.fromarray(tb.cpu().numpy() * 255).convert('RGB').resize(scan.level_dimensions[level])
