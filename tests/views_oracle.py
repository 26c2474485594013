"""Host model of the test-time views (include/wsi_hip.h: view id = T (1) | FY (2) | FX (4)) and the CPU restatement of the
cellularity scoring loop (reference utils/eval.py:307-336, :391-410) behind tests/golden/cellularity_views.npz.  Test helper only."""
import os

import numpy as np
import torch

from oracle import resnet_oracle as R
from wsi_segmentation_pipeline_amd import synthetic as W

VIEWS_REFERENCE = (0, 1, 2, 5)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cellularity_views.npz')


def apply_view(a, v, yx=(0, 1)):
    """View `v` of array `a` whose rows / columns are the axes `yx`: transpose first if T, then reverse the rows of the result if FY,
    then its columns if FX."""
    y, x = yx
    if v & 1:
        a = np.swapaxes(a, y, x)
    if v & 2:
        a = np.flip(a, y)
    if v & 4:
        a = np.flip(a, x)
    return np.ascontiguousarray(a)


def view_shape(v, ph, pw):
    return (pw, ph) if v & 1 else (ph, pw)


def compose(a, b):
    """The id of `apply a, then b` (on a square array), found by applying both to an index array."""
    idx = np.arange(16).reshape(4, 4)
    got = apply_view(apply_view(idx, a), b)
    return next(v for v in range(8) if np.array_equal(apply_view(idx, v), got))


def load_fixture():
    """The fixture as a dict, with the state dicts and u8 patches it names by seed rebuilt: 'sd' (ResNet-18 trunk), 'reg' (Regressor(512, 1)
    with the recorded constant added to fc.2.bias), 'cls' (Classifier(512, 4)), 'u8_sq' (6, 3, 64, 64), 'u8_ns' (3, 3, 64, 96)."""
    z = dict(np.load(FIXTURE))
    z['sd'] = W.make_resnet18_state_dict(int(z['weight_seed']), with_fc=False)
    reg = W.make_head_state_dict(int(z['regressor_seed']), 'regressor', 512, 1)
    reg['fc.2.bias'] = reg['fc.2.bias'] + torch.tensor(np.float32(z['fc2_bias_shift']))
    z['reg'] = reg
    z['cls'] = W.make_head_state_dict(int(z['classifier_seed']), 'classifier', 512, 4)
    z['u8_sq'] = W.make_u8_patches(int(z['input_seed_sq']), tuple(int(v) for v in z['input_shape_sq']))
    z['u8_ns'] = W.make_u8_patches(int(z['input_seed_ns']), tuple(int(v) for v in z['input_shape_ns']))
    return z


def restate(sd, reg, cls, u8_nchw, views=VIEWS_REFERENCE, trunk=R.trunk):
    """CPU restatement over the views of u8 patches (N, 3, H, W): (regressor outputs (N, V), classifier logits (N, V, 4)), fp32."""
    x = R.normalize_u8(u8_nchw).numpy()
    regs, clss = [], []
    with torch.no_grad():
        for v in views:
            fmap = trunk(sd, torch.from_numpy(apply_view(x, v, (2, 3))))
            regs.append(R.regressor(reg, fmap).view(-1).numpy())
            clss.append(R.classifier(cls, fmap).numpy())
    return np.stack(regs, 1), np.stack(clss, 1)


def mean_views(per_view):
    """((p0 + p1) + p2 + ...) / V in fp32 over axis 1, the reference's accumulation order."""
    acc = per_view[:, 0].astype(np.float32).copy()
    for k in range(1, per_view.shape[1]):
        acc = (acc + per_view[:, k].astype(np.float32)).astype(np.float32)
    return (acc / np.float32(per_view.shape[1])).astype(np.float32)

