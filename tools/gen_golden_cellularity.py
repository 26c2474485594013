#!/usr/bin/env python3
"""Generate tests/golden/cellularity_views.npz by running the REFERENCE's own modules through its test-time augmentation loop
(utils/eval.py:307-336 predict_reg, :391-410 predict_breastpathq).

Run from the repo root:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_cellularity.py

The reference's `resnets_shift.resnet18(False)` and `models.models.Regressor(512, 1)` / `Classifier(512, 4)` are imported read-only
through oracle.gen_golden.load_reference; nothing of them is copied.  The encoder is the net's own conv1 ... layer4 stack (the
arithmetic smp's encoder wrapper runs; the wrapper itself stays unpinned), weights `make_resnet18_state_dict(WEIGHT_SEED,
with_fc=False)`, heads `make_head_state_dict`.  Inputs: `make_u8_patches` of (6, 3, 64, 64) and of (3, 3, 64, 96) through the
transform arithmetic; the four views are the reference's torch expressions.  Only seeds, shapes and OUTPUTS are written.

A constant is added to the regressor's `fc.2.bias` (recorded as `fc2_bias_shift`) so that the clamp of :409-410 is exercised: at
least one clamped score is exactly 0 and at least one lies strictly inside (0, 1).  The generator asserts that, and: max |output|
<= 16 (the range the 1e-3 contract is stated for); for every pair of views the largest difference of the regressor outputs over the
patches of a set is >= 0.02 (20 x the bound: a swapped or mis-oriented view cannot pass the per-view check); oracle.resnet_oracle's
CPU restatement reproduces every stored value to 1e-5.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.gen_golden import load_reference                              # noqa: E402
from oracle.resnet_oracle import normalize_u8                             # noqa: E402  (transform arithmetic only)
from wsi_segmentation_pipeline_amd import synthetic as W                  # noqa: E402
from tools.gen_golden_resnet50 import save_npz_stable                     # noqa: E402
import views_oracle as VO                                                 # noqa: E402

WEIGHT_SEED, REGRESSOR_SEED, CLASSIFIER_SEED = 31, 32, 33
INPUTS = {'sq': (34, (6, 3, 64, 64)), 'ns': (35, (3, 3, 64, 96))}
MIN_VIEW_GAP = 0.02
OUT = os.path.join(ROOT, 'tests', 'golden', 'cellularity_views.npz')


def main():
    torch.set_num_threads(8)
    rs, mm, _ = load_reference()
    net = rs.resnet18(False)
    sd = W.make_resnet18_state_dict(WEIGHT_SEED, with_fc=False)
    missing = net.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all(k.startswith('fc') for k in missing.missing_keys), missing
    reg, cls = mm.Regressor(512, 1), mm.Classifier(512, 4)
    reg_sd = W.make_head_state_dict(REGRESSOR_SEED, 'regressor', 512, 1)
    cls_sd = W.make_head_state_dict(CLASSIFIER_SEED, 'classifier', 512, 4)
    reg.load_state_dict(reg_sd)
    cls.load_state_dict(cls_sd)
    for m in (net, reg, cls):
        m.eval()

    def encoder(x):
        x = net.maxpool(net.relu(net.bn1(net.conv1(x))))
        return [net.layer4(net.layer3(net.layer2(net.layer1(x))))]

    def run(image):
        augmented_set = [image, image.transpose(2, 3), image.flip(2), image.transpose(2, 3).flip(3)]
        regs, clss = [], []
        with torch.no_grad():
            for image_ in augmented_set:
                encoding = encoder(image_.contiguous())
                regs.append(reg(encoding[0]).view(-1).clone())
                clss.append(cls(encoding[0]).clone())
        pred = None
        for r in regs:                                                    # pred_cls_ = ...; pred_cls_ += ...; / len(augmented_set)
            pred = r.clone() if pred is None else pred.add_(r)
        return torch.stack(regs, 1).numpy(), (pred / len(augmented_set)).numpy(), torch.stack(clss, 1).numpy()

    images = {name: normalize_u8(W.make_u8_patches(seed, shape)) for name, (seed, shape) in INPUTS.items()}
    raw = run(images['sq'])[1]
    order = np.sort(raw)
    shift = np.float32(-0.5 * (float(order[len(order) // 2 - 1]) + float(order[len(order) // 2])))       # the median lands on 0
    with torch.no_grad():
        reg.fc[2].bias.add_(float(shift))
    reg_sd['fc.2.bias'] = reg_sd['fc.2.bias'] + torch.tensor(shift)
    assert torch.equal(reg.fc[2].bias.detach(), reg_sd['fc.2.bias'])

    rec = dict(weight_seed=WEIGHT_SEED, regressor_seed=REGRESSOR_SEED, classifier_seed=CLASSIFIER_SEED, fc2_bias_shift=shift,
               views=np.array(VO.VIEWS_REFERENCE))
    clamped_all = []
    for name, (seed, shape) in INPUTS.items():
        pv, mean, logits = run(images[name])
        clamped = np.minimum(np.maximum(mean, 0.0), 1.0)
        clamped_all.append(clamped)
        amax = max(float(np.abs(pv).max()), float(np.abs(logits).max()))
        gaps = {(a, b): float(np.abs(pv[:, a] - pv[:, b]).max()) for a in range(4) for b in range(a + 1, 4)}
        print('%s: |regressor| %.3f .. %.3f, max |logit| %.3f, smallest view-pair gap %.4f, clamped %s'
              % (name, float(np.abs(pv).min()), float(np.abs(pv).max()), float(np.abs(logits).max()), min(gaps.values()), clamped))
        assert amax <= 16.0, 'outputs outside the range the contract is stated for'
        assert min(gaps.values()) >= MIN_VIEW_GAP, ('two views are too close for the per-view check to tell them apart', gaps)
        assert np.array_equal(mean, VO.mean_views(pv)), 'the stated accumulation order is not the reference\'s'
        r_pv, r_logits = VO.restate(sd, reg_sd, cls_sd, W.make_u8_patches(seed, shape))
        err = max(float(np.abs(r_pv - pv).max()), float(np.abs(r_logits - logits).max()))
        print('%s: CPU restatement max error %.2e' % (name, err))
        assert err <= 1e-5, err
        rec.update({'input_seed_' + name: seed, 'input_shape_' + name: np.array(shape), 'reg_views_' + name: pv, 'reg_mean_' + name: mean,
                    'reg_clamped_' + name: clamped, 'cls_views_' + name: logits})
    c = np.concatenate(clamped_all)
    assert (c == 0.0).any() and ((c > 0.0) & (c < 1.0)).any(), c
    save_npz_stable(OUT, rec)
    print('wrote %s: %d bytes' % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
