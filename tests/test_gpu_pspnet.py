"""GPU parity of the PSPNet 'seg' model (ResNet encoder of either block type + smp's pyramid-pooling decoder: csrc/pspnet.hip for the
pyramid pool, the stage projection, the pyramid expand and the head's x8 upsample, the existing conv kernels for the fusing 1x1 conv and the
3x3 head; wsi_pspnet_* / wsi_pspnet_bneck_*) against the float64 CPU spec tests/pspnet_oracle.py: each single op, the decoder on a
caller-held map, the whole model under the project's ABSOLUTE 1e-3 contract at max |logit| 16, the launches one forward makes (the encoder
stops after layer 2), the u8 slide path, speed mode, the module surface and predict_tumorbed(mode='seg') with the model the smp-signature
factory returns.  Shapes are the smallest at which the code takes each of its paths, not the workload's."""
import json
import os

import numpy as np
import pytest
import torch

import pspnet_oracle as PO
import seg_model_checks as M
from oracle import resnet_oracle as R
from seg_model_checks import LOGIT_TOL, NEAR_TIE, SPEED_TOL, TAP_TOL, TOL_PARITY, TOL_SPEED, U8_TOL
from wsi_segmentation_pipeline_amd import synthetic as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R18, R34, R50, R101, B1 = [2, 2, 2, 2], [3, 4, 6, 3], [3, 4, 6, 3], [3, 4, 23, 3], [1, 1, 1, 1]
# (n, c, h, w): every bin the one pixel; a map smaller than 6 bins (bins repeat pixels); odd sizes with overlapping bins; non-square with
# 8 / 3 and 8 / 6; more images than one, 512 channels, bins of 2 x 2 repeating; more rows than one round of the kernel's 32 (planes 1: 16)
POOL_CASES = [(1, 128, 1, 1), (1, 128, 4, 4), (1, 128, 5, 7), (2, 128, 8, 12), (3, 512, 2, 2), (1, 128, 32, 32)]
PROJECT_CASES = [(1, 128), (3, 128), (1, 512), (3, 512)]
EXPAND_CASES = [(1, 1, 1), (2, 4, 4), (2, 8, 12), (1, 32, 32)]
HEAD_CASES = [('1x512x8x8 4 classes', (1, 8, 8), 4), ('2x512x8x8 1 class', (2, 8, 8), 1), ('2x512x4x6 16 classes', (2, 4, 6), 16)]
LOGIT_CASES = [('resnet18 3x64x64', 'basic', R18, (3, 64, 64)), ('resnet18 1x32x32', 'basic', R18, (1, 32, 32)),
               ('resnet18 2x64x96', 'basic', R18, (2, 64, 96)), ('resnet18 1x128x128', 'basic', R18, (1, 128, 128)),
               ('resnet34 1x64x64', 'basic', R34, (1, 64, 64)), ('[1, 1, 1, 1] basic 1x64x64', 'basic', B1, (1, 64, 64)),
               ('resnet50 2x64x64', 'bottleneck', R50, (2, 64, 64)), ('resnet101 1x64x64', 'bottleneck', R101, (1, 64, 64))]
MEASURED = {}             # what this run measured, by table and case; profiles/pspnet_parity.json was made from the printed PSPNET_MEASURED lines


def _record(table, key, value):
    MEASURED.setdefault(table, {})[key] = value
    print('PSPNET_MEASURED\t%s\t%s\t%.3e' % (table, key, value))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def sd():
    return W.make_pspnet_state_dict(31, R18, 4)


@pytest.mark.parametrize('shape', POOL_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_pyramid_pool_matches_float64(dev, shape):
    """The 50 bins of a PF map against float64 F.adaptive_avg_pool2d, in both line formats; the same bits on a second run (a fixed summation
    order, no atomics)."""
    from wsi_segmentation_pipeline_amd import engine as E
    n, c, h, w = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(100 + h * w + c)) * 3.0 + 1.0
    ref = PO.pyramid_pool(x)
    assert tuple(ref.shape) == (n, 50, c)
    errs = {}
    for planes, tol in ((2, TOL_PARITY), (1, TOL_SPEED)):
        run = lambda: E.pyramid_pool(E.pf_pack(x.to(dev), planes), n, h, w, c, planes)
        got = run()
        assert torch.equal(got, run())
        errs[planes] = M.rel(got, ref)
        _record('pool_rel_err', '%s planes %d' % ('x'.join(map(str, shape)), planes), errs[planes])
    assert errs[2] <= TOL_PARITY and errs[1] <= TOL_SPEED


@pytest.mark.parametrize('n,c', PROJECT_CASES, ids=['%dx50x%d' % s for s in PROJECT_CASES])
def test_stage_projection_matches_float64(dev, n, c):
    """relu([bn](stage conv)) and the stage's slice of the fusing conv on the 50 pooled pixels, fp32 FMA against float64, with the folded
    matrices of `unet.pspnet_fold` as the engine uploads them (transposed); both signs reach the ReLU."""
    from wsi_segmentation_pipeline_amd import engine as E
    from wsi_segmentation_pipeline_amd import unet
    ck = (W.make_pspnet_state_dict if c == 128 else W.make_pspnet_bottleneck_state_dict)(23, B1, 4)
    pooled = torch.randn(n, 50, c, generator=torch.Generator().manual_seed(n + c)).abs_() * 2.0
    mid0 = torch.nn.functional.conv2d(pooled[:, :1].transpose(1, 2).reshape(n, c, 1, 1), ck['decoder.psp.stages.0.pool.1.block.0.weight'])
    assert float(mid0.min()) < 0 < float(mid0.max())
    ref = PO.stage_terms(ck, pooled)
    fold = unet.pspnet_fold(ck, c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    got = E.pspnet_stage_project(pooled.to(dev), [t(a.T) for a in fold['stage_w']], [t(a) for a in fold['stage_b']], [t(a.T) for a in fold['proj_w']])
    assert tuple(got.shape) == tuple(ref.shape) == (n, 50, 512)
    err = M.rel(got, ref)
    _record('project_rel_err', '%dx50x%d' % (n, c), err)
    assert err <= TOL_PARITY


def _real_byte_mask(lib, n, h, w, pix_bytes, total):
    """True for the bytes of the real pixels' records of a PF buffer, False for the pad ring and the guards"""
    mask = np.zeros(total, bool)
    for i in range(n):
        for y in range(h):
            a = lib.wsi_pf_pixel_index(i, y, 0, h, w) * pix_bytes
            mask[a:a + w * pix_bytes] = True
    return mask


@pytest.mark.parametrize('n,h,w', EXPAND_CASES, ids=['%dx%dx%d' % s for s in EXPAND_CASES])
def test_pyramid_expand_matches_float64_and_leaves_the_pad_ring(dev, n, h, w):
    """Per pixel the sum of the bilinear samples (align_corners=True) of the four grids against float64 F.interpolate, in both line formats;
    a 1 x 1 map (every scale 0), maps smaller and larger than the grids.  The buffer starts as the byte 0x5A everywhere: afterwards only
    the real pixels' records differ."""
    from wsi_segmentation_pipeline_amd import engine as E
    from wsi_segmentation_pipeline_amd import native
    lib = native.load()
    terms = torch.randn(n, 50, 512, generator=torch.Generator().manual_seed(h * w + n)) * torch.linspace(0.5, 4.0, 50).reshape(1, 50, 1)
    ref = PO.expand(terms, (h, w))
    errs = {}
    for planes, tol in ((2, TOL_PARITY), (1, TOL_SPEED)):
        out = torch.full((lib.wsi_pf_bytes(n, h, w, 512, planes),), 0x5A, dtype=torch.uint8, device=dev)
        E.pyramid_expand(terms.to(dev), n, h, w, planes, out=out)
        raw = out.cpu().numpy()
        real = _real_byte_mask(lib, n, h, w, 512 * (2 if planes == 1 else 4), raw.size)
        assert (raw[~real] == 0x5A).all() and (~real).sum() > 0
        errs[planes] = M.rel(E.pf_unpack(out, n, 512, h, w, planes), ref)
        _record('expand_rel_err', '%dx%dx%d planes %d' % (n, h, w, planes), errs[planes])
    assert errs[2] <= TOL_PARITY and errs[1] <= TOL_SPEED


@pytest.mark.parametrize('name,shape,classes', HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_head_conv_up8_matches_float64(dev, name, shape, classes):
    """final_conv (3x3, padding 1, bias; its output channels zero-padded to one line for the conv kernel) and the bilinear x8
    (align_corners=True) against float64; signed outputs, 1 ... 16 classes."""
    from wsi_segmentation_pipeline_amd import engine as E
    n, h, w = shape
    g = torch.Generator().manual_seed(700 + h * w + classes)
    x = torch.randn(n, 512, h, w, generator=g).abs_()
    head = {'decoder.final_conv.weight': torch.randn(classes, 512, 3, 3, generator=g) * (2.0 / (512 * 9)) ** 0.5,
            'decoder.final_conv.bias': torch.randn(classes, generator=g)}
    ref, refq = PO.head(head, x)
    assert tuple(ref.shape) == (n, classes, 8 * h, 8 * w) and float(ref.min()) < 0 < float(ref.max())
    errs = {}
    for planes, tol in ((2, TOL_PARITY), (1, TOL_SPEED)):
        line = 64 if planes == 1 else 32
        wp, bp = torch.zeros(line, 512, 3, 3), torch.zeros(line)
        wp[:classes], bp[:classes] = head['decoder.final_conv.weight'], head['decoder.final_conv.bias']
        wpk, zero = E.prepack_conv(wp, None, planes, dev)
        assert not zero.any()
        got = E.pspnet_head_up8(E.pf_pack(x.to(dev), planes), wpk, bp.to(dev), n, h, w, classes, planes)
        errs[planes] = M.rel(got, ref)
        _record('head_rel_err', '%s planes %d' % (name, planes), errs[planes])
        scale = float(refq.abs().max())                                             # the output's corners are the 1/8 map's corners
        for yo, xo in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
            assert float((got[:, :, yo, xo].cpu().double() - refq[:, :, yo, xo]).abs().max()) <= (TOL_PARITY if planes == 2 else TOL_SPEED) * scale
    assert errs[2] <= TOL_PARITY and errs[1] <= TOL_SPEED


def _checkpoint(arch, layers):
    return W.make_pspnet_bottleneck_state_dict(31, layers, 4) if arch == 'bottleneck' else W.make_pspnet_state_dict(31, layers, 4)


@pytest.mark.parametrize('arch', ['basic', 'bottleneck'])
def test_decoder_on_a_caller_held_map(dev, arch):
    """wsi_pspnet_decoder / wsi_pspnet_bneck_decoder with enc_nchw = {NULL, NULL, x2, NULL, NULL} against pspnet_oracle.decoder on the same
    fp32 map, a 4 x 12 map of one image and of three."""
    from wsi_segmentation_pipeline_amd.unet import PSPNetEngine
    ck = _checkpoint(arch, B1)
    for n in (1, 3):
        x = R.normalize_u8(W.make_u8_patches(51 + n, (n, 3, 32, 96)))
        ck16, ref, ref_enc, _ = M.scaled_to_logit(PO, ck, x)
        eng = PSPNetEngine(ck16, dev, planes=2)
        got = eng.decode([None, None, ref_enc[2].to(dev), None, None])
        err = float((got.cpu().double() - ref).abs().max())
        _record('decoder_abs_err', '%s %dx32x96' % (arch, n), err)
        assert got.shape == ref.shape == (n, 4, 32, 96) and err <= LOGIT_TOL


@pytest.mark.parametrize('name,arch,layers,shape', LOGIT_CASES, ids=[c[0] for c in LOGIT_CASES])
def test_logits_hold_the_absolute_contract(dev, name, arch, layers, shape):
    """Whole forward, and model.decoder(model.encoder(x)) through fp32 NCHW maps, against the float64 spec at max |logit| 16; the logits of
    a run that also returns the five maps are bit for bit those of a run that stops after layer 2.  No case is damped: the decoder reads
    layer 2's output, and for resnet101 in particular layer 3 - whose 23 blocks are what grows a seeded draw - never runs on the logits'
    path; every map the line formats carry on that path is asserted to be inside the fp16 range (with enc=True the resnet101 draw's x3 and
    x4 leave it, 1.7e5: nothing here reads those two maps).  Arg-max flips are held to 0.002 where at most NEAR_TIE
    of the spec's own pixels are near-ties (a flip needs one)."""
    from wsi_segmentation_pipeline_amd.unet import PSPNetEngine
    n, h, w = shape
    x = R.normalize_u8(W.make_u8_patches(41 + h + w, (n, 3, h, w)))
    sd16, ref, ref_enc, maps = M.scaled_to_logit(PO, _checkpoint(arch, layers), x)
    assert abs(float(ref.abs().max()) - 16.0) < 1e-3
    assert max(float(t.abs().max()) for t in list(ref_enc[2:]) + maps) < 6e4       # inside the fp16 range of the line format
    eng = PSPNetEngine(sd16, dev, planes=2)
    assert eng.arch == arch and eng.trunk.layers == layers
    alone = eng.forward_f32(x.to(dev))[0].clone()
    got, enc = eng.forward_f32(x.to(dev), logits=True, enc=True)
    assert torch.equal(alone, got)
    two = eng.decode(enc)
    assert got.shape == ref.shape == (n, 4, h, w)
    err, err2 = float((got.cpu().double() - ref).abs().max()), float((two.cpu().double() - ref).abs().max())
    d12 = float((two - got).abs().max())
    # (the maps of layers 3 and 4 are the trunk's business - tests/test_gpu_resnet34.py, test_gpu_resnet50.py; here: what the decoder reads)
    e2 = float((enc[2].cpu() - ref_enc[2]).abs().max() / ref_enc[2].abs().max())
    flips, share = float((got.cpu().argmax(1) != ref.argmax(1)).float().mean()), M.near_tie_share(ref)
    print('pspnet %s parity: max |logit - spec| %.3e (decoder(encoder(x)): %.3e, between the two %.3e) ABSOLUTE at max |logit| 16; x2 rel err '
          '%.2e; arg-max flips %.5f, near-tie share %.5f' % (name, err, err2, d12, e2, flips, share))
    _record('logit_abs_err', name, max(err, err2))
    _record('x2_rel_err', name, e2)
    assert e2 <= TAP_TOL[arch]
    assert err <= LOGIT_TOL and err2 <= LOGIT_TOL and d12 <= LOGIT_TOL
    if share <= NEAR_TIE:
        assert flips <= 0.002


@pytest.mark.parametrize('arch,layers', [('basic', R34), ('bottleneck', R50)], ids=['resnet34', 'resnet50'])
def test_routes_of_one_forward(dev, arch, layers):
    """The profiler's records of one (2, 64, 64) forward.  Without enc_out the encoder stops after layer 2: the stem (4), then exactly the
    convs of layers 1 and 2 by the depth table - BasicBlock: 2 per block (kinds 5, 2, 1); Bottleneck: 3 per block plus one downsample per
    stage (kinds 11, 1, 2, 3) - no x0 glue (7), and the decoder [pool (18), projection (19), expand (20), fusing 1x1 (12), 3x3 head (6),
    x8 upsample (21)].  With the five maps requested the whole encoder runs, the maps are those of the trunk's own tap entry, and the
    logits are bit for bit the same."""
    from wsi_segmentation_pipeline_amd import native
    from wsi_segmentation_pipeline_amd.unet import PSPNetEngine
    ck = _checkpoint(arch, layers)
    x = R.normalize_u8(W.make_u8_patches(43, (2, 3, 64, 64))).to(dev)
    eng = PSPNetEngine(ck, dev, planes=2)
    eng.forward_f32(x)                                                              # (plans the workspace outside the recording)
    out = {}
    rec = native.profiled(lambda: out.update(alone=eng.forward_f32(x)[0].clone()), 512)[1]
    rec_enc = native.profiled(lambda: out.update(full=eng.forward_f32(x, enc=True)), 512)[1]
    kinds, kinds_enc = [k for k, _ in rec], [k for k, _ in rec_enc]
    print('prof kinds, pspnet %s: %r; with enc=True %r' % (arch, kinds, kinds_enc))
    decoder = [18, 19, 20, 12, 6, 21]
    per_block, per_stage = (3, 1) if arch == 'bottleneck' else (2, 0)
    convs = lambda stages: sum(per_block * layers[s] + per_stage for s in range(stages))
    assert kinds[0] == 4 and kinds[-6:] == decoder and 7 not in kinds and 9 not in kinds
    assert len(kinds) == 1 + convs(2) + 6 and all(k in (1, 2, 3, 5, 11) for k in kinds[1:-6])
    assert kinds_enc[-6:] == decoder and kinds_enc.count(7) == 1 and 9 not in kinds_enc
    assert len(kinds_enc) == 1 + convs(4) + 1 + 6
    assert all(f == 0.0 for k, f in rec if k in (18, 19, 20, 21))
    c = eng.enc_ch[2]
    assert [f for k, f in rec if k == 12][-1] == 2.0 * 2 * 8 * 8 * c * 512 and [f for k, f in rec if k == 6][-1] == 2.0 * 2 * 8 * 8 * 512 * 32 * 9
    logits, enc = out['full']
    assert torch.equal(logits, out['alone'])
    for i, layer in enumerate((4, 3, 2, 1)):
        tap = eng.trunk.forward_f32(x, tap=sum(layers[:layer]))
        err = float((enc[i] - tap).abs().max() / tap.abs().max())
        assert enc[i].shape == tap.shape and err <= TAP_TOL[arch], (layer, err)
    assert tuple(enc[4].shape) == (2, 64, 32, 32) and float(enc[4].abs().max()) > 0


def test_u8_slide_path_equals_f32_path(dev, sd):
    """forward_tiles on a 200 x 260 slide, four 64 x 64 tiles, one hanging over the edge, against forward_f32 of the gathered tiles."""
    from wsi_segmentation_pipeline_amd.unet import PSPNetEngine
    err, scale = M.u8_slide_path_equals_f32_path(PSPNetEngine, PO, sd, dev)
    _record('u8_slide_vs_f32_path', 'err over scale', err / scale)


def test_speed_mode_is_sane(dev, sd):
    """planes 1 (single-pass bf16): outside the contract; finite logits, and x2 (the map the decoder reads), within 0.1 of the spec's maximum."""
    from wsi_segmentation_pipeline_amd.unet import PSPNetEngine
    err, _ = M.speed_mode_is_sane(PSPNetEngine, PO, sd, dev, R.normalize_u8(W.make_u8_patches(45, (3, 3, 64, 64))), enc_index=2)
    _record('speed_mode', 'logits rel err', err)


def test_module_surface_and_mx_refusal(dev, sd):
    """model(x), model.encoder(x), model.decoder(encoding) in eval mode run on the engine; a CPU tensor is refused."""
    from wsi_segmentation_pipeline_amd import unet
    M.module_surface_and_mx_refusal(unet.PSPNet, unet.PSPNetEngine, PO, sd, dev)


def test_predict_tumorbed_seg_with_the_factory_model(dev, sd, tmp_path, monkeypatch):
    """predict_tumorbed(mode='seg') with unet.PSPNet('resnet18', classes=4) on the slide of tests/test_gpu_fpn.py: the fused tile path is the
    one taken (the PSPNet engine reads the tiles from the device-resident level), the class map and the heat map against the CPU chain
    (float64 spec -> float64 stitch -> threshold / heat map): heat pixels off by more than 1 LSB and class flips at most 0.002 each, where
    at most NEAR_TIE of the spec's own tile pixels are near-ties (checked on the CPU for this slide seed: 4e-5, so the rule applies)."""
    from wsi_segmentation_pipeline_amd import unet
    model = unet.PSPNet('resnet18', encoder_weights=None, classes=4, activation=None)
    M.predict_tumorbed_seg(model, lambda eng: type(eng) is unet.PSPNetEngine, PO, sd, tmp_path, monkeypatch, heat=True, near_tie_max=NEAR_TIE)


def test_recorded_bounds_match_the_profile():
    """profiles/pspnet_parity.json holds the values measured on an MI355X, one per case of the tests above; they are inside the bounds."""
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'pspnet_parity.json')))
    assert rec['per_op_bound'] == {'parity': TOL_PARITY, 'speed': TOL_SPEED} and rec['logit_bound'] == LOGIT_TOL
    assert rec['x2_bound'] == TAP_TOL and rec['u8_slide_vs_f32_path']['bound_times_scale'] == U8_TOL and rec['speed_mode']['bound'] == SPEED_TOL
    both = lambda keys: {'%s planes %d' % (k, p) for k in keys for p in (2, 1)}
    assert set(rec['pool_rel_err']) == both('x'.join(map(str, s)) for s in POOL_CASES)
    assert set(rec['project_rel_err']) == {'%dx50x%d' % s for s in PROJECT_CASES}
    assert set(rec['expand_rel_err']) == both('%dx%dx%d' % s for s in EXPAND_CASES)
    assert set(rec['head_rel_err']) == both(c[0] for c in HEAD_CASES)
    assert set(rec['logit_abs_err']) == set(rec['x2_rel_err']) == {c[0] for c in LOGIT_CASES}
    assert set(rec['decoder_abs_err']) == {'%s %dx32x96' % (a, n) for a in ('basic', 'bottleneck') for n in (1, 3)}
    for table in ('pool_rel_err', 'expand_rel_err', 'head_rel_err'):
        assert all(v <= (TOL_PARITY if k.endswith('planes 2') else TOL_SPEED) for k, v in rec[table].items()), table
    assert all(v <= TOL_PARITY for v in rec['project_rel_err'].values())
    assert all(v <= LOGIT_TOL for v in list(rec['logit_abs_err'].values()) + list(rec['decoder_abs_err'].values()))
    assert all(v <= TAP_TOL['bottleneck' if ('resnet50' in k or 'resnet101' in k) else 'basic'] for k, v in rec['x2_rel_err'].items())
    assert rec['u8_slide_vs_f32_path']['err over scale'] <= U8_TOL and rec['speed_mode']['logits rel err'] <= SPEED_TOL
