"""What the model-level GPU tests of the segmentation families share (tests/test_gpu_linknet.py, test_gpu_unet_bottleneck.py,
test_gpu_fpn.py, test_gpu_pspnet.py): the bounds, the three small measures and the bodies of the checks that read the same in every
family - the u8 slide path, speed mode, the module surface and predict_tumorbed(mode='seg').  A plain module, imported like the
``*_oracle.py`` files.  A check takes the family's factory, engine class, spec (a module with ``forward(sd, x) -> (logits, maps)`` and
``decoder(sd, maps, maps=None)``) and state dict; what a family does differently is an argument its test file passes, or stays in that
file."""
import numpy as np
import pytest
import torch

from oracle import resnet_oracle as R
from oracle import wsi_oracle as WO
from wsi_segmentation_pipeline_amd import synthetic as W

TOL_PARITY = 2e-5         # tests/test_gpu_kernels.py: one op, relative to the tensor's maximum, fp16 hi + lo pair (and fp32 arithmetic)
TOL_SPEED = 3e-2          # ... single-pass bf16
LOGIT_TOL = 1e-3          # BASELINE.json north_star: absolute, on logits of magnitude 16
TAP_TOL = {'basic': 7e-6, 'bottleneck': 2e-4}   # tests/test_gpu_resnet34.py TAP_TOL[2] / tests/test_gpu_resnet50.py TAP_TOL: encoder maps, relative to the map's maximum
U8_TOL = 2e-5             # tests/test_gpu_resnet50.py::test_u8_slide_path_equals_f32_path: u8 slide path against the f32 path, times the f32 path's maximum
SPEED_TOL = 0.1           # tests/test_gpu_resnet50.py::test_speed_mode_is_sane: speed mode, finite and within 0.1 of the maximum
NEAR_TIE = 0.0005         # arg-max flips are asserted only where at most this share of the spec's pixels has a top-two margin < 2 LOGIT_TOL


def rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def near_tie_share(ref):
    top = ref.topk(2, 1).values
    return float(((top[:, 0] - top[:, 1]) < 2 * LOGIT_TOL).double().mean())


def scaled_to_logit(oracle, sd, x, target=16.0):
    """final_conv scaled until the spec's max |logit| on these inputs is `target` (tests/test_gpu_unet.py: the contract is absolute on
    logits of the size trained heads produce).  Returns (state dict, spec logits, spec encoder maps, every decoder map the spec lists)."""
    with torch.no_grad():
        ref, enc = oracle.forward(sd, x)
    s = target / float(ref.abs().max())
    sd = dict(sd)
    for key in ('decoder.final_conv.weight', 'decoder.final_conv.bias'):
        sd[key] = sd[key] * s
    maps = []
    with torch.no_grad():
        return sd, oracle.decoder(sd, enc, maps=maps), enc, maps


def u8_slide_path_equals_f32_path(engine, oracle, sd, dev):
    """forward_tiles on a 200 x 260 slide, four 64 x 64 tiles, one hanging over the edge, against forward_f32 of the gathered tiles, at
    max |logit| 16: within U8_TOL of the f32 path's maximum.  Returns (error, that maximum)."""
    rng = np.random.default_rng(7)
    slide = rng.integers(0, 256, (200, 260, 3), dtype=np.uint8)
    xy = np.array([[0, 0], [100, 50], [260 - 64, 200 - 64], [230, 170]], np.int32)
    tiles = np.stack([WO.read_tile(slide, int(x), int(y), 64, 64) for x, y in xy]).transpose(0, 3, 1, 2)
    x = R.normalize_u8(tiles)
    sd16 = scaled_to_logit(oracle, sd, x)[0]
    eng = engine(sd16, dev, planes=2)
    b = eng.forward_f32(x.to(dev))[0].clone()
    a = eng.forward_tiles(torch.from_numpy(slide).to(dev), torch.from_numpy(xy).to(dev), 64, 64).clone()
    scale, err = float(b.abs().max()), float((a - b).abs().max())
    print('%s u8 slide path vs f32 path: %.3e of scale %.3e (bound %.1e)' % (engine.__name__, err, scale, U8_TOL * scale))
    assert a.shape == b.shape == (4, 4, 64, 64)
    assert err <= U8_TOL * scale
    return err, scale


def speed_mode_is_sane(engine, oracle, sd, dev, x, enc_index=0):
    """planes 1 (single-pass bf16): outside the contract; finite logits, and encoder map `enc_index`, within SPEED_TOL of the spec's
    maximum at max |logit| 16.  Returns the two errors."""
    sd16, ref, ref_enc, _ = scaled_to_logit(oracle, sd, x)
    eng = engine(sd16, dev, planes=1)
    got, enc = eng.forward_f32(x.to(dev), logits=True, enc=True)
    err, e_map = rel(got, ref), rel(enc[enc_index], ref_enc[enc_index])
    print('%s speed mode: logits rel err %.2e, encoder map %d rel err %.2e' % (engine.__name__, err, enc_index, e_map))
    assert np.isfinite(err) and err <= SPEED_TOL and np.isfinite(e_map) and e_map <= SPEED_TOL
    return err, e_map


def module_surface_and_mx_refusal(factory, engine, oracle, sd, dev):
    """model(x), model.encoder(x), model.decoder(encoding) of the factory's resnet18 model in eval mode run on the engine; a CPU tensor is
    refused, and so is mx precision."""
    model = factory('resnet18', encoder_weights=None, classes=4, activation=None)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    x = R.normalize_u8(W.make_u8_patches(46, (2, 3, 64, 64)))
    with torch.no_grad():
        ref = oracle.forward(sd, x)[0]
        y = model(x.cuda())
        enc = model.encoder(x.cuda())
        y2 = model.decoder(enc)
    assert isinstance(model.hip_engine(dev), engine)
    assert [tuple(t.shape[1:]) for t in enc] == [(512, 2, 2), (256, 4, 4), (128, 8, 8), (64, 16, 16), (64, 32, 32)]
    scale = float(ref.abs().max())
    assert float((y.cpu().double() - ref).abs().max()) <= 2e-4 * scale and float((y2.cpu().double() - ref).abs().max()) <= 4e-4 * scale
    with pytest.raises(RuntimeError):
        model(x)
    with pytest.raises(ValueError, match='mx'):
        engine(sd, dev, planes=3)


def predict_tumorbed_seg(model, is_engine, oracle, sd, tmp_path, monkeypatch, heat=True, near_tie_max=None):
    """predict_tumorbed(mode='seg') with `model` (a factory's model, `sd` not yet loaded) on the slide of
    tests/test_gpu_unet.py::test_predict_tumorbed_seg_and_predict_wsis_with_unet: the fused tile path is the one taken (an engine that
    `is_engine` accepts reads every tile from the device-resident level, forward_f32 is never called), and the class map against the CPU
    chain (spec -> float64 stitch -> threshold): class flips at most 0.002.  With `heat` the heat map too: pixels off by more than 1 LSB
    at most 0.002.  With `near_tie_max` the rule is first shown to apply: at most that share of the spec's own tile pixels are
    near-ties.  Returns the printed figures."""
    import myargs
    import utils.dataset as ds
    import utils.eval as val
    from wsi_segmentation_pipeline_amd import unet
    from wsi_segmentation_pipeline_amd.slide import ArraySlide
    a = myargs.args
    a.scan_level, a.scan_resize, a.num_classes, a.class_probs = 2, 1, 4, [0., 0., 0., 0.]
    a.tile_w = a.tile_h = 64
    a.tile_stride_w = a.tile_stride_h = 48
    a.val_save_pth, a.wsi_mask_pth = str(tmp_path / 'out'), str(tmp_path / 'nomask')
    rng = np.random.default_rng(13)
    l2 = np.clip(np.kron(rng.integers(60, 250, (7, 9, 3)), np.ones((32, 32, 1))) + rng.integers(-25, 25, (224, 288, 3)), 0, 255).astype(np.uint8)
    big = np.repeat(np.repeat(l2, 4, 0), 4, 1)
    slide = ArraySlide([np.repeat(np.repeat(big, 4, 0), 4, 1)[:8, :8], big[:8, :8], l2], [1.0, 4.0, 16.0])   # only level 2 is read
    slide.level_dimensions = ((288 * 16, 224 * 16), (288 * 4, 224 * 4), (288, 224))
    slide.name = 'seg.svs'
    model.load_state_dict(sd)
    model = model.cuda().eval()
    model.classifier, model.regressor = torch.nn.Identity(), torch.nn.Identity()
    calls = {'tiles': 0, 'f32': 0}
    real_tiles, real_f32 = unet.UNetEngine.forward_tiles, unet.UNetEngine.forward_f32

    def forward_tiles(self, *args, **kw):
        assert is_engine(self)
        calls['tiles'] += int(args[1].shape[0])
        return real_tiles(self, *args, **kw)

    def forward_f32(self, *args, **kw):
        calls['f32'] += 1
        return real_f32(self, *args, **kw)
    monkeypatch.setattr(unet.UNetEngine, 'forward_tiles', forward_tiles)
    monkeypatch.setattr(unet.UNetEngine, 'forward_f32', forward_f32)
    params = {'ph': 64, 'pw': 64, 'sh': 48, 'sw': 48}
    dataset = ds.Dataset_wsis({'seg.svs': slide}, params, bs=5)
    tiles = dataset.wsis['seg.svs']['iterator'].dataset.datalist
    mask = dataset.wsis['seg.svs']['mask']
    assert len(tiles) >= 12
    res = val.predict_tumorbed(model, dataset, 1, mode='seg')['seg.svs']
    assert calls == {'tiles': len(tiles), 'f32': 0}
    u8 = np.stack([WO.read_tile(l2, x, y, 64, 64) for x, y in tiles]).transpose(0, 3, 1, 2)
    with torch.no_grad():
        tp = oracle.forward(sd, R.normalize_u8(u8))[0]
    share = near_tie_share(tp)
    pred = WO.stitch_tumorbed(tiles, tp.numpy(), 4, l2.shape[:2], 1.0, 64, 64)
    ref_cls, ref_probs = WO.threshold_probs(pred)
    flips = float((res['classes'] != ref_cls).mean())
    dheat = np.abs(res['heatmap'].astype(int) - WO.tumorbed_heatmap(ref_probs, mask, 'seg').astype(int)) if heat else np.zeros(1, int)
    print('%s predict_tumorbed seg: class flips %.5f of %d pixels, heat pixels off by > 1: %d of %d; near-tie share of the spec tiles %.5f'
          % (type(model).__name__, flips, ref_cls.size, int((dheat > 1).sum()), dheat.size, share))
    if near_tie_max is not None:
        assert share <= near_tie_max
    assert flips <= 0.002 and (dheat > 1).mean() <= 0.002
    return {'flips': flips, 'heat_off': float((dheat > 1).mean()), 'near_tie_share': share}
