"""GPU tests of the pointwise-conv kernel (csrc/conv_pw.hip) through wsi_conv1x1_bn_act: the 1x1 convs of a Bottleneck block
(reference resnets_shift.py:68-108) against torch.nn.functional.conv2d in float64 on the CPU with folded BN, the gather kernel as
A/B (ConvMode.PW_GATHER: both kernels add the K lines in the same order, so the results are equal to the bit), pad positions, the
fp16 clamp, the planes-3 refusal, and the stride-2 conv2 route of the Bottleneck trunk.

Bounds: the project's own single-conv bounds (tests/test_gpu_kernels.py) relative to the output's maximum."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL_PARITY = 2e-5      # planes 2: fp16 hi + fp16 lo pair
TOL_SPEED = 3e-2       # planes 1: single-pass bf16
TOL = {2: TOL_PARITY, 1: TOL_SPEED}

# (64, 64) and (256, 64): 64-channel outputs, which the dispatch sends to the gather kernel (the A/B is then trivial); (256, 128) and
# (512, 128): the 128 x 128 tile class; the others: the 64 x 256 and 64 x 512 classes, (512, 2048) with its lines resident in LDS
CHANNELS = [(64, 64), (64, 256), (256, 64), (512, 2048), (2048, 512), (1024, 256), (256, 128), (512, 128)]
# several passes over cout with more input lines than the LDS holds (planes 2: 1024 channels x 64 pixels x 4 B = 256 KiB): every pass
# streams the lines again through the ring
STREAMED = [(1024, 2048), (2048, 1024)]
MAPS = [(5, 2, 2), (3, 8, 8), (2, 16, 9)]        # n, h, w: several images inside one pixel tile; whole tiles; an odd width


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


_packs = {}


def _weights(cin, cout, planes, dev):
    """Seeded conv weight + BN of one (cin, cout), its float64 folded form and the device pack of `planes` (made once)."""
    from wsi_segmentation_pipeline_amd import engine as E
    key = (cin, cout)
    if key not in _packs:
        g = torch.Generator().manual_seed(1000 + cin + 7 * cout)
        wt = torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5
        bn = (torch.rand(cout, generator=g) * 0.5 + 0.75, torch.randn(cout, generator=g) * 0.1,
              torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) * 0.5 + 0.75)
        _packs[key] = {'w': wt, 'bn': bn}
    ent = _packs[key]
    if planes not in ent:
        ent[planes] = E.prepack_conv(ent['w'], ent['bn'], planes, dev)
    return ent['w'], ent['bn'], ent[planes]


def _reference(x, wt, bn, resid, relu):
    ref = F.conv2d(x.double(), wt.double())
    ref = F.batch_norm(ref, bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(), False, 0.0, 1e-5)
    if resid is not None:
        ref = ref + resid.double()
    return F.relu(ref) if relu else ref


def _pad_rows_zero(buf, n, c, h, w, planes):
    """Every pad / guard position of a raw PF buffer is still zero (real pixels located with wsi_pf_pixel_index)."""
    from wsi_segmentation_pipeline_amd import native
    lib = native.load()
    rows = buf.view(-1, c * (2 if planes == 1 else 4))
    real = torch.zeros(rows.shape[0], dtype=torch.bool)
    first = np.array([[lib.wsi_pf_pixel_index(i, y, 0, h, w) for y in range(h)] for i in range(n)]).reshape(-1)
    idx = (first[:, None] + np.arange(w)[None, :]).reshape(-1)
    real[torch.from_numpy(idx)] = True
    return not bool(rows.cpu()[~real].ne(0).any())


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-6))


@pytest.mark.parametrize('maps', MAPS, ids=lambda m: 'n%d_%dx%d' % m)
@pytest.mark.parametrize('chans', CHANNELS, ids=lambda c: '%dto%d' % c)
def test_pointwise_conv_against_float64(dev, chans, maps):
    from wsi_segmentation_pipeline_amd import engine as E, native
    (cin, cout), (n, h, w) = chans, maps
    g = torch.Generator().manual_seed(cin * 31 + cout + h)
    x = torch.randn(n, cin, h, w, generator=g).abs_()
    r = torch.randn(n, cout, h, w, generator=g)
    for planes in (2, 1):
        wt, bn, (wpk, bias) = _weights(cin, cout, planes, dev)
        xpf, rpf = E.pf_pack(x.to(dev), planes), E.pf_pack(r.to(dev), planes)
        for resid in (True, False):
            for relu in (True, False):
                ref = _reference(x, wt, bn, r if resid else None, relu)
                opf = E.conv1x1_bn_act(xpf, n, h, w, cin, cout, wpk, bias, 1, rpf if resid else None, relu, planes)
                got = E.pf_unpack(opf, n, cout, h, w, planes).cpu()
                with native.conv_mode(native.ConvMode.PW_GATHER):
                    gpf = E.conv1x1_bn_act(xpf, n, h, w, cin, cout, wpk, bias, 1, rpf if resid else None, relu, planes)
                gat = E.pf_unpack(gpf, n, cout, h, w, planes).cpu()
                err, ab = _rel(got, ref), _rel(got, gat.double())
                print('pointwise %s %s planes %d resid %d relu %d: err %.2e, vs gather %.2e' % (chans, maps, planes, resid, relu, err, ab))
                assert err <= TOL[planes]
                assert ab <= 2 * TOL[planes] and torch.equal(got, gat)     # the same lines in the same order: equal to the bit
                assert _pad_rows_zero(opf, n, cout, h, w, planes), 'the pointwise kernel wrote to a pad position'


@pytest.mark.parametrize('maps', [MAPS[0], MAPS[2]], ids=lambda m: 'n%d_%dx%d' % m)
@pytest.mark.parametrize('chans', STREAMED, ids=lambda c: '%dto%d' % c)
def test_pointwise_streamed_passes(dev, chans, maps):
    """cout > 512 with an input too wide to stay in LDS: the ring is handed over between passes and every pass fetches its lines again."""
    from wsi_segmentation_pipeline_amd import engine as E, native
    (cin, cout), (n, h, w) = chans, maps
    g = torch.Generator().manual_seed(cin + 3 * cout + w)
    x = torch.randn(n, cin, h, w, generator=g).abs_()
    r = torch.randn(n, cout, h, w, generator=g)
    wt, bn, (wpk, bias) = _weights(cin, cout, 2, dev)
    xpf, rpf = E.pf_pack(x.to(dev), 2), E.pf_pack(r.to(dev), 2)
    for resid in (True, False):
        ref = _reference(x, wt, bn, r if resid else None, True)
        opf = E.conv1x1_bn_act(xpf, n, h, w, cin, cout, wpk, bias, 1, rpf if resid else None, True, 2)
        got = E.pf_unpack(opf, n, cout, h, w, 2).cpu()
        with native.conv_mode(native.ConvMode.PW_GATHER):
            gat = E.pf_unpack(E.conv1x1_bn_act(xpf, n, h, w, cin, cout, wpk, bias, 1, rpf if resid else None, True, 2), n, cout, h, w, 2).cpu()
        err = _rel(got, ref)
        print('streamed passes %s %s resid %d: err %.2e, equal to gather %s' % (chans, maps, resid, err, torch.equal(got, gat)))
        assert err <= TOL_PARITY and torch.equal(got, gat)
        assert _pad_rows_zero(opf, n, cout, h, w, 2), 'the pointwise kernel wrote to a pad position'


def test_pointwise_clamps_to_fp16_range(dev):
    """Outputs beyond +-65504 saturate as those of the 3x3 convs do (tests/test_gpu_kernels.py test_mx_clamp_to_fp16_range), on a shape
    the pointwise kernel takes (64 -> 128), without and with a residual that pushes further out and back inside."""
    from wsi_segmentation_pipeline_amd import engine as E
    n, ci, c, h, w = 2, 64, 128, 8, 8
    g = torch.Generator().manual_seed(5)
    x = torch.rand(n, ci, h, w, generator=g) * 400.0
    r = (torch.rand(n, c, h, w, generator=g) - 0.5) * 60000.0
    wt = torch.zeros(c, ci, 1, 1)
    for co in range(c):
        wt[co, (co * 7 + 3) % ci, 0, 0] = 300.0 if co % 2 == 0 else -300.0
    wpk, bias = E.prepack_conv(wt, None, 2, dev)
    xpf, rpf = E.pf_pack(x.to(dev), 2), E.pf_pack(r.to(dev), 2)
    for resid in (None, r):
        ref = F.conv2d(x.double(), wt.double()) + (0 if resid is None else E.pf_unpack(rpf, n, c, h, w, 2).cpu().double())
        assert float(ref.abs().max()) > 100000
        out = E.pf_unpack(E.conv1x1_bn_act(xpf, n, h, w, ci, c, wpk, bias, 1, None if resid is None else rpf, False, 2), n, c, h, w, 2).cpu()
        assert float(out.max()) == 65504.0 and float(out.min()) == -65504.0
        assert float((out.double() - ref.clamp(-65504.0, 65504.0)).abs().max() / 65504.0) <= TOL_PARITY


def test_pointwise_refuses_planes_3(dev):
    from wsi_segmentation_pipeline_amd import engine as E, native
    n, c, h, w = 1, 64, 4, 4
    wpk, bias = E.prepack_conv(torch.zeros(c, c, 1, 1), None, 2, dev)
    xpf = E.pf_zeros(n, c, h, w, 3, dev)
    for mode in (0, native.ConvMode.PW_GATHER):
        with native.conv_mode(mode):
            assert E.conv1x1_bn_act(xpf, n, h, w, c, c, wpk, bias, 1, None, True, 3, check=False)[1] == -22


@pytest.mark.parametrize('c', [128, 512])
def test_bottleneck_stride2_conv2_route(dev, c):
    """conv2 of a strided Bottleneck block: 3x3, stride 2, cin == cout, through the call the Bottleneck trunk makes (the stride-2 slab
    route of wsi_conv3x3_bn_act), in both modes the trunk runs."""
    from wsi_segmentation_pipeline_amd import engine as E
    n, h, w = 3, 8, 8
    g = torch.Generator().manual_seed(c)
    x = torch.randn(n, c, h, w, generator=g).abs_()
    wt = torch.randn(c, c, 3, 3, generator=g) * (2.0 / (c * 9)) ** 0.5
    bn = (torch.rand(c, generator=g) * 0.5 + 0.75, torch.randn(c, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1,
          torch.rand(c, generator=g) * 0.5 + 0.75)
    ref = F.conv2d(x.double(), wt.double(), None, 2, 1)
    ref = F.relu(F.batch_norm(ref, bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(), False, 0.0, 1e-5))
    for planes in (2, 1):
        wpk, bias = E.prepack_conv(wt, bn, planes, dev)
        opf = E.conv_bn_act(E.pf_pack(x.to(dev), planes), n, h, w, c, c, wpk, bias, 2, 3, None, True, planes)
        err = _rel(E.pf_unpack(opf, n, c, h // 2, w // 2, planes).cpu(), ref)
        print('stride-2 conv2 %d channels planes %d: err %.2e' % (c, planes, err))
        assert err <= TOL[planes]
        assert _pad_rows_zero(opf, n, c, h // 2, w // 2, planes)
