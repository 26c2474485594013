"""Every stride-1 3x3 tile configuration the product build dispatches (csrc/conv.hip wsi_slab_dispatch_cfg, csrc/conv_pp.hip
wsi_pp_dispatch), run through wsi_conv3x3_bn_act_cfg and checked against torch fp32 conv + BN on the CPU.

The kernels share one workgroup -> tile map, one dense tile geometry and one slab fetch (csrc/conv_dev.h), so tests that compare two
kernels with each other (test_pingpong_conv_equals_wide_kernel, test_row_stacked_kernel_matches_slab3) cannot see a mistake in the shared
part: this file compares each of them with the oracle, on the smallest shapes that reach each way the shared geometry can go wrong."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# the file-level tolerances of tests/test_gpu_kernels.py, unchanged (relative to the tensor's max magnitude)
TOL_PARITY = 2e-5      # fp16 hi + fp16 lo pair (3 MFMA passes)
TOL_SPEED = 3e-2       # single-pass bf16
TOL_MX = 1e-4          # fp16 main pass + MX-fp6 cross terms (mode 3), single layer
TOL = {1: TOL_SPEED, 2: TOL_PARITY, 3: TOL_MX}
EINVAL = -22

# cfg -> the precision modes (planes) its dispatch line accepts
CFG_PLANES = {30: (1, 2, 3), 31: (1, 2, 3), 38: (3,), 39: (1, 2, 3), 40: (3,), 41: (3,), 60: (1, 2, 3), 70: (1, 2, 3), 71: (1, 2, 3),
              72: (1, 3), 73: (1, 3), 74: (1, 3), 77: (1, 3), 78: (1, 3), 83: (2,), 90: (2, 3), 91: (2, 3)}

SHAPES = [  # n, cin, cout, h, w
    (3, 64, 64, 5, 7), (3, 128, 128, 5, 7),        # ragged last tile; tiles straddle images; W < 32 lane order
    (5, 128, 128, 8, 8),                           # D8 slab image with a last tile of one image instead of four
    (9, 128, 256, 4, 4),                           # tiny maps; mtiles * nblocks is no multiple of 8: the XCD early return runs
    (1, 64, 64, 8, 64), (3, 64, 128, 4, 64),       # 64-wide, H % 4 == 0: row-stacked and paired-tile kernels; the second has nblocks > 1
    (1, 64, 64, 6, 64),                            # H % 4 != 0: the row-stacked kernel declines, cfg 38 runs unpaired
    (1, 64, 64, 3, 130), (2, 32, 32, 5, 40),       # cfg 39 and cfg 90 / 91
    (2, 256, 256, 16, 16),                         # ping-pong with several tiles per image
]

_ran = {}              # shape -> {cfg: conv launches that ran}, filled once per shape


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


def _run_shape(dev, shape):
    """All cfgs x planes x (residual + ReLU, neither) x (default mode, XCD_ORDER) on one shape; returns {cfg: launches that ran}."""
    if shape in _ran:
        return _ran[shape]
    from wsi_segmentation_pipeline_amd import native, engine as E
    lib = native.load()
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(n, cin, h, w, generator=g).abs_()
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    bn = (torch.rand(cout, generator=g) * 0.5 + 0.75, torch.randn(cout, generator=g) * 0.1,
          torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) * 0.5 + 0.75)
    r = torch.randn(n, cout, h, w, generator=g)
    conv = F.batch_norm(F.conv2d(x, wt, None, 1, 1), bn[2], bn[3], bn[0], bn[1], False, 0.0, 1e-5)
    refs = {True: F.relu(conv + r), False: conv}                 # the oracle: computed once per shape
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ran = {cfg: 0 for cfg in CFG_PLANES}
    for planes in (1, 2, 3):
        if lib.wsi_prepack_conv_bytes(cout, cin, 3, planes) == 0:     # (speed mode keeps 64-channel lines)
            continue
        wpk, bias = E.prepack_conv(wt, bn, planes, dev)
        xpf, rpf = E.pf_pack(x.to(dev), planes), E.pf_pack(r.to(dev), planes)
        if planes == 3:          # pad pixels: whole 128-byte lines of pad positions, via the hi plane of an all-ones tensor
            real = E.pf_pack(torch.ones(n, cout, h, w, device=dev), 3).view(-1, 128)[:, :64].ne(0).any(1)
        else:
            real = E.pf_pack(torch.full((n, cout, h, w), 1.0 + 2.0 ** -12, device=dev), planes).view(torch.int16) != 0
        for cfg, accepted in CFG_PLANES.items():
            if planes not in accepted:
                continue
            for mode in (0, native.ConvMode.XCD_ORDER):            # 0: the default mode, in which XCD_RANGES is on
                for full in (True, False):                         # residual + ReLU, or neither
                    opf = E.pf_zeros(n, cout, h, w, planes, dev)
                    with native.conv_mode(mode):
                        rc = lib.wsi_conv3x3_bn_act_cfg(xpf.data_ptr(), opf.data_ptr(), rpf.data_ptr() if full else None, wpk.data_ptr(),
                                                        bias.data_ptr(), n, h, w, cin, cout, 1, int(full), planes, cfg, st)
                    if rc == EINVAL:
                        continue                                   # the cfg does not take this shape
                    assert rc == 0, (shape, cfg, planes, rc)
                    got = E.pf_unpack(opf, n, cout, h, w, planes).cpu()
                    ref = refs[full]
                    err = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6))
                    assert err <= TOL[planes], (shape, cfg, planes, int(mode), full, err)
                    # pad positions of the output buffer must still be zero (the next layer's implicit padding)
                    if planes == 3:
                        assert not bool(opf.view(-1, 128)[~real].ne(0).any()), ('kernel wrote to a pad position', shape, cfg, planes)
                    else:
                        assert not bool((opf.view(torch.int16)[~real] != 0).any()), ('kernel wrote to a pad position', shape, cfg, planes)
                    ran[cfg] += 1
    print('conv routes', shape, 'launches per cfg', ran)
    _ran[shape] = ran
    return ran


@pytest.mark.parametrize('shape', SHAPES)
def test_conv_cfg_matches_cpu_oracle(dev, shape):
    ran = _run_shape(dev, shape)
    assert sum(ran.values()) > 0, 'no cfg takes this shape'


def test_every_cfg_ran_and_few_pairs_skipped(dev):
    """A cfg that returns WSI_EINVAL for a shape is skipped for that shape: every cfg must still have run somewhere, and at most half
    of the (cfg, shape) pairs may have been skipped."""
    ran = {shape: _run_shape(dev, shape) for shape in SHAPES}
    for cfg in CFG_PLANES:
        assert any(ran[shape][cfg] for shape in SHAPES), 'cfg %d ran on no shape' % cfg
    skipped = sum(1 for shape in SHAPES for cfg in CFG_PLANES if not ran[shape][cfg])
    print('skipped (cfg, shape) pairs: %d of %d' % (skipped, len(SHAPES) * len(CFG_PLANES)))
    assert 2 * skipped <= len(SHAPES) * len(CFG_PLANES)
