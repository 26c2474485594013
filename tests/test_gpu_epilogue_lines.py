"""The two store shapes of the mode-3 conv epilogue write the same bytes: 64-byte sectors per lane quad (the default,
conv_dev.h mx_store_sectors) against the four 16-byte pieces of a lane's own pixel (WSI_CONV_MODE_EPILOGUE_PIECES).

Every case runs one conv (or the trunk) under both routes into zero-filled buffers and asserts that the WHOLE allocations agree
byte for byte, pads included, and - where the layout of the allocation is an ordinary or phase-split PF tensor - that no byte
outside the real lines was written.  The sector route ships on the row-stacked layer-1 kernel (the other kernels keep the piece
shape under both modes, so their cases pin that the route bit changes nothing there).

The 96-byte-line forms of the row-stacked kernel (96-byte input, output and residual; the stage's last conv, which reads 96-byte
lines and writes the phase-split 128-byte form) and the folded downsample segment of the wide kernel are not reachable as single
operations through the C ABI: the trunk cases cover them by comparing the whole workspace - every layer's tensor, its pads, the
phase-split hand-overs - after a forward under each route.  The workspace's pads are pinned to zero by tests/test_gpu_trunk.py
on the piece route's layout; equality of the whole allocation carries that over."""
import numpy as np
import pytest
import torch

from oracle import pf_lines_oracle as O
from tests.test_gpu_line_formats import _host, _ok, _pack, _pf_buffer, _st, dev, lib       # noqa: F401 (dev, lib: fixtures)
from wsi_segmentation_pipeline_amd import native

pytestmark = pytest.mark.gpu
PLANES = 3
ROUTES = (native.ConvMode.EPILOGUE_PIECES, 0)                                     # the piece shape first, then the default


def _weights(cout, cin, k, seed, dev):
    from wsi_segmentation_pipeline_amd import engine as E
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((cout, cin, k, k), generator=g) * (1.5 / np.sqrt(cin * k * k))
    wpk, _ = E.prepack_conv(w, None, PLANES, dev)
    return wpk, (torch.randn(cout, generator=g) * 0.5).to(dev)


def _input(lib, dev, shape, seed):
    rng = np.random.default_rng(seed)
    return _pack(lib, (rng.standard_normal(shape) * 2.0).astype(np.float32), PLANES, dev)


def _both_routes(run):
    """run() -> list of device byte tensors; under each route, from fresh zero-filled outputs"""
    got = []
    for flags in ROUTES:
        with native.conv_mode(flags):
            got.append([_host(t) for t in run()])
    for a, b in zip(*got):
        assert a.any(), 'nothing was written'
        assert np.array_equal(a, b), 'the routes differ in %d bytes, first at %d' % ((a != b).sum(), np.argmax(a != b))
    return got[1]


def _pads_zero(buf, n, c, h, w, phases=1):
    for img in buf.reshape(phases, -1):
        assert not O.other_bytes(img, n, c, h, w, PLANES).any(), 'a byte outside the real lines was written'


S1_CASES = [  # (n, channels, h, w): row-stacked kernel; wide kernel, tiles inside an image; wide kernel, tiles span images and the last one
              # is partial; slab3 non-dense route on an odd map (pads filtered inside the tile)
    (2, 64, 64, 64), (3, 128, 32, 32), (5, 512, 8, 8), (2, 64, 24, 40)]


@pytest.mark.parametrize('shape', S1_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_stride1_convs_store_the_same_bytes(dev, lib, shape):
    n, c, h, w = shape
    x, r = _input(lib, dev, (n, c, h, w), 1), _input(lib, dev, (n, c, h, w), 2)
    wpk, bias = _weights(c, c, 3, 3, dev)
    for resid in (None, r):
        def run():
            out = _pf_buffer(lib, n, c, h, w, PLANES, dev)
            _ok(lib.wsi_conv3x3_bn_act(x.data_ptr(), out.data_ptr(), resid.data_ptr() if resid is not None else None, wpk.data_ptr(),
                                       bias.data_ptr(), n, h, w, c, c, 1, 1, PLANES, _st()), 'wsi_conv3x3_bn_act')
            return [out]
        _pads_zero(_both_routes(run)[0], n, c, h, w)
    if h % 2 or w % 2 or c > 128:
        return
    for resid in (None, r):                                                       # phase-split output (the stage's last conv writes this form)
        def run_split():
            out = torch.zeros(lib.wsi_pf_split_bytes(n, h, w, c, PLANES), dtype=torch.uint8, device=dev)
            _ok(lib.wsi_conv3x3_bn_act_split(x.data_ptr(), out.data_ptr(), resid.data_ptr() if resid is not None else None, wpk.data_ptr(),
                                             bias.data_ptr(), n, h, w, c, c, 1, PLANES, _st()), 'wsi_conv3x3_bn_act_split')
            return [out]
        _pads_zero(_both_routes(run_split)[0], n, c, h // 2, w // 2, phases=4)


def test_stride2_split_entry_stores_the_same_bytes(dev, lib):
    """n = 3, 64 -> 128 channels from a phase-split 64 x 64 input: both outputs of the wide stride-2 kernel"""
    n, cin, cout, h, w = 3, 64, 128, 64, 64
    x = _input(lib, dev, (n, cin, h, w), 4)
    w0, b0 = _weights(cin, cin, 3, 5, dev)
    xs = torch.zeros(lib.wsi_pf_split_bytes(n, h, w, cin, PLANES), dtype=torch.uint8, device=dev)
    _ok(lib.wsi_conv3x3_bn_act_split(x.data_ptr(), xs.data_ptr(), None, w0.data_ptr(), b0.data_ptr(), n, h, w, cin, cin, 1, PLANES, _st()), 'split input')
    w3, b3 = _weights(cout, cin, 3, 6, dev)
    w1, b1 = _weights(cout, cin, 1, 7, dev)

    def run():
        o3, o1 = (_pf_buffer(lib, n, cout, h // 2, w // 2, PLANES, dev) for _ in range(2))
        _ok(lib.wsi_conv3x3s2_ds_fused_split(xs.data_ptr(), o3.data_ptr(), o1.data_ptr(), w3.data_ptr(), b3.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                                             n, h, w, cin, cout, PLANES, _st()), 'wsi_conv3x3s2_ds_fused_split')
        return [o3, o1]
    for buf in _both_routes(run):
        _pads_zero(buf, n, cout, h // 2, w // 2)


@pytest.mark.parametrize('n', [2, 3])
def test_trunk_workspace_and_logits_equal_between_the_routes(dev, n):
    """256 x 256 patches: layer 1 runs the row-stacked kernel on 96-byte lines (plain, 96-byte residual, the last conv's phase-split
    128-byte output), layers 2-4 the stride-2 split entries and the wide kernel with the folded downsample segment; the whole
    workspace, the features and the logits agree."""
    from wsi_segmentation_pipeline_amd import engine as E, synthetic as W
    from wsi_segmentation_pipeline_amd.engine import TrunkEngine
    sd = W.make_resnet18_state_dict(11, with_fc=False)
    cls = W.make_head_state_dict(22, 'classifier')
    eng = TrunkEngine(sd, dev, planes=PLANES, head=(cls['fc.0.weight'], cls['fc.0.bias']), max_batch=n)
    x = torch.randn((n, 3, 256, 256), device=dev, generator=torch.Generator(device=dev).manual_seed(n))
    got = []
    for flags in ROUTES:
        with native.conv_mode(flags):
            eng.release_workspaces()                                               # a fresh plan per route, initialised from all-zero
            ws, cap = eng._workspace(n, 256, 256)                                  # bytes: the allocator hands back stale memory, and
            ws.zero_()                                                             # no kernel writes e.g. the unfused stem's scratch
            native.check(eng._ws_init(E._ptr(ws), cap, 256, 256, PLANES, E._stream()), 'workspace init')
            feat, logits, _ = eng.forward_f32(x, feat=True, logits=True)
            assert eng._workspace(n, 256, 256)[0] is ws
            got.append((_host(ws), _host(feat), _host(logits)))
    for a, b, what in zip(got[0], got[1], ('workspace', 'features', 'logits')):
        assert a.any() and np.array_equal(a, b), '%s: the routes differ in %d places' % (what, (a != b).sum())
