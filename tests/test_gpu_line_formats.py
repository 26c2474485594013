"""The 128-byte activation line formats, byte for byte: every writer and reader of PF lines that one C-ABI call reaches is held
to the host model oracle/pf_lines_oracle.py (itself checked by tests/test_pf_lines_oracle.py).

(a) wsi_pf_pack writes the model's bytes, (b) wsi_pf_unpack reads what the model reads, (c) the conv epilogues - stride-1 3x3 on
the default route and on the named tile configurations, stride-2 3x3, 1x1, the fused stride-2 block entry, the fused upsample +
concat conv - write the model's bytes, all 128 of every real line (fp16 plane, both fp6 planes, both scale bytes, the zero
dwords) and nothing else, on inputs built so that the expected line needs no tolerance, (d) wsi_avgpool_fc reads every line
format at every channel count and pixel-group split, to a bound derived from fp32 summation alone.

(d') the stem - wsi_stem_conv7x7_bn_relu_maxpool and ..._lines96, 128- and 96-byte lines - is held to the model in
tests/test_gpu_stem_lines.py, which reuses the helpers here.

Out of scope: the 96-byte-line form of layer 1 is not reachable as a single operation through the C ABI; tests/test_gpu_trunk.py
ties it bit for bit to the 128-byte route that (c) pins here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import pf_lines_oracle as O

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from wsi_segmentation_pipeline_amd import native
    return native.load()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    assert rc == 0, '%s returned %d' % (what, rc)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _pf_buffer(lib, n, c, h, w, planes, dev, fill=0):
    nbytes = lib.wsi_pf_bytes(n, h, w, c, planes)
    assert nbytes > 0
    return torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)


def _pack(lib, x, planes, dev, fill=0):
    """x: (n, c, h, w) float32 numpy -> PF buffer on the device through wsi_pf_pack"""
    n, c, h, w = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    buf = _pf_buffer(lib, n, c, h, w, planes, dev, fill)
    _ok(lib.wsi_pf_pack(xd.data_ptr(), buf.data_ptr(), n, c, h, w, planes, _st()), 'wsi_pf_pack')
    torch.cuda.synchronize()
    return buf


def _planes_of(shape):
    return (2, 3) if shape[1] % 64 else (1, 2, 3)


# ------------------------------------------------------------------------------------------------ (a) wsi_pf_pack
PACK_SHAPES = [(3, 32, 5, 7), (2, 96, 3, 9), (3, 64, 5, 7), (2, 128, 4, 33), (1, 512, 2, 2)]


def _pack_input(shape, planes):
    """random normal times a per-line power of two from 2^-20 to 2^14 (values past +-65504 included), the crafted lines among them"""
    n, c, h, w = shape
    rng = np.random.default_rng(sum(shape) + planes)
    nl, cpl = n * h * w * (c // O.CHANNELS[planes]), O.CHANNELS[planes]
    lines = (rng.standard_normal((nl, cpl)) * 2.0 ** rng.integers(-20, 15, (nl, 1))).astype(np.float32)
    crafted = O.crafted_lines(planes)
    assert nl >= crafted.shape[0]
    lines[np.linspace(0, nl - 1, crafted.shape[0]).astype(int)] = crafted
    return O.from_lines(lines.reshape(n * h * w, -1, cpl), n, c, h, w)


@pytest.mark.parametrize('shape', PACK_SHAPES)
def test_pf_pack_writes_the_model_bytes(dev, lib, shape):
    n, c, h, w = shape
    for planes in _planes_of(shape):
        x = _pack_input(shape, planes)
        want = O.encode(O.to_lines(x, planes), planes)
        for fill in (0, 0xA5):
            buf = _host(_pack(lib, x, planes, dev, fill))
            d = O.diff_lines(O.real_lines(buf, n, c, h, w, planes), want)
            assert d is None, 'planes %d fill %#x: %s' % (planes, fill, d)
            assert np.all(O.other_bytes(buf, n, c, h, w, planes) == fill), 'planes %d: a byte outside the real lines was written' % planes


# ------------------------------------------------------------------------------------------------ (b) wsi_pf_unpack
def _random_lines(rng, count, planes):
    b = rng.integers(0, 256, (count, 128), dtype=np.uint8)
    if planes == 1:
        u = b.view(np.uint16)
        u[(u & 0x7f80) == 0x7f80] ^= 0x4000                                        # bf16: finite bit patterns only
        return b
    u = b[:, :64 if planes == 3 else 128].copy().view(np.uint16)
    u[(u & 0x7c00) == 0x7c00] ^= 0x4000                                            # fp16: finite bit patterns only
    b[:, :64 if planes == 3 else 128] = u.view(np.uint8)
    if planes == 3:
        scales = np.r_[0, 1, 100:141, 254].astype(np.uint8)
        b[:, O.SCALE_LO] = rng.choice(scales, count)
        b[:, O.SCALE_HI] = rng.choice(scales, count)
        b[::7, 64] = (b[::7, 64] & 0xC0) | 0x20                                    # the negative-zero code in field 0 of the lo6 plane
    return b


@pytest.mark.parametrize('shape', PACK_SHAPES)
def test_pf_unpack_reads_what_the_model_reads(dev, lib, shape):
    n, c, h, w = shape
    for planes in _planes_of(shape):
        rng = np.random.default_rng(sum(shape) * 3 + planes)
        nl = c // O.CHANNELS[planes]
        lines = _random_lines(rng, n * h * w * nl, planes).reshape(n * h * w, nl, 128)
        buf = np.zeros(lib.wsi_pf_bytes(n, h, w, c, planes), np.uint8)
        O.set_real_lines(buf, lines, n, c, h, w, planes)
        out = torch.full((n, c, h, w), float('nan'), device=dev)
        bd = torch.from_numpy(buf).to(dev)
        _ok(lib.wsi_pf_unpack(bd.data_ptr(), out.data_ptr(), n, c, h, w, planes, _st()), 'wsi_pf_unpack')
        got = _host(out).view(np.uint32)
        want = O.from_lines(O.decode(lines, planes), n, c, h, w).view(np.uint32)
        # float32 bit patterns; +0 and -0 compare equal (hi = -0 with a zero lo part: the sign of a zero sum is not part of the format)
        same = (got == want) | (((got << 1) == 0) & ((want << 1) == 0))
        assert same.all(), 'planes %d: %d values differ, first at %s: got %#x want %#x' % (
            planes, (~same).sum(), np.argwhere(~same)[0].tolist(), got[~same][0], want[~same][0])


# ------------------------------------------------------------------------------------------------ (c) conv epilogues
SCALES = (-14, -6, 0, 5, 12)


def _perm(cout, cin):
    return (7 * np.arange(cout) + 3) % cin                                         # output channel co reads input channel (7 co + 3) % cin


def _perm_weights(cout, cin, k):
    w = np.zeros((cout, cin, k, k), np.float32)
    w[np.arange(cout), _perm(cout, cin), k // 2, k // 2] = 1.0                     # a channel permutation at the centre tap
    return w


@functools.lru_cache(maxsize=None)
def _packed_weights(cout, cin, k, planes):
    from wsi_segmentation_pipeline_amd import engine as E
    wpk, zero_bias = E.prepack_conv(torch.from_numpy(_perm_weights(cout, cin, k)), None, planes, torch.device('cuda:0'))
    assert not bool(zero_bias.ne(0).any())
    return wpk


def _decoded(lib, x, planes, dev):
    """pack x on the device; the PF buffer and what its lines decode to, as (n, c, h, w) float32"""
    n, c, h, w = x.shape
    buf = _pack(lib, x, planes, dev)
    return buf, O.from_lines(O.decode(O.real_lines(_host(buf), n, c, h, w, planes), planes), n, c, h, w)


def _expected_lines(terms, relu, planes):
    """encode(relu?(sum of the float32 terms)): the sum in float64, which must be a float32 exactly (the premise of the test)"""
    s = sum(t.astype(np.float64) for t in terms)
    s32 = s.astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), s) and np.abs(s).max() < O.F16_MAX
    if relu:
        s32 = np.maximum(s32, np.float32(0))
    return O.encode(O.to_lines(s32, planes), planes)


def _compare_output(out, want, n, c, h, w, planes, what):
    """all 128 bytes of every real line, raw (the hardware convert and the scalar codec agree in every bit, the sign bit of an fp6
    zero included, so there is no canonical form to compare in), and not a byte anywhere else"""
    buf = _host(out)
    d = O.diff_lines(O.real_lines(buf, n, c, h, w, planes), want)
    assert d is None, '%s: %s' % (what, d)
    assert not O.other_bytes(buf, n, c, h, w, planes).any(), '%s: a byte outside the real lines was written' % what


class _S1Case:
    """inputs and expected lines of one stride-1 case: (shape, planes, k, with residual + bias + ReLU or without)"""
    def __init__(self, lib, dev, shape, planes, k, full):
        n, cin, cout, h, w = shape
        rng = np.random.default_rng(abs(hash((shape, planes, k, full))) % (1 << 32))
        self.xpf, xd = _decoded(lib, O.grid_values(rng, (n, cin, h, w), k), planes, dev)
        terms = [xd[:, _perm(cout, cin)]]
        self.rpf, bias = None, np.zeros(cout, np.float32)
        if full:
            self.rpf, rd = _decoded(lib, O.grid_values(rng, (n, cout, h, w), k), planes, dev)
            bias = O.grid_values(rng, (cout,), k)
            terms += [rd, np.broadcast_to(bias[None, :, None, None], rd.shape)]
        self.bias = torch.from_numpy(bias).to(dev)
        self.relu = int(full)
        self.want = _expected_lines(terms, full, planes)
        self.wpk = _packed_weights(cout, cin, 3, planes)


S1_SHAPES = [(2, 64, 64, 16, 16), (1, 64, 64, 5, 130), (1, 64, 64, 4, 64), (3, 256, 256, 4, 4), (2, 512, 512, 2, 2),
             (5, 128, 128, 32, 32), (2, 32, 32, 9, 40)]
S1_CFGS = (30, 38, 39, 40, 60, 70, 90)


@pytest.mark.parametrize('shape', S1_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_conv3x3_stride1_writes_the_model_bytes(dev, lib, shape):
    """wsi_conv3x3_bn_act (the default route, which may not decline) and wsi_conv3x3_bn_act_cfg on every named configuration
    (-22: the configuration does not serve this shape / mode).  cfg 40 sums in another order than cfg 38; here every sum is exact,
    so it owes the same bytes."""
    n, cin, cout, h, w = shape
    scales = (0,) if shape == (5, 128, 128, 32, 32) else SCALES
    ran, declined = {}, {}
    for planes in _planes_of(shape):
        for k in scales:
            for full in ((False,) if cin == 32 else (False, True)):
                c = _S1Case(lib, dev, shape, planes, k, full)
                rp = c.rpf.data_ptr() if c.rpf is not None else None
                for cfg in (-1,) + S1_CFGS:
                    out = _pf_buffer(lib, n, cout, h, w, planes, dev)
                    if cfg < 0:
                        rc = lib.wsi_conv3x3_bn_act(c.xpf.data_ptr(), out.data_ptr(), rp, c.wpk.data_ptr(), c.bias.data_ptr(), n, h, w, cin, cout,
                                                    1, c.relu, planes, _st())
                        _ok(rc, 'wsi_conv3x3_bn_act')
                    else:
                        rc = lib.wsi_conv3x3_bn_act_cfg(c.xpf.data_ptr(), out.data_ptr(), rp, c.wpk.data_ptr(), c.bias.data_ptr(), n, h, w, cin,
                                                        cout, 1, c.relu, planes, cfg, _st())
                        if rc == EINVAL:
                            declined.setdefault(cfg, set()).add(planes)
                            continue
                        _ok(rc, 'cfg %d' % cfg)
                    _compare_output(out, c.want, n, cout, h, w, planes, 'cfg %d planes %d k %d full %d' % (cfg, planes, k, full))
                    ran.setdefault(cfg, set()).add(planes)
    print('line formats, stride-1 %s: ran {cfg: planes} %s; -22 %s' % (
        shape, {k: sorted(v) for k, v in ran.items()}, {k: sorted(v) for k, v in declined.items()}))
    assert set(ran[-1]) == set(_planes_of(shape))


S2_SHAPES = [(3, 64, 128, 16, 16), (2, 256, 512, 4, 4)]


@pytest.mark.parametrize('shape', S2_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_stride2_convs_write_the_model_bytes(dev, lib, shape):
    """stride 2: the centre tap of the 3x3 conv and the 1x1 conv both give x[:, :, ::2, ::2]; wsi_conv3x3_bn_act, wsi_conv1x1_bn and
    both outputs of wsi_conv3x3s2_ds_fused.  Mode 3 has no stand-alone 1x1 kernel (its downsample runs inside other kernels) and no
    residual tail on its stride-2 kernels: both are refused with -22, not computed wrongly."""
    n, cin, cout, h, w = shape
    ho, wo = h // 2, w // 2
    src = _perm(cout, cin)
    for planes in (2, 3):
        w3, w1 = _packed_weights(cout, cin, 3, planes), _packed_weights(cout, cin, 1, planes)
        for k in SCALES:
            rng = np.random.default_rng(abs(hash((shape, planes, k))) % (1 << 32))
            xpf, xd = _decoded(lib, O.grid_values(rng, (n, cin, h, w), k), planes, dev)
            xs = xd[:, src, ::2, ::2]
            rpf, rd = _decoded(lib, O.grid_values(rng, (n, cout, ho, wo), k), planes, dev)
            b3n, b1n = O.grid_values(rng, (cout,), k), O.grid_values(rng, (cout,), k)
            zero = torch.zeros(cout, device=dev)
            b3, b1 = torch.from_numpy(b3n).to(dev), torch.from_numpy(b1n).to(dev)
            bc = lambda b: np.broadcast_to(b[None, :, None, None], xs.shape)
            new = lambda: _pf_buffer(lib, n, cout, ho, wo, planes, dev)
            tag = 'planes %d k %d' % (planes, k)
            # 3x3 stride 2: no residual, no ReLU / bias + ReLU (+ residual where the mode has one)
            out = new()
            _ok(lib.wsi_conv3x3_bn_act(xpf.data_ptr(), out.data_ptr(), None, w3.data_ptr(), zero.data_ptr(), n, h, w, cin, cout, 2, 0, planes, _st()), '3x3 s2')
            _compare_output(out, _expected_lines([xs], False, planes), n, cout, ho, wo, planes, '3x3 s2 plain ' + tag)
            out = new()
            rc = lib.wsi_conv3x3_bn_act(xpf.data_ptr(), out.data_ptr(), rpf.data_ptr(), w3.data_ptr(), b3.data_ptr(), n, h, w, cin, cout, 2, 1, planes, _st())
            if planes == 3:
                assert rc == EINVAL
                _ok(lib.wsi_conv3x3_bn_act(xpf.data_ptr(), out.data_ptr(), None, w3.data_ptr(), b3.data_ptr(), n, h, w, cin, cout, 2, 1, planes, _st()), '3x3 s2')
                _compare_output(out, _expected_lines([xs, bc(b3n)], True, planes), n, cout, ho, wo, planes, '3x3 s2 bias relu ' + tag)
            else:
                _ok(rc, '3x3 s2 resid')
                _compare_output(out, _expected_lines([xs, bc(b3n), rd], True, planes), n, cout, ho, wo, planes, '3x3 s2 full ' + tag)
            # 1x1 stride 2 (the entry has neither residual nor ReLU)
            for bt, bn in ((zero, np.zeros(cout, np.float32)), (b1, b1n)):
                out = new()
                rc = lib.wsi_conv1x1_bn(xpf.data_ptr(), out.data_ptr(), w1.data_ptr(), bt.data_ptr(), n, h, w, cin, cout, 2, planes, _st())
                if planes == 3 and rc == EINVAL:
                    continue                                                          # no mode-3 1x1 kernel behind this entry (see ds_fused below)
                _ok(rc, '1x1 s2')
                _compare_output(out, _expected_lines([xs, bc(bn)], False, planes), n, cout, ho, wo, planes, '1x1 s2 ' + tag)
            # the fused block entry: relu(conv3x3 s2 + b3) and conv1x1 s2 + b1 in one launch
            o3, o1 = new(), new()
            _ok(lib.wsi_conv3x3s2_ds_fused(xpf.data_ptr(), o3.data_ptr(), o1.data_ptr(), w3.data_ptr(), b3.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                                           n, h, w, cin, cout, planes, _st()), 'ds_fused')
            _compare_output(o3, _expected_lines([xs, bc(b3n)], True, planes), n, cout, ho, wo, planes, 'ds_fused conv ' + tag)
            _compare_output(o1, _expected_lines([xs, bc(b1n)], False, planes), n, cout, ho, wo, planes, 'ds_fused downsample ' + tag)


def test_upsample_concat_conv_writes_the_model_bytes(dev, lib):
    """wsi_conv3x3_up_concat_bn_act: cat(nearest x2 upsample of `up`, `skip`) through a centre-tap permutation over the concatenated
    channels; shape (n, c_up, c_skip, cout, h, w) as in tests/test_gpu_unet.py."""
    n, cu, cs, co, h, w = 2, 32, 32, 32, 8, 12
    src = _perm(co, cu + cs)
    for planes in (2, 3):
        wpk = _packed_weights(co, cu + cs, 3, planes)
        for k in SCALES:
            rng = np.random.default_rng(1000 + 10 * k + planes)
            upf, ud = _decoded(lib, O.grid_values(rng, (n, cu, h // 2, w // 2), k), planes, dev)
            spf, sd = _decoded(lib, O.grid_values(rng, (n, cs, h, w), k), planes, dev)
            cat = np.concatenate([ud.repeat(2, axis=2).repeat(2, axis=3), sd], 1)[:, src]
            bn = O.grid_values(rng, (co,), k)
            for relu, b in ((0, np.zeros(co, np.float32)), (1, bn)):
                out = _pf_buffer(lib, n, co, h, w, planes, dev)
                bt = torch.from_numpy(b).to(dev)
                _ok(lib.wsi_conv3x3_up_concat_bn_act(upf.data_ptr(), spf.data_ptr(), out.data_ptr(), wpk.data_ptr(), bt.data_ptr(), n, h, w, cu, cs, co,
                                                     relu, planes, _st()), 'up_concat')
                want = _expected_lines([cat, np.broadcast_to(b[None, :, None, None], cat.shape)], bool(relu), planes)
                _compare_output(out, want, n, co, h, w, planes, 'up_concat planes %d k %d relu %d' % (planes, k, relu))


# ------------------------------------------------------------------------------------------------ (d) wsi_avgpool_fc
POOL_C = [(3, 32), (3, 64), (3, 96), (3, 512), (3, 2048), (2, 32), (2, 64), (2, 512), (1, 64), (1, 512)]
U = 2.0 ** -24                                                                        # fp32 unit roundoff


def _pool_bounds(xd, n, c, hw, wt, b):
    """float64 reference of features and logits from the decoded lines, and the fp32-summation bounds: |feat - ref| <= HW u mean|x|
    per channel, |logit - ref| <= (C + HW) u sum|f w|"""
    v = xd.reshape(n, c, hw).astype(np.float64)
    feat = v.mean(2)
    fb = hw * U * np.abs(v).mean(2)
    logit = feat @ wt.astype(np.float64).T + b.astype(np.float64)
    lb = (c + hw) * U * (np.abs(feat)[:, None, :] * np.abs(wt.astype(np.float64))[None]).sum(2)
    return feat, fb, logit, lb


@pytest.mark.parametrize('planes,c', POOL_C)
def test_avgpool_fc_reads_every_line_format(dev, lib, planes, c):
    maps = [(2, 2)] if c == 2048 else [(1, 1), (2, 2), (3, 5), (8, 8), (16, 16)]
    rng = np.random.default_rng(100 * planes + c)
    for h, w in maps:
        for n in (1, 5):
            x = (rng.standard_normal((n, c, h, w)) * 3.0).astype(np.float32)
            buf = _pack(lib, x, planes, dev)
            lines = O.real_lines(_host(buf), n, c, h, w, planes)
            xd = O.from_lines(O.decode(lines, planes), n, c, h, w)
            if planes != 1:
                # the check bites: the same lines without their lo plane miss the bound against the full reference (host only)
                cut = lines.copy()
                cut[..., 64:] = 0
                feat, fb, _, _ = _pool_bounds(xd, n, c, h * w, np.zeros((1, c), np.float32), np.zeros(1, np.float32))
                fcut = O.from_lines(O.decode(cut, planes), n, c, h, w).reshape(n, c, h * w).astype(np.float64).mean(2)
                assert np.any(np.abs(fcut - feat) > fb)
            for K in (1, 4, 7):
                wt = (rng.standard_normal((K, c)) * 0.05).astype(np.float32)
                b = (rng.standard_normal(K) * 0.1).astype(np.float32)
                feat, fb, logit, lb = _pool_bounds(xd, n, c, h * w, wt, b)
                wd, bd = torch.from_numpy(wt).to(dev), torch.from_numpy(b).to(dev)
                for want_feat, want_logit in ((True, True), (False, True), (True, False)) if K == 4 else ((True, True),):
                    fo = torch.full((n, c), float('nan'), device=dev)
                    lo = torch.full((n, K), float('nan'), device=dev)
                    _ok(lib.wsi_avgpool_fc(buf.data_ptr(), n, h, w, c, wd.data_ptr(), bd.data_ptr(), K, fo.data_ptr() if want_feat else None,
                                           lo.data_ptr() if want_logit else None, planes, _st()), 'wsi_avgpool_fc')
                    fg, lg = _host(fo).astype(np.float64), _host(lo).astype(np.float64)
                    tag = 'planes %d c %d map %dx%d n %d K %d' % (planes, c, h, w, n, K)
                    if want_feat:
                        worst = float((np.abs(fg - feat) / np.maximum(fb, 1e-300)).max())
                        assert np.all(np.abs(fg - feat) <= fb), '%s: feature error %.3g of its bound' % (tag, worst)
                    else:
                        assert np.isnan(fg).all()
                    if want_logit:
                        worst = float((np.abs(lg - logit) / lb).max())
                        assert np.all(np.abs(lg - logit) <= lb), '%s: logit error %.3g of its bound' % (tag, worst)
                    else:
                        assert np.isnan(lg).all()


def test_avgpool_fc_argument_errors(dev, lib):
    """Channel counts that are no whole number of 128-byte lines (tensors wsi_pf_pack itself refuses), more than 2048 channels in
    mode 3 and planes outside 1..3 return -22 without a launch: the outputs stay untouched."""
    buf = torch.zeros(1 << 25, dtype=torch.uint8, device=dev)                             # (room for every shape below, were one to run)
    wt, b = torch.zeros(4 * 4096, device=dev), torch.zeros(4, device=dev)
    fo, lo = torch.full((4096,), float('nan'), device=dev), torch.full((4,), float('nan'), device=dev)
    for planes, c in ((2, 36), (3, 36), (2, 48), (3, 16), (1, 32), (1, 96), (1, 36), (3, 2080), (3, 4096), (0, 64), (4, 64), (-1, 64), (2, 0)):
        rc = lib.wsi_avgpool_fc(buf.data_ptr(), 1, 2, 2, c, wt.data_ptr(), b.data_ptr(), 4, fo.data_ptr(), lo.data_ptr(), planes, _st())
        assert rc == EINVAL, (planes, c, rc)
    assert lib.wsi_avgpool_fc(None, 1, 2, 2, 64, wt.data_ptr(), b.data_ptr(), 4, fo.data_ptr(), lo.data_ptr(), 2, _st()) == EINVAL
    assert lib.wsi_avgpool_fc(buf.data_ptr(), 1, 2, 2, 64, None, b.data_ptr(), 4, fo.data_ptr(), lo.data_ptr(), 2, _st()) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(fo).all()) and bool(torch.isnan(lo).all())
    # what wsi_pf_pack refuses, for comparison
    x = torch.zeros(1, 36, 2, 2, device=dev)
    assert lib.wsi_pf_pack(x.data_ptr(), buf.data_ptr(), 1, 36, 2, 2, 2, _st()) == EINVAL
