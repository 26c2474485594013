"""CPU-only: the C-ABI library builds/loads and exports every symbol include/wsi_hip.h declares;
host-side entry points (no GPU needed) behave."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from wsi_segmentation_pipeline_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


def test_header_symbols_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(wsi_[a-z0-9_]+)\s*\(', hdr))
    assert len(declared) >= 20
    assert declared == set(native.SIGNATURES), declared ^ set(native.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert int(re.search(r'#define WSI_HIP_ABI_VERSION (\d+)', hdr).group(1)) == native.ABI_VERSION == lib.wsi_hip_abi_version()


def test_mode_names_match_header():
    """native.ConvMode / StemMode mirror the WSI_CONV_MODE_* / WSI_STEM_MODE_* enumerators of the header, name for name and value for
    value; apart from the 0 / 1 / 3 base values every conv mode constant is one bit of its own."""
    hdr = open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for prefix, enum_cls in (('WSI_CONV_MODE_', native.ConvMode), ('WSI_STEM_MODE_', native.StemMode)):
        in_header = {m.group(1): int(m.group(2)) for m in re.finditer(prefix + r'(\w+)\s*=\s*(\d+)', hdr)}
        assert in_header == {name: int(m) for name, m in enum_cls.__members__.items()}, prefix
    M = native.ConvMode
    assert (int(M.S2_GATHER), int(M.S2_SLAB), int(M.S2_SLAB_128)) == (0, 1, 3)
    bits = [int(m) for name, m in M.__members__.items() if name not in ('S2_GATHER', 'S2_SLAB', 'S2_SLAB_128')]
    assert len(bits) >= 18 and all(b > 7 and b & (b - 1) == 0 for b in bits) and len(set(bits)) == len(bits)


def test_pf_layout_helpers(lib):
    # pixel (n,y,x) -> (W+2) + n*(H+1)*(W+1) + y*(W+1) + x
    assert lib.wsi_pf_pixel_index(0, 0, 0, 8, 8) == 10
    assert lib.wsi_pf_pixel_index(2, 3, 4, 8, 8) == 10 + 2 * 81 + 3 * 9 + 4
    nbytes = lib.wsi_pf_bytes(3, 8, 8, 512, 2)
    assert nbytes % (512 * 2 * 2) == 0
    assert nbytes // (512 * 4) >= 2 * 10 + 3 * 81
    assert lib.wsi_pf_bytes(0, 8, 8, 512, 2) == 0
    assert lib.wsi_trunk_workspace_bytes(4, 256, 256, 2) > 4 * 4 * 1024 * 1024
    assert lib.wsi_trunk_workspace_bytes(4, 250, 256, 2) == 0           # not a multiple of 32


def test_normalize_lut_matches_transform(lib):
    from oracle.resnet_oracle import normalize_u8, DATASET_MEAN, DATASET_STD
    from wsi_segmentation_pipeline_amd.engine import normalize_lut
    lut = normalize_lut(DATASET_MEAN, DATASET_STD)
    codes = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16).repeat(3, 1)
    ref = normalize_u8(codes).numpy().reshape(3, 256)
    assert np.array_equal(lut, ref)                                      # bit-exact: u8 -> fp32 affine


def _bf16_to_f32(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def test_prepack_conv_roundtrip(lib):
    rng = np.random.default_rng(0)
    cout, cin, k = 64, 128, 3
    w = rng.standard_normal((cout, cin, k, k)).astype(np.float32)
    g = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    m = rng.standard_normal(cout).astype(np.float32)
    v = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for planes in (1, 2):
        nbytes = lib.wsi_prepack_conv_bytes(cout, cin, k, planes)
        nblocks = (cout // 32) * (cin * planes // 64) * k * k * 4096
        assert nbytes == nblocks + (cout * 4 if planes == 2 else 0)      # mode 2: + the inverse per-channel weight scales
        pk = np.zeros(nbytes // 2, np.uint16)
        bias = np.zeros(cout, np.float32)
        assert lib.wsi_prepack_conv(p(w), p(g), p(b), p(m), p(v), 1e-5, cout, cin, k, planes, p(pk), p(bias)) == 0
        scale = g.astype(np.float64) / np.sqrt(v.astype(np.float64) + 1e-5)
        wf = (w.astype(np.float64) * scale[:, None, None, None]).astype(np.float32)
        assert np.allclose(bias, b - m * scale, atol=1e-6)
        # unpack [ntile][line][tap][f][lane][8] back to OIHW and compare hi+lo against the folded weights
        nl = cin * planes // 64
        body = pk[:nblocks // 2]
        if planes == 2:                                                  # fp16 pair of (weight x 2^e), max |.| per channel in [2^13, 2^14)
            frag = body.view(np.float16).astype(np.float32).reshape(cout // 32, nl, k * k, 4, 64, 8)
            inv = pk[nblocks // 2:].view(np.float32)
            assert inv.shape == (cout,) and np.all(np.log2(inv) == np.round(np.log2(inv)))
        else:
            frag = _bf16_to_f32(body).reshape(cout // 32, nl, k * k, 4, 64, 8)
            inv = np.ones(cout, np.float32)
        rec = np.zeros_like(wf)
        for nt in range(cout // 32):
            for l in range(nl):
                for f in range(4):
                    cbase = 32 * l + 16 * (f & 1) if planes == 2 else 64 * l + 16 * f
                    for lane in range(64):
                        co = nt * 32 + (lane & 31)
                        ci = cbase + 8 * (lane >> 5)
                        rec[co, ci:ci + 8] += frag[nt, l, :, f, lane, :].T.reshape(8, k, k)
        if planes == 2:
            amax = np.abs(rec).reshape(cout, -1).max(1)
            assert np.all((amax >= 2.0 ** 13) & (amax < 2.0 ** 14))
        rec = rec * inv[:, None, None, None]
        tol = 2 ** -21 if planes == 2 else 2 ** -8                       # fp16 pair: 22 significand bits where lo is normal
        assert np.abs(rec - wf).max() <= tol * np.abs(wf).max()


def test_bad_arguments_return_einval(lib):
    assert lib.wsi_prepack_conv_bytes(48, 64, 3, 2) == 0
    assert lib.wsi_prepack_conv(None, None, None, None, None, 1e-5, 64, 64, 3, 2, None, None) == -22
    assert lib.wsi_conv3x3_bn_act(None, None, None, None, None, 1, 8, 8, 64, 64, 1, 1, 2, None) == -22
    assert lib.wsi_trunk_forward(None, None, None, 0, 0, 0, None, None, 1, 64, 64, None, 0, None, None, None, None) == -22


def test_prepack_conv_mode3_fp6_planes(lib):
    """Mode-3 weight pack (fp16 hi + MX-fp6 cross-term planes, include/wsi_hip.h): decode the 4 KB blocks on the host and check
    them against the weights - frag 0/1 = fp16(w) in activation line order, frag 2/3 of lanes h=0 = fp6(hi / 2^(s-127)) and of
    lanes h=1 = fp6((w - hi) / 2^(s-127)) in the field order the conv epilogue produces, every element within half an fp6 step
    of its source and the block maximum inside fp6's top binade."""
    rng = np.random.default_rng(3)
    cout, cin, k = 32, 64, 3
    w = (rng.standard_normal((cout, cin, k, k)) * rng.uniform(0.05, 3.0, (1, cin, 1, 1))).astype(np.float32)
    nbytes = lib.wsi_prepack_conv_bytes(cout, cin, k, 3)
    assert nbytes == (cout // 32) * (cin // 32) * 9 * 4096
    out = np.zeros(nbytes, np.uint8)
    bias = np.zeros(cout, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.wsi_prepack_conv(p(w), None, None, None, None, 1e-5, cout, cin, k, 3, p(out), p(bias)) == 0
    assert not bias.any()
    line_chan = lambda pos: 8 * ((pos & 15) >> 2) + 4 * (pos >> 4) + (pos & 3)          # common.h mx_line_chan
    field_chan = lambda f: line_chan(16 * (f & 1) + (f >> 1))                           # common.h mx6_field_chan

    def fp6(code):
        e, m = (code >> 3) & 3, code & 7
        v = (8 + m) * (0.125, 0.25, 0.5)[e - 1] if e else m * 0.125
        return -v if code & 32 else v
    blocks = out.reshape(cin // 32, 9, 4, 64, 16)
    worst = 0.0
    for l in range(cin // 32):
        for t in range(9):
            for r in (0, 5, 31):
                wrow = w[r, 32 * l:32 * l + 32, t // 3, t % 3]
                hi = wrow.astype(np.float16).astype(np.float32)
                lo = wrow - hi
                for h in (0, 1):
                    lane = r + 32 * h
                    f16 = np.concatenate([blocks[l, t, 0, lane].view(np.float16), blocks[l, t, 1, lane].view(np.float16)])
                    pos = [8 * h + j for j in range(8)] + [16 + 8 * h + j for j in range(8)]
                    assert np.array_equal(f16.astype(np.float32), hi[[line_chan(q) for q in pos]])
                    words = np.concatenate([blocks[l, t, 2, lane].view(np.uint32), blocks[l, t, 3, lane].view(np.uint32)[:2]])
                    sbyte = int(blocks[l, t, 3, lane].view(np.uint32)[2])
                    bits = int.from_bytes(words.tobytes(), 'little')
                    src = hi if h == 0 else lo
                    amax = float(np.abs(src).max())
                    assert 1 <= sbyte <= 254
                    scale = 2.0 ** (sbyte - 127)
                    assert 3.75 < amax / scale <= 7.75                                    # the top binade, never more than saturation
                    for f in range(32):
                        q = fp6((bits >> (6 * f)) & 63) * scale
                        x = float(src[field_chan(f)])
                        step = 0.5 if abs(x) / scale >= 4 else 0.25 if abs(x) / scale >= 2 else 0.125
                        worst = max(worst, abs(q - x) / (step * scale))
    assert worst <= 0.5 + 1e-6


def test_unet_tail_prepack_is_the_polyphase_sum(lib):
    """wsi_unet_tail_prepack (host side of csrc/tail.hip): decoding the fp16 hi + lo fragments and undoing the per-channel power-of-two
    scale gives, per output parity (py, px) and low-resolution offset, the SUM of the 3x3 taps whose nearest-upsampled source falls on
    that offset (BN scale folded) - and running that 2 x 3-tap filter bank on a low-resolution image equals the 3x3 conv on its x2
    nearest upsampling.  conv2's fragments: rows 0-15 = output row k (dy = input row), rows 16-31 = output row k + 1 (dy = input row - 1)."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(3)
    cin, cmid, classes = 32, 16, 3
    w1 = rng.normal(0, 0.2, (cmid, cin, 3, 3)).astype(np.float32)
    w2 = rng.normal(0, 0.3, (cmid, cmid, 3, 3)).astype(np.float32)
    bn = [[rng.uniform(0.5, 1.5, cmid).astype(np.float32), rng.normal(0, 0.1, cmid).astype(np.float32),
           rng.normal(0, 0.1, cmid).astype(np.float32), rng.uniform(0.5, 1.5, cmid).astype(np.float32)] for _ in range(2)]
    hw = rng.normal(0, 1, (classes, cmid)).astype(np.float32)
    hb = rng.normal(0, 1, classes).astype(np.float32)
    blob = np.zeros(lib.wsi_unet_tail_prepack_bytes(), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.wsi_unet_tail_prepack(p(w1), *[p(a) for a in bn[0]], p(w2), *[p(a) for a in bn[1]], 1e-5, p(hw), p(hb), cin, cmid, classes, p(blob)) == 0
    assert lib.wsi_unet_tail_prepack(p(w1), *[p(a) for a in bn[0]], p(w2), *[p(a) for a in bn[1]], 1e-5, p(hw), p(hb), 64, cmid, classes, p(blob)) == -22
    fl = blob[(48 + 24) * 1024:].view(np.float32)
    sc = [bn[j][0].astype(np.float64) / np.sqrt(bn[j][3].astype(np.float64) + 1e-5) for j in range(2)]
    sh = [bn[j][1].astype(np.float64) - bn[j][2].astype(np.float64) * sc[j] for j in range(2)]
    assert np.allclose(fl[16:32], sh[0], rtol=1e-6, atol=1e-7) and np.allclose(fl[48:64], sh[1], rtol=1e-6, atol=1e-7)
    assert np.array_equal(fl[64:64 + 64].reshape(4, 16)[:classes], hw) and np.array_equal(fl[128:128 + classes], hb) and not fl[64 + 16 * classes:128].any()
    frags = blob[:(48 + 24) * 1024].view(np.float16).astype(np.float64).reshape(-1, 64, 8)       # [fragment][lane][j]

    def conv1_weight(py, t, row, ci):                            # hi + lo of A row `row`, input channel ci, tap t of parity class py
        base = (py * 6 + t) * 4
        f, lane, j = ci // 16, row + 32 * ((ci % 16) // 8), ci % 8
        return frags[base + f, lane, j] + frags[base + 2 + f, lane, j]
    wsets = {0: ([0], [1, 2]), 1: ([0, 1], [2])}                 # parity -> taps d feeding (first, second) low-resolution offset
    got = np.zeros((2, 2, 2, 3, cmid, cin))                     # [py][px][a][ox index][c][ci]
    for py in range(2):
        for t in range(6):
            for row in range(32):
                px, c = row // 16, row % 16
                for ci in range(cin):
                    got[py, px, t // 3, t % 3, c, ci] = conv1_weight(py, t, row, ci) * fl[c]
    wf = (w1.astype(np.float64) * sc[0][:, None, None, None]).astype(np.float32).astype(np.float64)
    for py in range(2):
        for px in range(2):
            for a_ in range(2):
                for oxi in range(3):
                    b_ = oxi - px
                    exp = np.zeros((cmid, cin))
                    if 0 <= b_ <= 1:
                        for dy in wsets[py][a_]:
                            for dx in wsets[px][b_]:
                                exp += wf[:, :, dy, dx]
                    assert np.abs(got[py, px, a_, oxi] - exp).max() <= 2e-6 * np.abs(wf).max(), (py, px, a_, oxi)
    # the filter bank on a low-resolution image == the 3x3 conv on its nearest x2 upsampling (the identity the kernel rests on)
    x = torch.from_numpy(rng.normal(0, 1, (1, cin, 6, 7)))
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), torch.from_numpy(wf), padding=1)
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros_like(ref)
    for py in range(2):
        for px in range(2):
            acc = 0
            for a_ in range(2):
                for oxi in range(3):
                    oy, ox = py - 1 + a_, oxi - 1
                    acc = acc + torch.einsum('oc,nchw->nohw', torch.from_numpy(got[py, px, a_, oxi]), xp[:, :, 1 + oy:1 + oy + 6, 1 + ox:1 + ox + 7])
            out[:, :, py::2, px::2] = acc
    assert float((out - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    # conv2: 12 taps = 4 input rows x 3 columns, two output rows per tile
    w2f = (w2.astype(np.float64) * sc[1][:, None, None, None]).astype(np.float32).astype(np.float64)
    for t in range(12):
        for row in range(32):
            rs, c = row // 16, row % 16
            dy, dx = t // 3 - rs, t % 3
            for ci in range(cmid):
                lane, j = row + 32 * (ci // 8), ci % 8
                v = (frags[48 + t * 2, lane, j] + frags[48 + t * 2 + 1, lane, j]) * fl[32 + c]
                exp = w2f[c, ci, dy, dx] if 0 <= dy <= 2 else 0.0
                assert abs(v - exp) <= 2e-6 * np.abs(w2f).max(), (t, row, ci)


def test_unet_tail_bands_rule(lib):
    """wsi_unet_tail_bands (the fused tail's bands per image, csrc/tail.hip): a power of two dividing h with h / b >= 8 (one band when
    h < 8); on 256 CUs the shipped batch of 512 tiles of 256 x 256 (h = 128 low-resolution rows) runs ONE band per image and a single
    image 16; every count 1 .. 16 is reached by some batch <= 512 (tests/test_gpu_unet_tail_edges.py runs each of them)."""
    f = lib.wsi_unet_tail_bands
    for cus in (1, 80, 256, 304):
        for h in list(range(1, 130)) + [256, 384, 512]:
            for n in (1, 2, 3, 5, 16, 31, 32, 33, 64, 100, 255, 256, 257, 512, 1008, 1009, 4096):
                b = f(n, h, cus)
                assert b >= 1 and b & (b - 1) == 0 and h % b == 0, (n, h, cus, b)
                assert h // b >= 8 or (h < 8 and b == 1), (n, h, cus, b)
    assert f(512, 128, 256) == 1 and f(1, 128, 256) == 16
    assert {f(n, 128, 256) for n in range(1, 513)} == {1, 2, 4, 8, 16}
    assert f(0, 128, 256) == -22 and f(1, 0, 256) == -22 and f(1, 128, 0) == -22


def test_s2_slab_images_rule(lib):
    """wsi_s2_slab_images (images per launch of the stride-2 block entry's phase-slab kernel, csrc/capi.hip): the whole batch when its
    PF input is under 4 GiB, else the largest count that is, so consecutive launches of that many images (the last one shorter) cover
    the batch and each reads less than 4 GiB.  The layer-2 entry of 512 x 512 patches reads 128 x 128 x 64 maps: 1008 images per
    launch at 4 bytes per channel (modes 2 and 3), 2016 at 2 (mode 1)."""
    f, pf = lib.wsi_s2_slab_images, lib.wsi_pf_bytes
    lim = 0xffffffff
    assert f(1008, 128, 128, 64, 2) == f(1008, 128, 128, 64, 3) == 1008
    assert f(1009, 128, 128, 64, 2) == f(1009, 128, 128, 64, 3) == 1008
    assert f(2016, 128, 128, 64, 1) == 2016 and f(2017, 128, 128, 64, 1) == 2016
    for planes in (1, 2, 3):
        for hw, cin in ((64, 64), (72, 64), (96, 64), (128, 64), (192, 64), (256, 64), (32, 128), (16, 256)):
            for n in (1, 2, 450, 451, 1000, 1008, 1009, 1550, 2016, 2017, 3148, 3149, 3970, 3971, 6162, 24648):
                per = f(n, hw, hw, cin, planes)
                assert 1 <= per <= n, (planes, hw, n, per)
                assert pf(per, hw, hw, cin, planes) < lim, (planes, hw, n, per)
                assert per == n or pf(per + 1, hw, hw, cin, planes) >= lim, (planes, hw, n, per)
                sizes = [min(per, n - i) for i in range(0, n, per)]   # the launches of wsi_conv3x3s2_ds_fused
                assert sum(sizes) == n and min(sizes) >= 1 and max(sizes) == per
    assert f(1, 8192, 8192, 64, 3) == 0                          # one image over 4 GiB: no slab launch at all
    assert f(0, 128, 128, 64, 3) == -22 and f(1, 0, 128, 64, 3) == -22 and f(1, 128, 128, 0, 3) == -22
    assert f(1, 128, 128, 64, 0) == -22 and f(1, 128, 128, 64, 4) == -22


def _ints(n, seed, lo, hi):
    """n fp32 values in [lo, hi] from integer arithmetic alone (no random generator: the digests below must not depend on numpy's)"""
    u = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed)) % np.uint64(20011)
    return (lo + (hi - lo) * (u.astype(np.float64) / 20010.0)).astype(np.float32)


def _bn(n, seed):
    """BatchNorm weight, bias, running mean and running variance of n channels"""
    return [_ints(n, seed + 1, 0.5, 1.5), _ints(n, seed + 2, -1.0, 1.0), _ints(n, seed + 3, -1.0, 1.0), _ints(n, seed + 4, 0.5, 1.5)]


def _packed_weight_digests(lib):
    import hashlib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    sha = lambda *arrays: hashlib.sha256(b''.join(a.tobytes() for a in arrays)).hexdigest()
    none4 = [None] * 4
    got = {}
    for cout, cin, k in ((64, 128, 3), (128, 64, 1)):
        w = _ints(cout * cin * k * k, 7 * cout + k, -1.0, 1.0).reshape(cout, cin, k, k)
        w[3] = 0.0                                                       # an all-zero channel: scale 1
        w[5] *= np.float32(2.0 ** -100)                                  # the exponent clamp of the planes-2 channel scale
        w[6] *= np.float32(2.0 ** 20)
        for planes in (1, 2, 3):
            for bn in (_bn(cout, cin), none4):
                pk = np.full(lib.wsi_prepack_conv_bytes(cout, cin, k, planes), 0xa5, np.uint8)
                bias = np.zeros(cout, np.float32)
                assert lib.wsi_prepack_conv(p(w), *[p(a) for a in bn], 1e-5, cout, cin, k, planes, p(pk), p(bias)) == 0
                got['conv %d %d %d planes %d %s' % (cout, cin, k, planes, 'bn' if bn is not none4 else 'no bn')] = sha(pk, bias)
    w = _ints(64 * 3 * 7 * 7, 11, -0.5, 0.5)
    bn = _bn(64, 13)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    for planes in (1, 2, 3):
        pk = np.full(lib.wsi_prepack_stem_bytes(planes), 0xa5, np.uint8)
        bias = np.zeros(64, np.float32)
        assert lib.wsi_prepack_stem(p(w), *[p(a) for a in bn], 1e-5, planes, p(pk), p(bias)) == 0
        got['stem planes %d' % planes] = sha(pk, bias)
    pk = np.full(lib.wsi_prepack_stem_bytes(2), 0xa5, np.uint8)
    bias = np.zeros(64, np.float32)
    assert lib.wsi_prepack_stem_u8(p(w), *[p(a) for a in bn], 1e-5, p(mean), p(std), 2, p(pk), p(bias)) == 0
    got['stem u8 planes 2'] = sha(pk, bias)
    for cmid in (16, 12):
        w1, w2 = _ints(cmid * 32 * 9, 17, -0.6, 0.6), _ints(cmid * cmid * 9, 19, -0.9, 0.9)
        hw, hb = _ints(3 * cmid, 23, -2.0, 2.0), _ints(3, 29, -1.0, 1.0)
        for head_b in (hb, None):
            blob = np.full(lib.wsi_unet_tail_prepack_bytes(), 0xa5, np.uint8)
            assert lib.wsi_unet_tail_prepack(p(w1), *[p(a) for a in _bn(cmid, 31)], p(w2), *[p(a) for a in _bn(cmid, 37)], 1e-5, p(hw),
                                             p(head_b), 32, cmid, 3, p(blob)) == 0
            got['tail cmid %d %s' % (cmid, 'head_b' if head_b is not None else 'no head_b')] = sha(blob)
    lut = np.zeros(3 * 256, np.float32)
    assert lib.wsi_normalize_u8_lut(p(mean), p(std), p(lut)) == 0
    got['lut'] = sha(lut)
    return got


# recorded from the library as built before the split (the commit that named the conv route switches)
_PACKED_WEIGHT_DIGESTS = {'conv 64 128 3 planes 1 bn': '7f9f8b331290550917daf0a750667d19aadc9b4ce62d638e3576a8ef62506464',
 'conv 64 128 3 planes 1 no bn': '3abc4473eeaf78fb4162ccefb7aeadb1e70a5081a8a61acf0c5f01a70872e5ea',
 'conv 64 128 3 planes 2 bn': '145e747e351e27c4781efa2954d97db970107b59198f5dd91ccadcc536179766',
 'conv 64 128 3 planes 2 no bn': '2e3c247f046afd760c547edb82cb152b4c6d34aefe735789e7d18fa5bb7a5a87',
 'conv 64 128 3 planes 3 bn': 'f694529bca8228f95a1f4bc3f4508a2146a664ad325329c6bc631e0dc458c026',
 'conv 64 128 3 planes 3 no bn': 'fd3449a9a7bff0757ac3e100873aa126110b12a1cbb05e948f71722adb0c4479',
 'conv 128 64 1 planes 1 bn': '603b86a62ff34590f2f335eccc1b52c389adf842e9ec34497b2f6aa1c54a7779',
 'conv 128 64 1 planes 1 no bn': '7bbeecd389ec414a9592ad9ae3bdc126f15a2007fd5c6bdb5d7cb275a3384761',
 'conv 128 64 1 planes 2 bn': '6a503aae9622ea660fcb78e584eb3b163c2b7764a26fba9afa88de17ec6565ea',
 'conv 128 64 1 planes 2 no bn': '1336745a7aa4a7de7481580c0ff03326bc913fa220b1d35c5f7c70fc1cf61651',
 'conv 128 64 1 planes 3 bn': 'b84e1275e17694c0e66aa30860014c76b051207e2e1d8cf88a87b089093338f9',
 'conv 128 64 1 planes 3 no bn': '5a6328ecc9fa9f9cc5cbd22ad1a31b63c346a51fe759562f61a94df85fe67bd5',
 'stem planes 1': '9b5d8af972e1fc956264ef09f720ed9be8850cece1955160bb8684fc946847c2',
 'stem planes 2': '3bc3bf5b348c2ad49b2b05a471c569c00288c38076e91a8698c0595db7a502bc',
 'stem planes 3': '3bc3bf5b348c2ad49b2b05a471c569c00288c38076e91a8698c0595db7a502bc',
 'stem u8 planes 2': '64426db08384fafb2b055d76cfc00044c4a6dd60ef18d4d6b383af78e1f1d105',
 'tail cmid 16 head_b': 'd2db4cd5b15e4b97192246de1783ae42de631537c25e1ae495730aa320a9b737',
 'tail cmid 16 no head_b': 'a8555cc24a547e896b6f2ab4e663d9ffa84293c3620a74a1e61e09f659389aab',
 'tail cmid 12 head_b': 'be1e2dac5223069610c7956bfcb211fb9102e323f0bc0d9938e8f8d02a84ac71',
 'tail cmid 12 no head_b': '708e96f9ec1a60a3313891a220fac0c255d6facd94667f6575322287ce849dc4',
 'lut': '1d8b9af12b7b391827f7c801265239e21435c7e29b4d78c6189a35e437633897'}


def test_packed_weights_byte_identical(lib):
    """Every host-side pack (wsi_prepack_conv at planes 1-3 with and without BN, with an all-zero output channel, one at 2^-100 - the
    exponent clamp of the channel scale - and one at 2^20; wsi_prepack_stem, wsi_prepack_stem_u8, wsi_unet_tail_prepack, wsi_normalize_u8_lut)
    is byte for byte what the library produced before csrc/prepack.hip was split off and folded each weight once: SHA-256 over the
    packed bytes and the bias, inputs from integer arithmetic.  The buffers start as 0xa5, so a byte the pack stops writing shows
    as well."""
    assert _packed_weight_digests(lib) == _PACKED_WEIGHT_DIGESTS
