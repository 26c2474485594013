#!/usr/bin/env python3
"""Milliseconds of the six stain-normalisation kernels (csrc/stain.hip) on one resident level, what each reaches of the copy rate, the
two applies beside the same arithmetic in torch ops, and the normalisation of a slide beside that slide's infer_slide_cls.

  python tools/stain_times.py [--size 16384] [--window 1.0] [--repeats 3] [--out profiles/stain_bench.json] [--parity profiles/stain_parity.json]

A synthetic H&E-like level of size x size pixels is built on the device (805 MB at the default: larger than the 256 MiB Infinity Cache).
The versions alternate in one process; each gets a window of at least --window seconds of back-to-back calls (HIP events per call) after
a warm-up of every version, and the whole comparison is repeated --repeats times: the figure is the median round, the spread its range.
Bytes a kernel has to move: 3 per pixel for a fit step (one read of the level), 6 per pixel for an apply (one read, one write); the share
is those bytes over the time, against the 6.29 TB/s of a device-to-device copy (README.md).  `copy` is that copy itself on this level.
The parity file holds, for a 1024 x 1024 crop, the device fit and the two applies against the float64 spec (tests/stain_oracle.py).
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from wsi_segmentation_pipeline_amd import native, slide as S, stain, synthetic as W  # noqa: E402
from wsi_segmentation_pipeline_amd.engine import TrunkEngine  # noqa: E402

COPY_RATE = 6.29e12                      # bytes / s of a device-to-device copy on this card (README.md)


def he_level(size, dev, seed=5):
    """H&E-like u8 (size, size, 3): saturated white background, pink stroma in smooth regions (about a third of the level), purple nuclei,
    noise - built in bands of 1024 rows from two low-resolution random fields"""
    g = torch.Generator(device=dev).manual_seed(seed)
    lo = max(8, size // 256)
    field = torch.rand((1, 1, lo, lo), device=dev, generator=g)
    nuc = torch.rand((1, 1, size // 8, size // 8), device=dev, generator=g)
    out = torch.empty((size, size, 3), dtype=torch.uint8, device=dev)
    stroma = torch.tensor([185., 115., 165.], device=dev)
    purple = torch.tensor([80., 45., 130.], device=dev)
    up = torch.nn.functional.interpolate(field, size=(size // 8, size // 8), mode='bilinear', align_corners=False)
    for y in range(0, size, 1024):
        rows = min(1024, size - y)
        t = torch.nn.functional.interpolate(up[:, :, y // 8:(y + rows + 7) // 8], size=(rows, size), mode='bilinear', align_corners=False)[0, 0] > 0.58
        n = torch.nn.functional.interpolate(nuc[:, :, y // 8:(y + rows + 7) // 8], size=(rows, size), mode='nearest')[0, 0] > 0.9
        img = torch.full((rows, size, 3), 255.0, device=dev)
        noise = torch.randn((rows, size, 3), device=dev, generator=g) * 10
        img = torch.where(t[..., None], stroma + noise, img)
        img = torch.where((t & n)[..., None], purple + noise, img)
        out[y:y + rows] = img.round().clamp(0, 255).to(torch.uint8)
    return out


def torch_macenko(img, m, io, lut, v_max):
    """wsi_stain_macenko_apply in torch ops (fp32), background kept"""
    od = lut[img.reshape(-1, 3).long()]
    new = torch.floor(io * torch.exp2(od @ m.t()) + 0.5).clamp_(0, 255).to(torch.uint8).view(img.shape)
    return torch.where((img.amax(-1) <= v_max)[..., None], new, img)


def torch_reinhard(img, g33, g3, rgb2lms, lms2rgb256, v_max):
    """wsi_stain_reinhard_apply in torch ops (fp32), background kept"""
    rgb = (img.reshape(-1, 3).float() + 1.0) * (1.0 / 256)
    lms = torch.exp2(torch.log2(rgb @ rgb2lms.t()) @ g33.t() + g3)
    new = torch.floor(lms @ lms2rgb256.t() - 0.5).clamp_(0, 255).to(torch.uint8).view(img.shape)
    return torch.where((img.amax(-1) <= v_max)[..., None], new, img)


def timed(versions, window, repeats):
    rounds = {k: [] for k in versions}
    for _ in range(repeats):
        for k, fn in versions.items():                                        # the versions alternate
            spent, calls = 0.0, 0
            while spent < window * 1e3:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                spent += a.elapsed_time(b)
                calls += 1
            rounds[k].append(spent / calls)
    return rounds


def parity(level, dev):
    import stain_oracle as SO
    crop = level[:1024, :1024].contiguous()
    host = crop.cpu().numpy()
    doc = {'what': 'a 1024 x 1024 crop of the level: device against tests/stain_oracle.py (float64)', 'tissue_share': round(float(SO.tissue(host).mean()), 4)}
    he, mc, n = SO.fit_macenko(host)
    p = stain.fit_macenko(crop)
    ang = [math.atan2(float(np.linalg.norm(np.cross(p.he[:, k], he[:, k]))), float(p.he[:, k] @ he[:, k])) for k in range(2)]
    doc['macenko_fit'] = {'n_equal': bool(p.n == n), 'he_angle_to_oracle_rad': ang, 'angle_bin_rad': 2 * math.pi / stain.ANGLE_BINS,
                          'max_c_minus_oracle': [float(v) for v in p.max_c - mc], 'conc_bin': stain.CONC_MAX / stain.CONC_BINS}
    mean, std, _ = SO.fit_reinhard(host)
    r = stain.fit_reinhard(crop)
    doc['reinhard_fit'] = {'mean_relative': float(np.abs(r.mean / mean - 1).max()), 'std_relative': float(np.abs(r.std / std - 1).max())}
    tgt = stain.ReinhardParams(mean + np.array([0.08, -0.02, 0.01]), std * np.array([1.15, 0.9, 1.1]), n)
    for bg in ('keep', 'all'):
        for name, got, want in (('macenko', stain.normalize_macenko(crop, stain.MacenkoParams(he, mc, n), background=bg),
                                 SO.apply_macenko(host, SO.macenko_matrix(he, mc), bg)),
                                ('reinhard', stain.normalize_reinhard(crop, tgt, stain.ReinhardParams(mean, std, n), background=bg),
                                 SO.apply_reinhard(host, (mean, std), (tgt.mean, tgt.std), bg))):
            d = np.abs(got.cpu().numpy().astype(int) - want.astype(int))
            doc['%s_apply_%s' % (name, bg)] = {'bytes': int(d.size), 'differ': int((d > 0).sum()), 'share': float((d > 0).mean()), 'largest': int(d.max())}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--parity', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs a GPU')
    dev = torch.device('cuda:0')
    lib = native.load()
    size = args.size
    level = he_level(size, dev)
    npix = size * size
    st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    v_max = stain.tissue_v_max()
    lut = torch.from_numpy(stain.od_table()).to(dev)
    # parameters: fitted on the x16 thumbnail, as StainedSlide does
    thumb = level[::16, ::16].contiguous()
    mp, rp = stain.fit_macenko(thumb), stain.fit_reinhard(thumb)
    rt = stain.ReinhardParams(rp.mean + np.array([0.08, -0.02, 0.01]), rp.std * np.array([1.15, 0.9, 1.1]), rp.n)
    m33 = torch.from_numpy((-math.log2(math.e) * stain.macenko_matrix(mp)).astype(np.float32)).to(dev)
    g33_64, g3_64 = stain.reinhard_affine(rp, rt)
    g12 = torch.from_numpy(np.concatenate((g33_64.reshape(9), g3_64 * math.log2(10.0))).astype(np.float32)).to(dev)
    plane = torch.from_numpy(stain.macenko_plane(stain._moments(thumb.unsqueeze(0), False, stain.IO, stain.BETA)[0]).astype(np.float32)).to(dev)
    pinv = torch.from_numpy(np.linalg.pinv(mp.he).astype(np.float32)).to(dev)
    vm = torch.tensor([v_max], dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.wsi_stain_moments_scratch_bytes(npix, 1), dtype=torch.uint8, device=dev)
    mom = torch.empty(10, dtype=torch.float64, device=dev)
    hist = torch.empty(2 * stain.CONC_BINS, dtype=torch.int64, device=dev)
    out = torch.empty_like(level)
    p = lambda t: t.data_ptr()
    chk = native.check
    kernels = {
        'od_moments': lambda: chk(lib.wsi_stain_od_moments(p(level), npix, 1, v_max, p(lut), p(mom), p(scratch), st()), 'od_moments'),
        'lab_moments': lambda: chk(lib.wsi_stain_lab_moments(p(level), npix, 1, v_max, p(mom), p(scratch), st()), 'lab_moments'),
        'angle_hist': lambda: chk(lib.wsi_stain_angle_hist(p(level), npix, 1, v_max, p(lut), p(plane), stain.ANGLE_BINS, p(hist), st()), 'angle_hist'),
        'conc_hist': lambda: chk(lib.wsi_stain_conc_hist(p(level), npix, 1, v_max, p(lut), p(pinv), stain.CONC_BINS, stain.CONC_MAX, p(hist), st()), 'conc_hist'),
        'macenko_apply': lambda: chk(lib.wsi_stain_macenko_apply(p(level), p(out), npix, 1, p(vm), p(lut), p(m33), float(stain.IO), st()), 'macenko_apply'),
        'reinhard_apply': lambda: chk(lib.wsi_stain_reinhard_apply(p(level), p(out), npix, 1, p(vm), p(g12), st()), 'reinhard_apply'),
    }
    rgb2lms = torch.from_numpy(stain.RGB2LMS.astype(np.float32)).to(dev)
    lms2rgb256 = torch.from_numpy((256 * stain.LMS2RGB).astype(np.float32)).to(dev)
    versions = dict(kernels)
    versions['copy'] = lambda: out.copy_(level)
    versions['macenko_torch_ops'] = lambda: torch_macenko(level, m33, float(stain.IO), lut, v_max)
    versions['reinhard_torch_ops'] = lambda: torch_reinhard(level, g12[:9].view(3, 3), g12[9:], rgb2lms, lms2rgb256, v_max)
    need = {'od_moments': 3, 'lab_moments': 3, 'angle_hist': 3, 'conc_hist': 3, 'macenko_apply': 6, 'reinhard_apply': 6, 'copy': 6,
            'macenko_torch_ops': 6, 'reinhard_torch_ops': 6}
    res = {'what': 'one level of %d x %d pixels (%d MB), tissue share %.3f; HIP events per call, windows of >= %.1f s per version, the versions '
                   'alternating, %d rounds; share = bytes the kernel has to move (3 per pixel for a fit step, 6 for an apply) over its time, '
                   'against the %.2f TB/s copy rate' % (size, size, npix * 3 // 10 ** 6, float((level.amax(-1) <= v_max).float().mean()),
                                                        args.window, args.repeats, COPY_RATE / 1e12)}
    with torch.no_grad():
        kernels['macenko_apply']()
        a = out.clone()
        b = versions['macenko_torch_ops']()
        res['macenko_bytes_differing_from_torch_ops'] = int((a != b).sum())
        kernels['reinhard_apply']()
        a.copy_(out)
        b = versions['reinhard_torch_ops']()
        res['reinhard_bytes_differing_from_torch_ops'] = int((a != b).sum())
        del a, b
        for fn in versions.values():
            fn()
        torch.cuda.synchronize()
        rounds = timed(versions, args.window, args.repeats)
    for k, r in rounds.items():
        ms = float(np.median(r))
        res[k] = {'ms': round(ms, 3), 'rounds_ms': [round(v, 3) for v in r], 'spread': round((max(r) - min(r)) / ms, 4),
                  'share_of_copy_rate': round(need[k] * npix / (ms * 1e-3) / COPY_RATE, 4)}
        print(k, json.dumps(res[k]), flush=True)
    for name in ('macenko', 'reinhard'):
        res['%s_torch_ops_over_kernel' % name] = round(res[name + '_torch_ops']['ms'] / res[name + '_apply']['ms'], 2)
    # a slide: the fit on the thumbnail and the apply on the level, beside infer_slide_cls of that level (ResNet-18, 256 x 256 tiles)
    norm = stain.Normalizer('macenko')

    def normalise_slide():
        norm.apply(level, norm.fit(thumb), out=out)
    eng = TrunkEngine(W.make_resnet18_state_dict(11, with_fc=False), dev, head=tuple(W.make_head_state_dict(22, 'classifier')[k] for k in ('fc.0.weight', 'fc.0.bias')))
    tiles = S.tile_grid(size, size, 256, 256, 256, 256)
    map_hw = (size // 16, size // 16)

    def infer():
        S.infer_slide_cls(eng, out, tiles, 256, 256, 1.0 / 16, map_hw, 4, (0., 0., 0., 0.))
    with torch.no_grad():
        normalise_slide()
        infer()
        torch.cuda.synchronize()
        rounds = timed({'normalise_slide_macenko': normalise_slide, 'infer_slide_cls': infer}, args.window, args.repeats)
    for k, r in rounds.items():
        res[k] = {'ms': round(float(np.median(r)), 3), 'rounds_ms': [round(v, 3) for v in r]}
        print(k, json.dumps(res[k]), flush=True)
    res['infer_slide_cls']['tiles'] = int(len(tiles))
    res['normalise_over_infer'] = round(res['normalise_slide_macenko']['ms'] / res['infer_slide_cls']['ms'], 4)
    for path, doc in ((args.out, res), (args.parity, parity(level, dev) if args.parity else None)):
        if path:
            with open(path, 'w') as fh:
                json.dump(doc, fh, indent=1)
                fh.write('\n')
    print(json.dumps(res['normalise_over_infer']))


if __name__ == '__main__':
    main()
