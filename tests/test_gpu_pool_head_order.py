"""wsi_avgpool_fc in mx mode (csrc/heads.hip avgpool_fc_mx_kernel: one wave per image, a lane owns whole 32-channel lines) against a
NumPy fp32 model of its summation order, bit for bit.  The order is part of the contract: per channel, chain k of npg = 64 / (C / 32)
adds the pixels p = k, k + npg, ... in ascending order onto +0.0f, each term (float)hi + lo6 * scale; the chains are combined as
((0 + part[0]) + part[1]) + ..., then * 1 / (H W); logit k is the sum over lanes l of (sum over c = l, l + 64, ... of
feat[c] * w[k][c]) by a butterfly (offsets 32, 16, .., 1), + b[k].  Inputs with exact sums (a coarse grid) and with inexact ones."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pf_lines_oracle as O

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


def model(terms, wt, b):
    """terms: (n, c, hw) float32, the decoded values in raster order -> (feat, logits, the pooled sums before * 1 / (H W)), every
    operation rounded to float32"""
    n, c, hw = terms.shape
    npg = 64 // (c // 32)
    part = np.zeros((npg, n, c), F)
    for k in range(npg):
        for p in range(k, hw, npg):
            part[k] = part[k] + terms[:, :, p]
    t = np.zeros((n, c), F)
    for k in range(npg):
        t = t + part[k]
    feat = t * (F(1.0) / F(hw))
    lanes = np.arange(64)
    logits = np.zeros((n, wt.shape[0]), F)
    for k in range(wt.shape[0]):
        acc = np.zeros((n, 64), F)
        for c0 in range(0, c, 64):
            m = min(64, c - c0)
            acc[:, :m] = acc[:, :m] + feat[:, c0:c0 + m] * wt[k, c0:c0 + m]
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ o]
        logits[:, k] = acc[:, 0] + b[k]
    return feat, logits, t


# The last four pin the chain walk over padded-flat positions: 512 at 6 x 6 (step 4 against a row of 6: the wrap falls on a different
# x every row, nine pixels a chain = two full groups of loads in flight and one partial), 256 at 6 x 6 (step 8 = one row + 2: row and
# column step together, chains of 5 and of 4 pixels), 1024 at 3 x 3 (two chains, odd map), 96 at 5 x 5 (3 lines: 21 chains on 63
# lanes, one lane idle, chains of 2 and of 1 pixels).
@pytest.mark.parametrize('c,h,w,n', [(512, 8, 8, 5), (64, 4, 4, 1), (256, 2, 2, 9), (512, 6, 6, 3), (256, 6, 6, 2), (1024, 3, 3, 2), (96, 5, 5, 6)])
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'inexact'])
def test_pool_head_matches_the_summation_order(dev, c, h, w, n, exact):
    from wsi_segmentation_pipeline_amd import engine as E, native
    lib = native.load()
    rng = np.random.default_rng(c + 10 * n + exact)
    # exact: multiples of 2^-6 below 4 (fp16 holds them, the lo part is zero, every partial sum is a float32)
    x = (rng.integers(-255, 256, (n, c, h, w)) / 64.0).astype(F) if exact else (rng.standard_normal((n, c, h, w)) * 3.0).astype(F)
    K = 4
    wt = (rng.integers(-8, 9, (K, c)) / 8.0).astype(F) if exact else (rng.standard_normal((K, c)) * 0.05).astype(F)
    b = (rng.standard_normal(K) * 0.1).astype(F)
    buf = E.pf_pack(torch.from_numpy(x).to(dev), 3)                                     # lines built by wsi_pf_pack
    torch.cuda.synchronize()
    lines = O.real_lines(buf.cpu().numpy(), n, c, h, w, 3)
    terms = O.from_lines(O.decode(lines, 3), n, c, h, w).reshape(n, c, h * w)            # (float)hi + lo6 * scale, float32
    want_f, want_l, sums = model(terms, wt, b)
    if exact:                                                                            # the premise of the exact case (the sums: 1 / (H W) is
        assert np.array_equal(sums.astype(np.float64), terms.astype(np.float64).sum(2))  # a power of two on some of the maps only)
    wd, bd = torch.from_numpy(wt).to(dev), torch.from_numpy(b).to(dev)
    fo = torch.full((n, c), float('nan'), device=dev)
    lo = torch.full((n, K), float('nan'), device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    native.check(lib.wsi_avgpool_fc(buf.data_ptr(), n, h, w, c, wd.data_ptr(), bd.data_ptr(), K, fo.data_ptr(), lo.data_ptr(), 3, st),
                 'wsi_avgpool_fc')
    torch.cuda.synchronize()
    got_f, got_l = fo.cpu().numpy(), lo.cpu().numpy()
    print('c %d %dx%d n %d exact %d: feat bits differ %d, logit bits differ %d' % (
        c, h, w, n, exact, int((got_f.view(np.uint32) != want_f.view(np.uint32)).sum()), int((got_l.view(np.uint32) != want_l.view(np.uint32)).sum())))
    assert np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32))
    assert np.array_equal(got_l.view(np.uint32), want_l.view(np.uint32))
