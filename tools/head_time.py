#!/usr/bin/env python3
"""HIP-event time of wsi_avgpool_fc alone (the trunk's pooling head has no wsi_prof record): the 512-channel 8 x 8 tensor of a batch
of 256 x 256 patches, packed once, the call repeated.
Usage: python tools/head_time.py [--planes 3] [--n 6162] [--reps 200]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wsi_segmentation_pipeline_amd import engine as E, native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--planes', type=int, default=3)
    ap.add_argument('--n', type=int, default=6162)
    ap.add_argument('--reps', type=int, default=200)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    lib = native.load()
    n, c, h, w, K = args.n, 512, 8, 8, 4
    g = torch.Generator(device=dev).manual_seed(5)
    buf = E.pf_pack(torch.randn(n, c, h, w, device=dev, generator=g), args.planes)
    wt, b = torch.randn(K, c, device=dev, generator=g) * 0.05, torch.randn(K, device=dev, generator=g)
    feat, logits = torch.empty(n, c, device=dev), torch.empty(n, K, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        native.check(lib.wsi_avgpool_fc(buf.data_ptr(), n, h, w, c, wt.data_ptr(), b.data_ptr(), K, feat.data_ptr(), logits.data_ptr(),
                                        args.planes, st), 'wsi_avgpool_fc')
    for _ in range(10):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for a, z in ev:
        a.record(); call(); z.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(z) for a, z in ev])
    nbytes = buf.numel() * (0.75 if args.planes == 3 else 1.0)                        # (mx: the hi6 plane is not read)
    print('avgpool_fc planes %d n %d: median %.4f ms  min %.4f  max %.4f  (%.2f TB/s at the median)  checksum %.6f' % (
        args.planes, n, np.median(ms), ms.min(), ms.max(), nbytes / np.median(ms) / 1e9, float(logits.double().sum())))


if __name__ == '__main__':
    main()
