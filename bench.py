#!/usr/bin/env python3
"""Headline benchmark: patches/sec (256x256x3) whole-slide 'cls' inference on MI355X.

Workloads (BASELINE.json configs):
  cfg3 (default, every N) ONE 40 000 x 40 000 synthetic slide, tile 256 / stride 256 -> 24 648 tiles (reference grid
       utils/dataset.py:143-166), the tile list sharded contiguously over the N ranks (STRONG scaling), every rank
       keeping only the slide regions its own tiles touch resident in HBM (slide.region_plan), ONE RCCL all-gather
       of the per-tile logits, float64 stitch + softmax / heat map on every rank.
  cfg2 10 000-tile synthetic slide per GPU (weak scaling; the r01 headline, kept for comparison).
  cfg4 region-proposal bags: R regions x 16 crops of 64x64 (ResNet.forward bag path, resnets_shift.py:189-217),
       bags sharded by count over the ranks, ensemble logits gathered (metric: 64x64 crops/s).
One "step" = one full pass over the slide (or over all bags).  Tile read + colour normalisation + conv stack run
on the HIP kernels of libwsi_hip.so; inputs are resident in HBM when the timed region starts.

`python bench.py --gpus N` starts its own N ranks as fresh child processes (the parent never touches a GPU); under
`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` it uses the ranks it was given.

Prints ONE JSON line: `metric`, `value`, `unit`, `ms_per_step` (wall time of one timed step), `dtype`, ... .  A plain run
sets up, warms up, times --steps steps and prints the line.  Everything measured or checked beside the headline runs only
with --full, after the timed region: `kernels` / `kernel_leg` and the `roofline*` objects (HIP events on the launch stream,
one pass of the same steps with one batch in flight), `roofline_bf16` (the dominant kernel in single-pass bf16),
`cpu_baseline` (the CPU oracle on the host cores over a bounded sample of the same tiles), `contract`, the `parity` leg
(the other precision mode), the `api` leg (the reference-named drop-in API) and cfg5's `postprocess` leg; without --full
those keys are null / empty.

--dump-outputs DIR writes the arrays the last timed step returned (rank 0) as DIR/<name>.npy, float64 for float64 and
32/64-bit integer arrays, float32 otherwise, at most DUMP_BYTES in all: an array over its share of that is replaced by a
fixed sample of its flattened values, the same positions for the same shape in every run (see dump_outputs).  Inputs and
weights are seeded, so two builds given the same arguments can be compared output for output.
"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

TILE = 256
NX = 72                                   # cfg2: (NX+1)*(NY+1) - 1 = 10 000 for NY = 136
PEAK_BF16_TFLOPS = 2500.0                 # dense MFMA bf16 / fp16, MI355X_MICROARCH.md chip table
PEAK_HBM_GBS = 8000.0
# BASELINE.json's metric, verbatim
METRIC = 'patches/sec (256×256×3) whole-slide inference, 1/2/4/8 MI355X + CPU ref'
KIND_NAMES = {1: 'conv3x3_s1', 5: 'conv3x3_s1_layer1', 2: 'conv3x3_s2', 3: 'conv1x1_s2', 4: 'stem_maxpool',
              6: 'unet_decoder_conv3x3', 7: 'unet_glue', 8: 'unet_head_1x1', 10: 'unet_tail_fused'}
SEG_DECODER_GFLOP = 6.04                  # decoder 3x3 convs per 256x256 tile over REAL channels (encoder trunk 3.63 + stem 0.31)
SEG_TILE_GFLOP = 3.63 + 0.31 + 6.04
DUMP_BYTES = 48 << 20                     # --dump-outputs: all files together (.npy headers aside)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--workload', choices=('cfg2', 'cfg3', 'cfg4', 'cfg5', 'seg'), default='cfg3',
                    help="seg: the dense per-pixel mode (predict_tumorbed mode='seg': ResNet-18 encoder + U-Net decoder), --seg-tiles tiles of 256x256 per step")
    ap.add_argument('--seg-tiles', type=int, default=512)
    ap.add_argument('--seg-batch', type=int, default=512, help='seg: tiles per U-Net call (77 MB of workspace per tile; r05 sweep 128 / 256 / 512: 28.1 / 31.2 / 33.1 k patches/s)')
    ap.add_argument('--mode', choices=('parity', 'mx', 'speed'), default=None,
                    help='parity: fp16 hi + fp16 lo pair, 3 MFMA passes (logit error ~1e-5); mx: fp16 pass + MX-fp6 cross terms '
                         '(5e-4, inside the 1e-3 contract); speed: single-pass bf16 (2e-2, outside the contract).  Default: mx; for '
                         '--workload seg parity (the drop-in UNetSeg default: per-pixel logits have no average pool behind them and mx '
                         'is 3-4e-3 off at |logit| 16 there), with an mx leg reported beside it')
    ap.add_argument('--batch', type=int, default=6200, help='cap of tiles per trunk call, <= 51 GB of workspace (r02: 2000 -> 103.8 k, 4200 -> 105.7 k, 6200 -> 106.6 k patches/s; the drop-in engines default to 2000).  A cap of 6656 lets engine.batch_sizes cut 24 648 tiles into whole rounds of the chip (3 x 6 144 + 6 216): +0.2 % (r03, inside the run-to-run noise)')
    ap.add_argument('--tiles', type=int, default=10000, help='cfg2: tiles per GPU per step')
    ap.add_argument('--size', type=int, default=40000, help='cfg3: slide edge in pixels')
    ap.add_argument('--regions', type=int, default=4000, help='cfg4: region bags (16 crops of 64x64 each) in total')
    ap.add_argument('--chunks', type=str, default='', help='stem_chunk,layer1_chunk sub-batch sizes (default: library default)')
    ap.add_argument('--stem', type=str, default='', help='fused,rows_per_seg for the stem kernel (A/B)')
    ap.add_argument('--s2', type=int, default=-1, help='wsi_conv_set_mode value for A/B runs (see include/wsi_hip.h)')
    ap.add_argument('--streams', type=int, default=2, help='batches in flight (HIP streams, own workspace each; r02-r03: +3 %% over one).  The per-kernel HIP-event leg (roofline) runs in '
                         'its own pass with ONE batch in flight right after the timed region: overlapping launches would distort per-kernel times')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-prof', action='store_true', help='disable per-launch HIP events (roofline leg)')
    ap.add_argument('--no-bf16-leg', action='store_true', help='skip the single-pass bf16 timing of the dominant kernel')
    ap.add_argument('--no-parity-leg', action='store_true', help='skip the parity-mode leg after the timed region')
    ap.add_argument('--no-api-leg', action='store_true', help="skip the `api` leg (cfg3 / seg, one GPU): the same slide through the reference-named drop-in API with ITS defaults")
    ap.add_argument('--full', action='store_true', help='after the timed region, also run the legs beside the headline: per-kernel HIP events and '
                         'rooflines, bf16 leg, CPU baseline, contract check, other-precision leg, API leg, cfg5 post-process leg (the --no-* '
                         'switches above then skip single legs)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step returned as DIR/<name>.npy (float32 / float64, a fixed sample of large arrays)')
    return ap.parse_args()


def spawn_ranks(n):
    """Parent of a plain `python bench.py --gpus N`: N fresh child processes, one per GPU, rendezvous on 127.0.0.1.
    The parent makes no GPU call (nothing here imports torch); a failed child fails the run."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    try:
        pending = list(procs)
        while pending:
            for p in list(pending):
                code = p.poll()
                if code is None:
                    continue
                pending.remove(p)
                if code != 0 and rc == 0:
                    rc = code
                    for q in pending:                    # a dead rank leaves the others in the rendezvous: stop them (exact PIDs)
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


def slide_geometry_cfg2(n_tiles):
    ny = (n_tiles + 1 + NX) // (NX + 1) - 1
    while (NX + 1) * (ny + 1) - 1 < n_tiles:
        ny += 1
    return 257 + NX * TILE, 257 + ny * TILE          # (iw, ih)


def collect_prof(lib, np, cap, dt):
    ms = np.zeros(cap, np.float32)
    kind = np.zeros(cap, np.int32)
    fl = np.zeros(cap, np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nrec = lib.wsi_prof_end(p(ms), p(kind), p(fl), cap)
    assert nrec >= 0
    per_kind = {}
    for k, name in KIND_NAMES.items():
        sel = kind[:nrec] == k
        if sel.any():
            tms, tfl = float(ms[:nrec][sel].sum()), float(fl[:nrec][sel].sum())
            per_kind[name] = {'launches': int(sel.sum()), 'avg_ms': tms / int(sel.sum()),
                              'tflops': tfl / (tms * 1e-3) / 1e12, 'share_of_step': (tms * 1e-3 / dt) if dt else None}
    return per_kind


def output_arrays(out, prefix=''):
    """(name, array) pairs of what a step returned: dict entries, nested dicts and the public attributes of result objects
    (postprocess.TumorBed) as '<key>.<attr>', Python numbers as 0-d arrays; None and strings are skipped."""
    import numpy as np
    import torch
    items = out.items() if isinstance(out, dict) else [(k, v) for k, v in vars(out).items() if not k.startswith('_')]
    for k, v in items:
        name = prefix + str(k)
        if isinstance(v, (torch.Tensor, np.ndarray)):
            yield name, v
        elif isinstance(v, (bool, int, float)):
            yield name, np.asarray(v, np.float64)
        elif isinstance(v, dict) or (v is not None and not isinstance(v, str) and hasattr(v, '__dict__')):
            yield from output_arrays(v, name + '.')


def dump_outputs(out, path):
    """--dump-outputs: every array of `out` as path/<name>.npy.  float64 and 32/64-bit integers are written as float64, the
    rest (fp32, u8 maps, bool) as float32.  Smallest first, each array may take an equal share of what the ones before it
    left of DUMP_BYTES; a larger one is written as the 1-d sample of its flattened values at the sorted, de-duplicated
    positions np.unique(default_rng(0).integers(0, n, k)), which depend only on the shapes."""
    import numpy as np
    import torch
    arrays = []
    for name, a in output_arrays(out):
        t = torch.as_tensor(a)
        dt = torch.float64 if t.dtype in (torch.float64, torch.int32, torch.int64) else torch.float32
        arrays.append((t.numel() * (8 if dt == torch.float64 else 4), name, t, dt))
    os.makedirs(path, exist_ok=True)
    left = DUMP_BYTES
    for i, (_, name, t, dt) in enumerate(sorted(arrays, key=lambda e: (e[0], e[1]))):
        k = left // (len(arrays) - i) // (8 if dt == torch.float64 else 4)
        if t.numel() > k:
            flat = t.reshape(-1)
            idx = np.unique(np.random.default_rng(0).integers(0, flat.numel(), k))
            t = flat[torch.from_numpy(idx).to(flat.device)]
        a = t.to(dt).cpu().numpy()
        left -= a.nbytes
        np.save(os.path.join(path, name + '.npy'), a)


def run_rank(args):
    import numpy as np
    import torch
    import torch.distributed as dist

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        raise SystemExit('WORLD_SIZE=%d but --gpus %d' % (world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a GPU: the inference path has no CPU fallback')
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    dist_on = world > 1 or os.environ.get('WSI_FORCE_COLLECTIVE') == '1'      # (the latter: RCCL path rehearsal on one GPU)
    if dist_on:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29533')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)      # "nccl" is RCCL on ROCm

    from wsi_segmentation_pipeline_amd import native, slide as S
    from wsi_segmentation_pipeline_amd.engine import TrunkEngine, PARITY, SPEED, MX
    from wsi_segmentation_pipeline_amd import synthetic as W   # seeded checkpoint (no trained one exists offline)

    planes = {'parity': PARITY, 'mx': MX, 'speed': SPEED}[args.mode]
    lib = native.load()
    if args.chunks:
        cs, c1 = (int(v) for v in args.chunks.split(','))
        native.check(lib.wsi_trunk_set_chunks(cs, c1), 'wsi_trunk_set_chunks')
    if args.stem:
        f, r = (int(v) for v in args.stem.split(','))
        native.check(lib.wsi_stem_set_mode(f, r), 'wsi_stem_set_mode')
    if args.s2 >= 0:
        native.check(lib.wsi_conv_set_mode(args.s2), 'wsi_conv_set_mode')

    def fence():
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
            torch.cuda.synchronize()

    # ------------------------------------------------------------------------------- workload set-up
    if args.workload == 'seg':
        # the dense path of predict_tumorbed(mode='seg') / predict_wsis (reference utils/eval.py:51,199-200; eval_tumorbed.py:21-28):
        # tiles read from an HBM-resident u8 slide -> (N, 4, 256, 256) logits; each rank runs its own --seg-tiles tiles (weak scaling)
        from wsi_segmentation_pipeline_amd.unet import UNetEngine
        usd = W.make_unet_state_dict(5, classes=4)
        # the seeded decoder ends in |logit| ~ 216 (softmax saturated everywhere); the 1e-3 contract is stated on logits of the
        # size trained heads produce, so the final 1x1 conv is scaled by 8/216: max |logit| ~ 16 on the bench tiles, the magnitude of the
        # hot margin families
        for key in ('decoder.final_conv.weight', 'decoder.final_conv.bias'):
            usd[key] = usd[key] * (8.0 / 216.0)
        eng = UNetEngine(usd, dev, planes=planes, max_batch=args.seg_batch)
        eng._streams = []
        side = int(np.ceil(np.sqrt(args.seg_tiles)))
        gseg = torch.Generator(device=dev).manual_seed(1 + rank)
        level0 = torch.randint(0, 256, (side * TILE, side * TILE, 3), dtype=torch.uint8, device=dev, generator=gseg)
        sxy = torch.tensor([[TILE * (i % side), TILE * (i // side)] for i in range(args.seg_tiles)], dtype=torch.int32, device=dev)

        def step():
            return {'seg_logits': eng.forward_tiles(level0, sxy, TILE, TILE)}
        units_per_step = args.seg_tiles * world
        unit = 'patches/s'
        metric = "patches/sec (256x256x3) dense U-Net segmentation, predict_tumorbed(mode='seg') inner loop (the reference's default eval mode)"
        workload_desc = ('seg: %d tiles of 256x256 per rank from an HBM-resident u8 slide, ResNet-18 encoder + smp-style U-Net decoder '
                         '(5 blocks, channels 256/128/64/32/16) + 1x1 head -> (N, 4, 256, 256) fp32 logits, batches of %d' % (args.seg_tiles, args.seg_batch))
        scaling, parallelism, tiles_total = 'weak', 'independent tiles x%d (no collective in the timed region)' % world, units_per_step
        args.batch = args.seg_batch
    elif args.workload == 'cfg4':
        from wsi_segmentation_pipeline_amd import bags as B
        sd = W.make_resnet18_state_dict(11, with_fc=True)
        eng = TrunkEngine(sd, dev, planes=planes, head=(sd['fc0.weight'], sd['fc0.bias']), max_batch=args.batch * 16)
        wl = B.BagWorkload(eng, sd, args.regions, seed=4, device=dev, rank=rank, world=world)
        units_per_step = wl.total_crops
        step = wl.step
        unit, metric = 'crops/s', 'crops/sec (64x64x3, 16-crop region bags, ensemble head) region-proposal inference (BASELINE configs[3])'
        workload_desc = ('cfg4: %d region bags x 16 crops of 64x64, ResNet-18 bag forward (fc0 per crop + fc 8192->4096->4 per bag), '
                         'bags sharded by count over %d rank(s), ensemble logits gathered' % (args.regions, world))
        scaling = 'strong'
        parallelism = 'bag-shard x%d + 1 all-gather' % world
        tiles_total = units_per_step
    else:
        sd = W.make_resnet18_state_dict(11, with_fc=False)
        cls = W.make_head_state_dict(22, 'classifier')
        eng = TrunkEngine(sd, dev, planes=planes, head=(cls['fc.0.weight'], cls['fc.0.bias']), max_batch=args.batch,
                          streams=args.streams)
        if args.workload in ('cfg3', 'cfg5'):
            iw = ih = args.size
            tiles = S.tile_grid(iw, ih, TILE, TILE, TILE, TILE)
            total_tiles = len(tiles)
            scaling = 'strong'
        else:
            total_tiles = args.tiles * world
            iw, ih = slide_geometry_cfg2(total_tiles)
            tiles = S.tile_grid(iw, ih, TILE, TILE, TILE, TILE)[:total_tiles]
            assert len(tiles) == total_tiles, (len(tiles), total_tiles)
            scaling = 'weak'
        # this rank's share of the slide: only the rectangles its own tiles touch are generated and kept in HBM
        lo, hi = S.shard_range(total_tiles, rank, world)
        src = S.SyntheticRows(iw, ih, 3, dev)
        rects, atlas_hw, local_xy = S.region_plan(tiles[lo:hi], TILE, TILE)
        level0 = S.resident_regions(src, rects, atlas_hw, dev)
        resident_gb = level0.numel() / 1e9
        m = 1.0 / 16.0                                       # downsample[0] / downsample[2]
        map_hw = (ih // 16, iw // 16)
        mask = torch.ones(map_hw, dtype=torch.uint8, device=dev)
        class_probs = (0., 0., 0., 0.)

        def step():
            return S.infer_slide_cls(eng, level0, tiles, TILE, TILE, m, map_hw, 4, class_probs, mask, rank, world,
                                     want_probs=False, local_xy=local_xy)
        if args.workload == 'cfg5':
            # BASELINE configs[4]: tumour-bed evaluation = the cfg3 slide pass + the post-process on the full stitched map
            # (paper_tools/overlay_tb_wsi.py:46-64: threshold -> open 30x30 -> convex hull -> perimeter -> dilate 20x20;
            # contour_ordering esp over the hull; utils/eval.py:104 IoU against a ground-truth bed), all on the device.
            # Random weights give a flat heat map (class-1 probability rounds to code 0 almost everywhere), so the binary input
            # of the post-process is built from the stitched map itself - the pixels whose class-1 logit sum lies above the map's
            # 0.95 quantile (tile-sized speckle of 16 x 16 map pixels on ~5 % of the tiles: isolated tiles, the rare pairs and the
            # 12-pixel-wide overlap strips of the edge column / row are all narrower than the 30 x 30 opening and vanish in it; the
            # r03 bench thresholded at the MEDIAN, whose blobs of neighbouring tiles survived the opening, so the hull was the
            # whole map: IoU 0.39, 16 vertices) - united with a disc of radius 0.30 H that survives the opening; the
            # ground-truth bed is the concentric disc of radius 0.35 H, so IoU of the hulls ~ (0.30 / 0.35)^2 = 0.73.
            from wsi_segmentation_pipeline_amd import postprocess as PP
            slide_step = step
            yy, xx = torch.meshgrid(torch.arange(map_hw[0], device=dev), torch.arange(map_hw[1], device=dev), indexing='ij')
            r2 = (yy - map_hw[0] / 2) ** 2 + (xx - map_hw[1] / 2) ** 2
            tb_gt = (r2 <= (0.35 * map_hw[0]) ** 2).to(torch.uint8)
            seed_disc = r2 <= (0.30 * map_hw[0]) ** 2
            state = {}

            def postprocess(r):
                if 'thr' not in state:
                    state['thr'] = float(torch.quantile(r['pred'][1].flatten()[::7].float(), 0.95).item())
                codes = ((r['pred'][1] > state['thr']) | seed_disc).to(torch.uint8)
                tb = PP.tumor_bed(codes, 1, 30, 20)
                return codes, tb, tb.outline_points(64), PP.mask_iou(tb_gt, tb.tb_pred)

            def step():
                r = slide_step()
                r['codes'], r['tumor_bed'], r['outline_points'], r['tb_iou'] = postprocess(r)
                return r
        units_per_step = total_tiles
        unit, metric = 'patches/s', METRIC
        if args.workload in ('cfg3', 'cfg5'):
            workload_desc = ('%s: ONE %dx%d synthetic slide, tile 256 stride 256 -> %d tiles sharded over %d rank(s) (each holds '
                             'only its own slide regions: %.2f GB on rank 0), ResNet-18 trunk + Classifier, fused read+normalise+conv HIP '
                             'path, 1 all-gather, float64 stitch + softmax%s' % (args.workload, iw, ih, total_tiles, world, resident_gb,
                              ' + tumour-bed post-process on the 2500x2500 map (threshold, open 30x30, convex hull, perimeter, dilate 20x20, esp, IoU)' if args.workload == 'cfg5' else ''))
        else:
            workload_desc = ('cfg2: ResNet-18 trunk + Classifier, %d-tile slide per GPU, tile 256 stride 256, '
                             'fused read+normalise+conv HIP path, float64 stitch + softmax' % args.tiles)
        parallelism = 'tile-shard x%d + 1 all-gather' % world
        tiles_total = total_tiles

    # ------------------------------------------------------------------------------- timed region
    for _ in range(args.warmup):
        step()
    fence()
    prof_on = args.full and not args.no_prof
    per_rank_units = (units_per_step + world - 1) // world
    nb = max(1, -(-per_rank_units // (args.batch * (16 if args.workload == 'cfg4' else 1))))
    launches_per_step = (64 if args.workload == 'seg' else 24) * nb
    if args.chunks:                                         # sub-batched stem / layer 1: one stem launch per stem chunk, four convs per layer-1 chunk
        cs_, c1_ = (int(v) for v in args.chunks.split(','))
        per = min(args.batch, per_rank_units)
        launches_per_step = nb * (16 + (-(-per // cs_) if cs_ else 1) + 4 * (-(-per // c1_) if c1_ else 1) + (-(-per // c1_) if c1_ and cs_ else 0))
    # The cyclic garbage collector is switched off for the timed region, as `timeit` does: r05 found a generation-2 collection of
    # ~45 ms (the tile lists and bag index lists are millions of Python objects) landing INSIDE the five timed steps of cfg4 whenever
    # the import graph grew by a module - 1.52 M crops/s measured as 1.24 M, with identical kernels and an identical GPU timeline
    # (tools/cfg4_steps.py, profiles/r05_bench_gc_pause.txt).  WSI_BENCH_GC=on keeps it running.
    import gc
    gc_off = os.environ.get('WSI_BENCH_GC') != 'on'
    if gc_off:
        gc.collect()
        gc.disable()
    t0 = time.perf_counter()
    step_marks = []                                         # WSI_BENCH_STEP_TIMES=1: host time at which each step's enqueue returned (diagnosis)
    for _ in range(args.steps):
        out = step()
        step_marks.append(time.perf_counter() - t0)
    fence()
    dt = time.perf_counter() - t0
    if gc_off:
        gc.enable()
    if args.dump_outputs and rank == 0:                     # before any leg below runs the engine again
        dump_outputs(out, args.dump_outputs)
    if os.environ.get('WSI_BENCH_STEP_TIMES') == '1' and rank == 0:
        print('step enqueue returns (ms): %s | fence %.1f' % (' '.join('%.1f' % (m * 1e3) for m in step_marks), dt * 1e3), file=sys.stderr)
    # Per-kernel leg (roofline objects): the SAME steps once more, right after the timed region, with ONE batch in flight and HIP
    # events on the launch stream around every conv / stem launch (wsi_prof_begin/_end).  r01-r03 took these events inside the
    # timed region and therefore benchmarked one batch in flight; two in flight are ~3 % faster, and their overlapping launches
    # would make per-kernel event times meaningless.  `kernels.*.share_of_step` refers to this pass's own wall time.
    per_kind, prof_dt = {}, None
    if prof_on and launches_per_step * args.steps <= 16384:
        saved_streams = eng._streams
        eng._streams = []
        native.check(lib.wsi_prof_begin(launches_per_step * args.steps), 'wsi_prof_begin')
        p0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        fence()
        prof_dt = time.perf_counter() - p0
        per_kind = collect_prof(lib, np, launches_per_step * args.steps, prof_dt)
        eng._streams = saved_streams
    else:
        prof_on = False
    if dist_on:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    value = units_per_step * args.steps / dt

    # ------------------------------------------------------------------------------- roofline objects (rank 0's kernels)
    eff_batch = -(-per_rank_units // nb) if args.workload not in ('cfg4', 'seg') else None
    roofline = roofline_l1 = roofline_bf16 = roofline_stem = None
    prof_tag = os.environ.get('WSI_TRAFFIC_JSON', '')
    tj = None
    for cand in ([prof_tag] if prof_tag else []) + [os.path.join(ROOT, 'profiles', f) for f in
                                                    ({3: ['r05_traffic_mx.json', 'r04_traffic_mx.json', 'r03_traffic_mx.json'], 2: ['r02_traffic.json', 'r01_traffic.json']}.get(planes, []))]:
        if cand and os.path.exists(cand):
            tj, tpath = json.load(open(cand)), cand
            break

    def pmc_bytes(substr, batch):
        # HBM bytes per launch from the committed PMC passes (tools/collect_traffic.sh: FETCH_SIZE x2 + WRITE_SIZE; r04: collected
        # at this command's own batch, r01-r03 at a cap of 1000), scaled by this run's tiles per launch / the collection's
        if not tj or batch is None:
            return None
        subs = (substr,) if isinstance(substr, str) else substr
        sel = [v for k, v in tj['kernels'].items() if any(x in k for x in subs)]
        if not sel:
            return None
        return round(sum(v['hbm_bytes_per_launch'] * v['launches'] for v in sel) / sum(v['launches'] for v in sel) * batch / float(tj.get('batch', 1000)))

    passes = {2: '6 fp16 K=16 per 32-channel step', 3: '2 fp16 K=16 + 1 MX-fp6 K=64 per 32-channel step', 1: '2 bf16 K=16 per 32-channel step'}
    if 'conv3x3_s1' in per_kind:
        k = per_kind['conv3x3_s1']
        # Dominant kernel = the stride-1 3x3 conv of layers 2-4 (9 launches per batch); algorithmic FLOPs = 2*M*N*K over
        # real output pixels (302 MFLOP per conv and 256x256 patch); split passes are not counted
        roofline = {'kernel': 'stride-1 3x3 convs of layers 2-4, 9 launches per batch: ' + {3: 'conv3x3s1_wide_kernel', 2: 'conv3x3s1_pp_kernel (layers 3-4) + conv3x3s1_slab3_kernel (layer 2)',
                                                                                             1: 'conv3x3s1_wide_kernel (layers 2-3) + conv3x3s1_pp_kernel (layer 4)'}[planes],
                    'bound': 'mfma', 'achieved': round(k['tflops'], 2), 'peak': PEAK_BF16_TFLOPS, 'unit': 'TFLOP/s',
                    'frac': round(k['tflops'] / PEAK_BF16_TFLOPS, 4),
                    'traffic': pmc_bytes(('conv3x3s1_wide', 'conv3x3s1_pp'), eff_batch),
                    'traffic_unit': 'HBM bytes per launch (PMC FETCH_SIZE x2 + WRITE_SIZE)',
                    'traffic_source': ('%s: rocprofv3 --pmc passes of this command (separate runs, one batch in flight) at %s tiles per launch, scaled to this run\'s %d' %
                                       (os.path.relpath(tpath, ROOT), ('%.0f' % tj['batch']) if 'batch' in tj else '1000', eff_batch or 0)) if tj else 'not collected for this mode',
                    'avg_launch_ms': round(k['avg_ms'], 4), 'mfma_passes': passes[planes], 'precision_mode': args.mode}
    l1 = per_kind.get('conv3x3_s1_layer1')
    if l1 and eff_batch:
        bpc = 2 if planes == 1 else 4
        tensor = eff_batch * 64 * 64 * 64 * bpc
        # algorithmic bytes per launch: input + output (+ residual on every second launch) = 2.5 tensors on average.
        # r03, mx: stem output and layer-1 tensors are stored in 96-byte lines (3 of the 4 bytes per channel),
        # except the last conv's output: (4 inputs + 3 outputs + 2 residuals) x 0.75 + 1 output = 7.75 tensors over 4 launches
        lines96 = planes == MX and not (args.s2 >= 0 and args.s2 & 16384)
        alg = (7.75 / 4 if lines96 else 2.5) * tensor
        gbs = alg / (l1['avg_ms'] * 1e-3) / 1e9
        l1_names = ('conv3x3s1_rows_kernel', 'conv3x3s1_slab3_kernel<4, 2, 2')
        l1_sel = [v for k_, v in tj['kernels'].items() if any(x in k_ for x in l1_names)] if tj else []
        sc = eff_batch / float(tj.get('batch', 1000)) if tj else 0.0
        traffic_l1 = None
        if not lines96:
            traffic_l1 = pmc_bytes(l1_names, eff_batch)
        elif l1_sel and all('hbm_bytes_per_launch_calibrated96' in v for v in l1_sel):
            # 96-byte lines: FETCH_SIZE calibrated per access pattern (slab x0.972, residual tiles x0.5: tools/probes/fetch_calib96,
            # tools/traffic_json.py), WRITE_SIZE exact
            nl = sum(v['launches'] for v in l1_sel)
            traffic_l1 = round(sum(v['hbm_bytes_per_launch_calibrated96'] * v['launches'] for v in l1_sel) / nl * sc)
        roofline_l1 = {'kernel': 'conv3x3s1_rows_kernel (4 launches per batch: the 64-channel layer 1 on 64-wide maps; line-planar 96-byte lines since r05)', 'bound': 'hbm',
                       'achieved': round(gbs, 1), 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'frac': round(gbs / PEAK_HBM_GBS, 4),
                       'traffic': traffic_l1,
                       'algorithmic_bytes_per_launch': round(alg), 'line_bytes': 96 if lines96 else 128,
                       'avg_launch_ms': round(l1['avg_ms'], 4), 'tflops': round(l1['tflops'], 2)}
        if lines96 and l1_sel:
            nl = sum(v['launches'] for v in l1_sel)
            roofline_l1['traffic_parts'] = {
                'write_bytes_per_launch': round(sum(v['write_bytes_per_launch'] * v['launches'] for v in l1_sel) / nl * sc),
                'fetch_size_raw_bytes_per_launch': round(sum(v['read_bytes_per_launch'] * v['launches'] for v in l1_sel) / nl * sc / 2),
                'note': ('96-byte lines are line-planar since r05: contiguous reads, FETCH_SIZE follows the x2 rule for the slab and the residual-tile '
                         'pattern alike (tools/probes/fetch_calib96 kplanar: x0.500, profiles/r05_fetch_calib96.txt; r03-r04, lines interleaved per pixel: x0.945 / x0.5)') if traffic_l1 else
                        'FETCH_SIZE uncalibrated for 96-byte-line reads (x1.03 .. x2): no total; algorithmic reads are 59 % of the algorithmic bytes'}

    # stem (tile read + transform + conv7x7 + BN + ReLU + maxpool, one launch per batch): HBM-side roofline.  Algorithmic bytes per tile =
    # the tile's u8 pixels in (256 x 256 x 3) + the pooled 64 x 64 x 64 map out (3 bytes per channel in mx's 96-byte lines, 4 in 128-byte
    # lines, 2 in single-pass bf16).  The kernel is VALU-bound: the PMC read-out says how far from the byte floor.
    roofline_stem = None
    st_k = per_kind.get('stem_maxpool')
    if st_k and eff_batch:
        lines96_s = planes == MX and not (args.s2 >= 0 and args.s2 & 16384)
        alg_s = eff_batch * (TILE * TILE * 3 + 64 * 64 * 64 * (3 if lines96_s else 2 if planes == 1 else 4))
        gbs_s = alg_s / (st_k['avg_ms'] * 1e-3) / 1e9
        roofline_stem = {'kernel': 'stem_pool_kernel (1 launch per batch: u8 tile read + ToTensor / Normalize folded into integer weights + conv7x7 s2 + BN + ReLU + maxpool 3x3 s2)',
                         'bound': 'hbm', 'achieved': round(gbs_s, 1), 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'frac': round(gbs_s / PEAK_HBM_GBS, 4),
                         'traffic': pmc_bytes('stem_pool', eff_batch), 'algorithmic_bytes_per_launch': round(alg_s),
                         'avg_launch_ms': round(st_k['avg_ms'], 4), 'share_of_step': st_k['share_of_step'],
                         'limiter': 'VALU: ~10 vector instructions per i8 MFMA, matrix pipe ~0.43 busy (profiles/r05_pmc/trunk_kernels_counters.txt); '
                                    'times over the byte floor at the achievable 6.3 TB/s: %.1f' % (st_k['avg_ms'] * 1e-3 / (alg_s / 6.3e12))}

    # the same dominant kernel in single-pass bf16 (the literal dtype of BASELINE configs[1]; logit error ~2e-2, outside the
    # contract, so never the headline): one profiled pass on rank 0, outside the timed region
    if rank == 0 and prof_on and not args.no_bf16_leg and planes != SPEED and args.workload not in ('cfg4', 'seg'):
        eng.release_workspaces()                               # two batches in flight = two workspaces (~51 GB each): the legs below need the room
        eng1 = TrunkEngine(sd, dev, planes=SPEED, head=(cls['fc.0.weight'], cls['fc.0.bias']), max_batch=args.batch)
        nsub = min(hi - lo, 2 * args.batch)
        sub = torch.from_numpy(np.ascontiguousarray(local_xy[:nsub])).to(dev)
        eng1.forward_tiles(level0, sub, TILE, TILE, logits=True)
        torch.cuda.synchronize()
        native.check(lib.wsi_prof_begin(256), 'wsi_prof_begin')
        for _ in range(3):
            eng1.forward_tiles(level0, sub, TILE, TILE, logits=True)
        torch.cuda.synchronize()
        k1 = collect_prof(lib, np, 256, 0.0).get('conv3x3_s1')
        if k1:
            roofline_bf16 = {'kernel': 'stride-1 3x3 conv of layers 2-4, single-pass bf16 (precision mode "speed")', 'bound': 'mfma',
                             'achieved': round(k1['tflops'], 2), 'peak': PEAK_BF16_TFLOPS, 'unit': 'TFLOP/s',
                             'frac': round(k1['tflops'] / PEAK_BF16_TFLOPS, 4), 'avg_launch_ms': round(k1['avg_ms'], 4),
                             'batch': -(-nsub // max(1, -(-nsub // args.batch))), 'timed': 'outside the timed region (3 passes over %d tiles)' % nsub}
        eng1.release_workspaces()
        del eng1

    # ------------------------------------------------------------------------------- CPU baseline (rank 0, N = 1)
    cpu_baseline = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline and args.workload not in ('cfg4', 'seg'):
        from oracle import resnet_oracle as R                 # the checker, never the thing measured above
        avail = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
        res = {}
        with torch.no_grad():
            phys = avail // 2 if avail >= 64 else avail        # the pool's hosts show two hardware threads per core
            legs = [(1, 32), (min(16, avail), 128)] + ([(phys, 512)] if phys > 16 else [])      # 1-3 s per pass, 4 passes each
            for cores, nsample in legs:
                lxy = local_xy[:nsample]                                       # the same first tiles, read from the resident atlas
                u8 = torch.stack([level0[y:y + TILE, x:x + TILE] for x, y in lxy]).permute(0, 3, 1, 2).contiguous().cpu().numpy()
                torch.set_num_threads(cores)
                ref = R.tile_logits(sd, cls, u8)                               # warm-up (also the sanity reference)
                ts = []
                for _ in range(3):
                    c0 = time.perf_counter()
                    R.tile_logits(sd, cls, u8)
                    ts.append(time.perf_counter() - c0)
                res[cores] = (nsample / float(np.median(ts)), nsample, ref)
        many = max(res, key=lambda c: res[c][0])               # the fastest leg is the baseline; every leg is listed
        big = max(res, key=lambda c: res[c][1])
        got = out['logits'][:res[big][1]].cpu()
        oracle_sample = (res[big][2], res[big][1])
        cpu_baseline = {'value': round(res[many][0], 2), 'unit': 'patches/s', 'cores': many, 'kind': 'port',
                        'sample': 'first %d tiles of the same slide, fp32 torch CPU oracle (oracle/resnet_oracle.py), 1 warm-up + median of 3' % res[many][1],
                        'legs': [{'cores': c, 'value': round(res[c][0], 2), 'sample': 'first %d tiles' % res[c][1]} for c in sorted(res)],
                        'single_thread': {'value': round(res[1][0], 2), 'cores': 1, 'sample': 'first %d tiles' % res[1][1]},
                        'host_threads_available': avail, 'physical_cores_assumed': phys,
                        'max_abs_logit_diff_vs_gpu': float((got - res[big][2]).abs().max())}

    # ------------------------------------------------------------------------------- the contract this line was measured under
    # (1e-3 on the logits against the fp32 reference path): this run's own check against the CPU oracle on the baseline
    # sample, the worst case over the reference-generated margin families (profiles/r03_margin_families.json, written from
    # tests/test_gpu_margin.py's output), and - when the headline mode is not `parity` - a parity-mode leg of the same step,
    # timed after the timed region
    contract = parity_leg = None
    if rank == 0 and args.full and args.workload not in ('cfg4', 'seg'):
        fam = None
        fpath = next((q for q in (os.path.join(ROOT, 'profiles', f) for f in ('r05_margin_families.json', 'r04_margin_families.json', 'r03_margin_families.json')) if os.path.exists(q)),
                     os.path.join(ROOT, 'profiles', 'r05_margin_families.json'))
        if os.path.exists(fpath):
            fam = json.load(open(fpath))
        contract = {'mode': args.mode, 'tolerance': 1e-3,
                    'max_abs_logit_diff_vs_oracle': cpu_baseline['max_abs_logit_diff_vs_gpu'] if cpu_baseline else None,
                    'oracle_sample_tiles': oracle_sample[1] if cpu_baseline else None,
                    'families_max': (fam or {}).get(args.mode), 'families_source': os.path.relpath(fpath, ROOT) if fam else None}
    if rank == 0 and world == 1 and args.full and planes != PARITY and not args.no_parity_leg and args.workload in ('cfg2', 'cfg3'):
        eng.release_workspaces()
        engp = TrunkEngine(sd, dev, planes=PARITY, head=(cls['fc.0.weight'], cls['fc.0.bias']), max_batch=args.batch, streams=args.streams)

        def pstep():
            return S.infer_slide_cls(engp, level0, tiles, TILE, TILE, m, map_hw, 4, class_probs, mask, rank, world,
                                     want_probs=False, local_xy=local_xy)
        outp = pstep()
        torch.cuda.synchronize()
        p0 = time.perf_counter()
        for _ in range(2):
            outp = pstep()
        torch.cuda.synchronize()
        pdt = (time.perf_counter() - p0) / 2
        parity_leg = {'mode': 'parity', 'value': round(units_per_step / pdt, 1), 'unit': unit, 'ms_per_step': round(pdt * 1e3, 3),
                      'steps': 2, 'timed': 'after the timed region, same slide and batch',
                      'max_abs_logit_diff_vs_oracle': float((outp['logits'][:oracle_sample[1]].cpu() - oracle_sample[0]).abs().max()) if cpu_baseline else None,
                      'max_abs_logit_diff_vs_headline_mode': float((outp['logits'] - out['logits']).abs().max())}
        engp.release_workspaces()
        del engp

    # ------------------------------------------------------------------------------- what a reference-side caller gets
    # north_star: "behind the existing models.models / utils.eval API".  The timed region above drives slide.infer_slide_cls with a
    # hand-built engine; this leg runs the SAME slide through the reference-named modules exactly as eval_tumorbed.py would
    # (/root/reference/eval_tumorbed.py:44-48, utils/eval.py:155-286): resnets_shift.resnet18 + models.models.Classifier,
    # a utils.dataset.Dataset_wsis over the slide, utils.eval.predict_tumorbed(model, dataset, ep, mode='cls') - every default
    # left alone (precision='auto': per-slide probe; batch and streams: the engine's own sizing).  Timed after the timed region.
    api = None
    if rank == 0 and world == 1 and args.full and args.workload == 'cfg3' and not args.no_api_leg:
        import tempfile
        import myargs
        import resnets_shift
        import utils.dataset as UD
        import utils.eval as UE
        from models.models import Classifier
        from PIL import Image
        # the bare engine under the SAME conditions as the API calls below - one slide per call, a host synchronisation after each, this
        # late in the run (clocks settle lower than in the timed region, and back-to-back steps of the timed region overlap at their ends)
        ts_ref = []
        for rep in range(4):
            torch.cuda.synchronize()
            r0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            ts_ref.append(time.perf_counter() - r0)
        t_ref = float(np.median(ts_ref[1:]))
        # The API's own engines plan their own 2 x 51 GB beside the timed region's: releasing those first and re-allocating costs the API
        # engine 3 % (218.6 against 212.3 ms for the same 24 648 tiles; a first allocation in a fresh process: 207.6 - where its workspaces
        # land in HBM matters, profiles/r05_api_breakdown.txt), so they are only released when the memory is needed
        if torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev) < 130e9:
            eng.release_workspaces()
            torch.cuda.empty_cache()
        net = resnets_shift.resnet18(False)                  # precision='auto' is the constructor default
        net.load_state_dict(sd, strict=False)                # (the seeded checkpoint has no bag-head keys: fc / fc1 / fc2 stay as initialised, unused here)
        head = Classifier(512, 4)
        head.load_state_dict(cls)
        model = UE.SlideClassifierModel(net, head).to(dev).eval()
        full = level0 if tuple(level0.shape[:2]) == (ih, iw) and np.array_equal(np.asarray(local_xy), np.asarray(tiles)) else src.full()
        ma = myargs.args
        saved = {k: getattr(ma, k) for k in ('scan_level', 'scan_resize', 'num_classes', 'class_probs', 'tile_w', 'tile_h', 'tile_stride_w',
                                             'tile_stride_h', 'wsi_mask_pth', 'val_save_pth')}
        with tempfile.TemporaryDirectory() as td:
            ma.scan_level, ma.scan_resize, ma.num_classes, ma.class_probs = 0, 1, 4, [0., 0., 0., 0.]
            ma.tile_w = ma.tile_h = ma.tile_stride_w = ma.tile_stride_h = TILE
            ma.wsi_mask_pth, ma.val_save_pth = td, os.path.join(td, 'out')
            Image.fromarray(np.ones(map_hw, np.uint8)).save(os.path.join(td, 'bench.svs.png'))          # "no mask": everything is foreground (0 / 1, as find_nuclei returns it)

            def make_dataset():
                sl = S.ArraySlide([full, np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8)], [1.0, 4.0, 16.0])
                sl.level_dimensions = ((iw, ih), (iw // 4, ih // 4), (iw // 16, ih // 16))
                sl.name = 'bench.svs'
                return UD.Dataset_wsis({'bench.svs': sl}, {'ph': TILE, 'pw': TILE, 'sh': TILE, 'sw': TILE}, bs=ma.batch_size)
            dsw = make_dataset()
            n_api = len(dsw.wsis['bench.svs']['iterator'].dataset)
            res = UE.predict_tumorbed(model, dsw, 0, mode='cls', save=False)['bench.svs']      # warm-up (plans the workspaces)
            torch.cuda.synchronize()
            ts, ts_png = [], []
            marks = []
            if os.environ.get('WSI_API_MARKS') == '1':             # diagnosis: synchronised stopwatch inside the call (tools/api_breakdown.py)
                orig_infer = S.infer_slide_cls

                def mark(name):
                    torch.cuda.synchronize()
                    marks.append((name, time.perf_counter()))

                def timed_infer(e_, *a_, **k_):
                    mark('enter infer')
                    mxf, parf = e_._mx.forward_tiles, e_._par.forward_tiles
                    e_._mx.forward_tiles = lambda *x, **y: (mxf(*x, **y), mark('mx done'))[0]
                    e_._par.forward_tiles = lambda *x, **y: (parf(*x, **y), mark('parity sample done'))[0]
                    try:
                        r_ = orig_infer(e_, *a_, **k_)
                    finally:
                        e_._mx.forward_tiles, e_._par.forward_tiles = mxf, parf
                    mark('leave infer')
                    return r_
                UE.S.infer_slide_cls = timed_infer
            for rep in range(3):
                dsw = make_dataset()
                torch.cuda.synchronize()
                a0 = time.perf_counter()
                marks[:] = [('start', a0)]
                res = UE.predict_tumorbed(model, dsw, 0, mode='cls', save=False)['bench.svs']
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - a0)
                if len(marks) > 1:
                    marks.append(('end', time.perf_counter()))
                    print('api rep %d: ' % rep + ' | '.join('%s +%.2f' % (marks[i][0], (marks[i][1] - marks[i - 1][1]) * 1e3) for i in range(1, len(marks))), file=sys.stderr)
            if os.environ.get('WSI_API_MARKS') == '1':
                UE.S.infer_slide_cls = orig_infer
            dsw = make_dataset()
            a0 = time.perf_counter()
            UE.predict_tumorbed(model, dsw, 0, mode='cls')                                       # save=True: + heat-map and overlay PNGs, as the reference writes them
            torch.cuda.synchronize()
            t_png = time.perf_counter() - a0
        for k, v in saved.items():
            setattr(ma, k, v)
        t_api = float(np.median(ts))
        api_eng = net.hip_engine(dev)
        inner = getattr(api_eng, '_chosen', None) or api_eng
        same = bool(np.array_equal(res['heatmap'], out['heatmap'].cpu().numpy())) if res['precision'] and res['precision'].get('mode') == args.mode else None
        api = {'value': round(n_api / t_api, 1), 'unit': unit, 'ms_per_slide': round(t_api * 1e3, 3), 'tiles': n_api,
               'vs_headline': round(n_api / t_api / value, 4),
               'bare_engine_one_slide_per_call': {'value': round(n_api / t_ref, 1), 'ms_per_slide': round(t_ref * 1e3, 3),
                                                  'note': 'slide.infer_slide_cls on the hand-built engine of the timed region, one call + one synchronisation per slide, '
                                                          'measured right before the API calls (median of 3 after one warm-up)'},
               'vs_bare_engine_one_slide_per_call': round(t_ref / t_api, 4),
               'call': "utils.eval.predict_tumorbed(SlideClassifierModel(resnets_shift.resnet18(), models.models.Classifier(512, 4)), utils.dataset.Dataset_wsis(...), ep, mode='cls', save=False)",
               'precision': res['precision'], 'engine_defaults': {'batches_in_flight': max(1, len(getattr(inner, '_streams', []))),
                                                                  'batch_cap': inner._auto_cap(TILE, TILE) if hasattr(inner, '_auto_cap') else None},
               'timed': 'after the timed region: median of 3 calls after one warm-up call; includes the per-slide two-mode probe, mask upload, stitch, softmax, u8 maps to the host',
               'with_png_write': {'value': round(n_api / t_png, 1), 'ms_per_slide': round(t_png * 1e3, 3),
                                  'note': 'save=True (the reference default): + the heat-map and overlay PNG files of the 2500 x 2500 map, host-side PIL'},
               'heatmap_equals_timed_region': same}
        del model, net, head
        torch.cuda.empty_cache()

    if rank == 0 and world == 1 and args.full and args.workload == 'seg' and not args.no_api_leg:
        # The dense path through the reference-named API: utils.eval.predict_tumorbed(model, dataset, ep, mode='seg') with the model a
        # UNetSeg (the smp.Unet drop-in) over a utils.dataset.Dataset_wsis of the SAME slide (/root/reference/utils/eval.py:196-215).
        # r05: that call takes the engine's fused tile path (utils.eval._dense_batches); `generic_iterator_path` times the loop the
        # reference writes - model.decoder(model.encoder(batch_image)) over the iterator's batches of myargs.batch_size tiles - on the
        # same kernels, by hiding the model's type from the dispatch.
        import tempfile
        import myargs
        import utils.dataset as UD
        import utils.eval as UE
        from PIL import Image
        from wsi_segmentation_pipeline_amd.unet import UNetSeg
        ts_ref = []
        for rep in range(4):
            torch.cuda.synchronize()
            r0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            ts_ref.append(time.perf_counter() - r0)
        t_ref = float(np.median(ts_ref[1:]))
        # ... and the bare engine followed by the stages the API call adds behind it, written out by hand: float64 map, dense stitch,
        # exponent-span guard, softmax + threshold + arg-max with a device-resident mask, both u8 maps to the host
        from wsi_segmentation_pipeline_amd import engine as EN
        n_side = side * TILE
        mask_dev = torch.ones((n_side, n_side), dtype=torch.uint8, device=dev)

        def bare_pipeline():
            pred_ = torch.zeros((4, n_side, n_side), dtype=torch.float64, device=dev)
            lg_ = eng.forward_tiles(level0, sxy, TILE, TILE)
            EN.stitch_add_dense(pred_, lg_, sxy)
            EN.exponent_span(lg_)
            cls_, _, heat_ = EN.softmax_threshold_argmax(pred_, [0., 0., 0., 0.], mask_dev, 'seg', want_probs=False)
            return UE._to_host(heat_, cls_)
        ts_pipe = []
        for rep in range(4):
            torch.cuda.synchronize()
            r0 = time.perf_counter()
            bare_pipeline()
            torch.cuda.synchronize()
            ts_pipe.append(time.perf_counter() - r0)
        t_pipe = float(np.median(ts_pipe[1:]))
        del mask_dev
        model = UNetSeg(4, precision=args.mode)
        model.load_state_dict(usd)
        model = model.to(dev).eval()
        model.hip_engine(dev).max_batch = args.seg_batch

        class _Opaque(torch.nn.Module):                      # same kernels, but not a UNetSeg: the generic iterator loop
            def __init__(self, u):
                super().__init__()
                self.encoder, self.decoder = u.encoder, u.decoder
        ma = myargs.args
        saved = {k: getattr(ma, k) for k in ('scan_level', 'scan_resize', 'num_classes', 'class_probs', 'tile_w', 'tile_h', 'tile_stride_w',
                                             'tile_stride_h', 'wsi_mask_pth', 'val_save_pth')}
        with tempfile.TemporaryDirectory() as td:
            ma.scan_level, ma.scan_resize, ma.num_classes, ma.class_probs = 0, 1, 4, [0., 0., 0., 0.]
            ma.tile_w = ma.tile_h = ma.tile_stride_w = ma.tile_stride_h = TILE
            ma.wsi_mask_pth, ma.val_save_pth = td, os.path.join(td, 'out')
            Image.fromarray(np.ones((n_side, n_side), np.uint8)).save(os.path.join(td, 'bench.svs.png'))

            def make_dataset():
                sl = S.ArraySlide([level0], [1.0])           # one level: the map is stitched at the scan level (m = 1)
                sl.level_dimensions = ((n_side, n_side),)
                sl.name = 'bench.svs'
                return UD.Dataset_wsis({'bench.svs': sl}, {'ph': TILE, 'pw': TILE, 'sh': TILE, 'sw': TILE}, bs=ma.batch_size)

            def timed(mdl, reps):
                ts_ = []
                for rep in range(reps + 1):                  # first call: warm-up (plans the workspaces)
                    dsw_ = make_dataset()
                    n_ = len(dsw_.wsis['bench.svs']['iterator'].dataset)
                    torch.cuda.synchronize()
                    a0 = time.perf_counter()
                    res_ = UE.predict_tumorbed(mdl, dsw_, 0, mode='seg', save=False)['bench.svs']
                    torch.cuda.synchronize()
                    ts_.append(time.perf_counter() - a0)
                return float(np.median(ts_[1:])), res_, n_
            t_api, res, n_api = timed(model, 3)
            t_gen, res_gen, _ = timed(_Opaque(model), 1)
        for k, v in saved.items():
            setattr(ma, k, v)
        api = {'value': round(n_api / t_api, 1), 'unit': unit, 'ms_per_slide': round(t_api * 1e3, 3), 'tiles': n_api,
               'vs_headline': round(n_api / t_api / value, 4),
               'bare_engine_one_slide_per_call': {'value': round(args.seg_tiles / t_ref, 1), 'ms_per_slide': round(t_ref * 1e3, 3), 'tiles': args.seg_tiles,
                                                  'note': 'UNetEngine.forward_tiles of the timed region (logits only: no stitch, no softmax, no maps to the host), one call + one '
                                                          'synchronisation per slide, right before the API calls (median of 3 after one warm-up)'},
               'vs_bare_engine_one_slide_per_call': round((n_api / t_api) / (args.seg_tiles / t_ref), 4),
               'bare_pipeline_one_slide_per_call': {'value': round(args.seg_tiles / t_pipe, 1), 'ms_per_slide': round(t_pipe * 1e3, 3), 'tiles': args.seg_tiles,
                                                    'note': 'the same engine call followed by what the API adds behind it, written by hand against the engine module: float64 '
                                                            'map, dense stitch, exponent-span guard, softmax + threshold + arg-max (device-resident mask), both u8 maps to the host'},
               'vs_bare_pipeline_one_slide_per_call': round((n_api / t_api) / (args.seg_tiles / t_pipe), 4),
               'call': "utils.eval.predict_tumorbed(UNetSeg(4, precision=%r), utils.dataset.Dataset_wsis(...), ep, mode='seg', save=False)" % args.mode,
               'timed': 'after the timed region: median of 3 calls after one warm-up call; includes the mask upload, the float64 dense stitch of every '
                        '(4, 256, 256) block, the exponent-span guard, softmax + threshold + argmax on the %d x %d map, u8 maps to the host' % (n_side, n_side),
               'generic_iterator_path': {'value': round(n_api / t_gen, 1), 'ms_per_slide': round(t_gen * 1e3, 3),
                                         'note': 'the loop as the reference writes it: model.decoder(model.encoder(batch_image)) per iterator batch of %d tiles '
                                                 '(myargs.batch_size), fp32 batches and fp32 encoder maps between the two calls; one call after a warm-up' % ma.batch_size,
                                         'class_map_pixels_differing_from_fused_path': round(float((res_gen['classes'] != res['classes']).mean()), 6),
                                         'why_not_zero': 'the generic loop feeds normalised fp32 tiles (split into the kernel format), the fused path the integer stem on u8 pixels: '
                                                         'logits differ inside the 1e-3 contract, near-ties of the arg-max flip'}}
        del model
        torch.cuda.empty_cache()

    if args.workload == 'seg' and rank == 0 and args.full:
        # roofline of the seg path's dominant kernels = the ten 3x3 convs of the decoder (same conv3x3s1 kernels as the trunk on PF
        # tensors): algorithmic FLOPs over REAL channels (6.04 GFLOP per tile) / their summed HIP-event time in the kernel leg
        k6, k10 = per_kind.get('unet_decoder_conv3x3'), per_kind.get('unet_tail_fused')
        if k6:
            dec_ms = k6['avg_ms'] * k6['launches'] + (k10['avg_ms'] * k10['launches'] if k10 else 0.0)
            tf = SEG_DECODER_GFLOP * 1e9 * args.seg_tiles * args.steps / (dec_ms * 1e-3) / 1e12
            roofline = {'kernel': 'U-Net decoder 3x3 convs (per batch: 8 launches of conv3x3s1_wide_kernel / conv3x3s1_slab3_kernel on 16..128-wide maps + the fused '
                                  'last block and head, unet_tail2_kernel; three-launch tail: 10 launches)' if k10 else
                                  'U-Net decoder 3x3 convs (10 launches per batch: conv3x3s1_wide_kernel / conv3x3s1_slab3_kernel on 16..256-wide maps)',
                        'bound': 'mfma', 'achieved': round(tf, 2), 'peak': PEAK_BF16_TFLOPS, 'unit': 'TFLOP/s', 'frac': round(tf / PEAK_BF16_TFLOPS, 4),
                        'traffic': None, 'avg_launch_ms': round(dec_ms / (k6['launches'] + (k10['launches'] if k10 else 0)), 4),
                        'share_of_step': k6['share_of_step'] + (k10['share_of_step'] if k10 else 0.0),
                        'algorithmic_gflop_per_tile': SEG_DECODER_GFLOP, 'precision_mode': args.mode,
                        'whole_path_tflops': round(SEG_TILE_GFLOP * 1e9 * units_per_step * args.steps / dt / 1e12, 2)}
            if k10:
                # the fused tail alone: FLOPs of the reference formulation over real channels (9 * (32 * 16 + 16 * 16) + 16 * 4 MACs per pixel), its
                # HBM traffic from the PMC passes of profiles/r05_traffic_seg.txt (2.15 MB read + 1.05 MB written per tile = the algorithmic bytes)
                roofline['tail'] = {'kernel': 'unet_tail2_kernel (nearest x2 upsample + conv 32->16 + conv 16->16 + 1x1 head, one launch)', 'bound': 'mfma',
                                    'achieved': round(k10['tflops'], 2), 'peak': PEAK_BF16_TFLOPS, 'unit': 'TFLOP/s', 'frac': round(k10['tflops'] / PEAK_BF16_TFLOPS, 4),
                                    'avg_launch_ms': round(k10['avg_ms'], 4), 'share_of_step': k10['share_of_step'],
                                    'traffic': {'read_bytes_per_tile': 2.15e6, 'write_bytes_per_tile': 1.05e6, 'algorithmic_bytes_per_tile': 128 * 128 * 128 + 4 * 256 * 256 * 4,
                                                'source': 'profiles/r05_traffic_seg.txt (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, FETCH x2)'},
                                    'note': 'three passes of fp16 MFMA per product (parity mode) on polyphase-packed tiles: 36 MFMAs of 32 cycles per 32 output pixels = '
                                            '124 us of matrix-pipe time per 128 tiles'}
        if world == 1 and not args.no_cpu_baseline:
            from oracle import unet_oracle as UO                 # the checker, never the thing measured above
            from oracle import resnet_oracle as R
            avail = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
            cores, nsample = min(16, avail), 8
            u8 = torch.stack([level0[y:y + TILE, x:x + TILE] for x, y in sxy[:nsample].tolist()]).permute(0, 3, 1, 2).contiguous().cpu()
            xin = R.normalize_u8(u8.numpy())
            torch.set_num_threads(cores)
            with torch.no_grad():
                ref = UO.unet_forward(usd, xin)
                ts = []
                for _ in range(3):
                    c0 = time.perf_counter()
                    UO.unet_forward(usd, xin)
                    ts.append(time.perf_counter() - c0)
            got = out['seg_logits'][:nsample].cpu()
            cpu_baseline = {'value': round(nsample / float(np.median(ts)), 2), 'unit': 'patches/s', 'cores': cores, 'kind': 'port',
                            'sample': 'first %d tiles of the same slide, fp32 torch CPU spec (oracle/unet_oracle.py: parity unpinned, smp absent), 1 warm-up + median of 3' % nsample,
                            'max_abs_logit_diff_vs_gpu': float((got - ref).abs().max())}
            contract = {'mode': args.mode, 'tolerance': 1e-3, 'max_abs_logit_diff_vs_oracle': cpu_baseline['max_abs_logit_diff_vs_gpu'],
                        'max_abs_logit': float(ref.abs().max()), 'oracle_sample_tiles': nsample,
                        'note': 'per-pixel logits (4 x 256 x 256 per tile) of the first %d tiles against the CPU spec; final 1x1 conv of the seeded decoder scaled by 8/216' % nsample}
        seg_ref = ref if (world == 1 and not args.no_cpu_baseline) else None
        if planes != MX and not args.no_parity_leg:
            # the faster mode beside it: timed after the timed region; outside the contract on this path (no average pool
            # behind the per-pixel logits: its error is ~2.5e-4 of the largest |logit|)
            engx = UNetEngine(usd, dev, planes=MX, max_batch=args.seg_batch)
            ox = engx.forward_tiles(level0, sxy, TILE, TILE)
            torch.cuda.synchronize()
            x0 = time.perf_counter()
            for _ in range(2):
                ox = engx.forward_tiles(level0, sxy, TILE, TILE)
            torch.cuda.synchronize()
            xdt = (time.perf_counter() - x0) / 2
            parity_leg = {'mode': 'mx', 'value': round(args.seg_tiles / xdt, 1), 'unit': unit, 'ms_per_step': round(xdt * 1e3, 3), 'steps': 2,
                          'timed': 'after the timed region, same slide and batch',
                          'max_abs_logit_diff_vs_oracle': float((ox[:8].cpu() - seg_ref).abs().max()) if seg_ref is not None else None,
                          'note': 'outside the 1e-3 contract on the dense path: the drop-in UNetSeg defaults to parity'}
            del engx, ox

    if rank == 0:
        if contract and contract.get('max_abs_logit_diff_vs_oracle') is not None:      # pass / fail of THIS run against the stated tolerance
            contract['within_tolerance'] = bool(contract['max_abs_logit_diff_vs_oracle'] <= contract['tolerance'])
        if parity_leg and parity_leg.get('max_abs_logit_diff_vs_oracle') is not None:
            parity_leg['within_tolerance'] = bool(parity_leg['max_abs_logit_diff_vs_oracle'] <= 1e-3)
        line = {
            'metric': metric, 'value': round(value, 1), 'unit': unit,
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(dt / args.steps * 1e3, 3),
            'higher_is_better': True, 'scaling': scaling, 'vs_baseline': None,
            'dtype': {2: 'fp16 hi + fp16 lo pair (3 MFMA passes, fp32 accumulate)', 3: 'fp16 + MX-fp6 cross terms (fp32 accumulate)',
                      1: 'bf16 (fp32 accumulate)'}[planes],
            'data': 'synthetic (seeded u8 slide resident in HBM, seeded random ResNet-18 weights)',
            'config': {'workload': workload_desc, 'tiles_total': tiles_total, 'batch': args.batch, 'mode': args.mode,
                       'parallelism': parallelism, 'batches_in_flight': max(1, args.streams)},
            'roofline': roofline, 'roofline_layer1': roofline_l1, 'roofline_stem': roofline_stem, 'roofline_bf16': roofline_bf16, 'cpu_baseline': cpu_baseline,
            'contract': contract, 'parity': parity_leg, 'api': api,
            'timing': {'python_gc': 'disabled inside the timed region (timeit convention; gc.collect() right before it)' if gc_off else 'enabled',
                       'longest_step_ms': round(max(b - a_ for a_, b in zip([0.0] + step_marks[:-1], step_marks)) * 1e3, 3),
                       'note': 'longest_step_ms = the largest gap between the host returns of two consecutive steps (steps that end in a host read - cfg4, cfg5 - are '
                               'synchronous, so this is the slowest step; slide steps return after enqueueing)'},
            'kernels': per_kind,
            'kernel_leg': ({'ms_per_step': round(prof_dt / args.steps * 1e3, 3), 'steps': args.steps, 'batches_in_flight': 1,
                            'timed': 'separate pass right after the timed region: HIP events on the launch stream around every conv / stem launch'}
                           if prof_dt else None),
        }
        if args.workload == 'cfg4':
            line['roofline'] = wl.roofline(per_kind)
            line['roofline_layer1'] = None
        if args.workload == 'cfg5' and args.full:
            # the post-process leg alone (outside the timed region): HIP events around 5 repetitions on the last step's heat map
            from wsi_segmentation_pipeline_amd import postprocess as PP
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                codes, tb, pts, iou = postprocess(out)
            e1.record()
            torch.cuda.synchronize()
            npx = codes.numel()
            ms = e0.elapsed_time(e1) / 5
            line['postprocess'] = {'ms_per_map': round(ms, 3), 'map': '%dx%d' % tuple(codes.shape),
                                   'foreground_fraction': round(float(codes.float().mean()), 4),
                                   'hull_vertices': int(tb.polygon().shape[0]), 'outline_points': int(pts.shape[0]),
                                   'tb_iou_vs_synthetic_disc': round(iou, 4),
                                   'algorithmic_bytes': 'threshold 8+1, open 30x30 4 passes x 2, hull 3, perimeter 2, dilate 2 passes x 2 = 27 B/px',
                                   'GBps': round(27 * npx / (ms * 1e-3) / 1e9, 1)}
        print(json.dumps(line), flush=True)
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()


def main():
    args = parse_args()
    if args.mode is None:
        args.mode = 'parity' if args.workload == 'seg' else 'mx'
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(spawn_ranks(args.gpus))
    run_rank(args)


if __name__ == '__main__':
    main()
