"""Drop-in for the whole-slide evaluation drivers of the reference's ``utils.eval``:
predict_tumorbed (/root/reference/utils/eval.py:155-286) and predict_wsis (:22-152), plus the
region-paint stage that the reference keeps as module-level code in scannet.py:145-155, and the
patch scoring drivers predict_reg (:289-351), predict_breastpathq (:354-412) and predict_cls (:415-449).

Everything between "tile list" and "u8 heat map" stays on the GPU: batches come from the device
tile producer, the encoder/classifier run on the HIP trunk, per-tile logits are accumulated into
the float64 map by wsi_stitch_add and the softmax/threshold/argmax/heat-map is one kernel.  Only the
finished u8 images are copied back to be written as PNG.  There is no CPU fallback.

Scope: the 'cls' path composes with the first-party backbone and is implemented
end to end; predict_tumorbed(mode='seg') (the reference's default) drives ``model.decoder(model.encoder(x))`` of any GPU
model - e.g. wsi_segmentation_pipeline_amd.unet.UNetSeg, the restatement of the third-party smp U-Net the reference
uses, whose accuracy is therefore pinned to this repo's own specification of smp 0.0.x, not to the reference (absent
package, no fixtures: "parity unpinned"); predict_wsis runs any caller-supplied dense GPU module and does the
accumulate / resize / arg-max / tumour-bed post-process on the device (post-process oracles: parity unpinned too)."""
import os

import numpy as np
import torch

from myargs import args
from wsi_segmentation_pipeline_amd import engine as E
from wsi_segmentation_pipeline_amd import slide as S


class TrunkEncoder(torch.nn.Module):
    """``model.encoder`` surface over a resnets_shift.ResNet of any BasicBlock depth or a Bottleneck net (resnet50(), resnet101()):
    encoder(x) -> [deepest feature map] (the reference indexes ``encoding[0]`` for the 512-channel map, utils/eval.py:196-198;
    2048 channels for a Bottleneck net).  ``out_shapes`` lists the channels of the net's five maps, deepest first, as smp's encoders
    do; only the deepest is produced here.  The full five-map encoder of the dense 'seg' model is
    wsi_segmentation_pipeline_amd.unet.UNetEncoder (BasicBlock nets) / UNetBottleneckEncoder."""

    def __init__(self, resnet):
        super().__init__()
        self.net = resnet
        self.out_shapes = (2048, 1024, 512, 256, 64) if getattr(resnet, 'bottleneck', False) else (512, 256, 128, 64, 64)

    def forward(self, x):
        return [self.net.features(x)]


class SlideClassifierModel(torch.nn.Module):
    """First-party composition that predict_tumorbed(mode='cls') drives: ResNet trunk (resnets_shift.resnet18(), resnet34() or any
    other BasicBlock depth with 512-wide heads; resnet50() / resnet101() with 2048-wide heads) as ``encoder`` +
    models.models.Classifier / Regressor heads."""

    def __init__(self, resnet, classifier, regressor=None):
        super().__init__()
        self.encoder = TrunkEncoder(resnet)
        self.classifier = classifier
        self.regressor = regressor if regressor is not None else torch.nn.Identity()
        self.decoder = torch.nn.Identity()

    def fused_engine(self, device):
        """HIP engine with the classifier's Linear fused behind the average pool."""
        eng = self.encoder.net.hip_engine(device)
        lin = self.classifier.fc[0]
        sig = (lin.weight.data_ptr(), lin.weight._version, lin.bias._version)
        if getattr(self, '_head_sig', None) != (id(eng), sig):
            eng.set_head((lin.weight, lin.bias))
            self._head_sig = (id(eng), sig)
        return eng


    def _views_mlp(self, name):
        """The Linear tensors of `regressor.fc` / `classifier.fc` as wsi_mlp_views takes them, rebuilt when a tensor changes."""
        fc = getattr(self, name).fc
        lins = [m for m in fc if isinstance(m, torch.nn.Linear)]
        sig = tuple((t.data_ptr(), t._version) for m in lins for t in (m.weight, m.bias))
        cache = self.__dict__.setdefault('_views_mlp_cache', {})
        if cache.get(name, (None, None))[0] != sig:
            cache[name] = (sig, tuple(t.detach().to(torch.float32).contiguous() for m in lins for t in (m.weight, m.bias)))
        return cache[name][1]

    def regress_views(self, device=None, **kw):
        """engine.forward_views with ``regressor.fc`` (Linear, ReLU, Linear) as the MLP head: the mean regressor output over the views
        (default: the reference's four) of every patch; kw: x= or slide_u8=, tile_xy=, ph=, pw=; views=, clamp=, per_view=."""
        return self.encoder.net.hip_engine(device).forward_views(mlp=self._views_mlp('regressor'), **kw)

    def classify_views(self, device=None, **kw):
        """regress_views with ``classifier.fc`` (one Linear) as the head: mean logits over the views."""
        return self.encoder.net.hip_engine(device).forward_views(mlp=self._views_mlp('classifier'), **kw)


def _device_of(model):
    p = next(model.parameters())
    if not p.is_cuda:
        raise RuntimeError('move the model to the GPU first (model.cuda()): the eval drivers run on HIP kernels only')
    return p.device


def _to_host(*tensors):
    """Device tensors -> NumPy arrays: asynchronous copies into pinned host buffers, ONE synchronisation for all of them."""
    outs = []
    for t in tensors:
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=t.is_cuda)
        h.copy_(t, non_blocking=True)
        outs.append(h)
    if any(t.is_cuda for t in tensors):
        torch.cuda.current_stream().synchronize()
    return tuple(h.numpy() for h in outs)


def _save_png(arr, path):
    from PIL import Image
    Image.fromarray(arr).save(path)


def _dense_batches(model, it, scan, dev, forward):
    """(xy (B,2) int ndarray, logits (B,C,ph,pw)) per batch of a dense (per-pixel) model over a slide's tile iterator.
    Fused fast path (r05) when the model is this repo's UNetSeg and the tiles are read at the scan level's own resolution: the
    U-Net engine reads the tiles straight from the HBM-resident level (integer stem on the u8 pixels, no normalised fp32 batch,
    no fp32 round trip of the five encoder maps between `encoder` and `decoder`) in ITS batch size - the reference's
    `batch_size` flag (30 tiles, myargs.py) leaves the chip mostly idle.  Any other model, a resized scan or a host iterator:
    `forward(batch_image)` over the iterator, as the reference writes it (utils/eval.py:52-60, :196-215)."""
    from wsi_segmentation_pipeline_amd.unet import UNetSeg, equal_batches
    ds = getattr(it, 'dataset', None)
    if isinstance(model, UNetSeg) and args.scan_resize == 1 and hasattr(it, 'span') and hasattr(scan, 'device_level'):
        eng = model.hip_engine(dev)
        level = scan.device_level(args.scan_level, dev)
        lo, hi = it.span
        ph, pw = ds.params.ph, ds.params.pw
        batches = equal_batches(hi - lo, eng._batch(ph, pw))    # none for an empty span (a rank with no tiles still joins the gather)
        if not batches:
            return
        xy_dev = S._upload(ds.tile_xy[lo:hi], torch.int32, dev)     # one asynchronous upload: the host keeps enqueuing batches ahead of the GPU
        for a, b in batches:
            yield np.ascontiguousarray(ds.tile_xy[lo + a:lo + b]), eng.forward_tiles(level, xy_dev[a:b], ph, pw)
        return
    for batch_x, batch_y, batch_image in it:
        yield np.stack((batch_x.numpy(), batch_y.numpy()), 1), forward(batch_image.to(dev))


def predict_tumorbed(model, dataset, ep, mode='seg', rank=0, world=1, save=True, save_tiff=False, save_xml=False, region_table=False, bed_size=False):
    """Tumour-bed heat maps for every slide in ``dataset`` (a utils.dataset.Dataset_wsis).
    Writes <val_save_pth>/<ep>/<key>_<stride>_heatmap.png and _overlay.png (rank 0; with save_tiff also _heatmap.tif, the heat map as
    a one-component JPEG-tiled pyramid encoded on the device, wsi_segmentation_pipeline_amd.tiffwrite; with save_xml also _tb.xml, the
    tumour bed of the heat map - tumor_bed_overlay's (heat / 255 >= 0.9) -> open 30 x 30 -> convex hull - traced on the device into ImageScope
    regions named 'Invasive', in level-0 coordinates: wsi_segmentation_pipeline_amd.contours; MicronsPerPixel is the slide's where it
    states one, `scan.mpp` or openslide's mpp-x property, else 1.0) and returns
    {key: {'heatmap': u8 (H2,W2) ndarray, 'classes': u8 ndarray, 'logits': (T,C) tensor}}.
    region_table: the result gains 'slide_positive' - does the slide hold tumour at all, the reference's rule
    (paper_tools/check_for_false_positives.py:61-69: heat >= 0.99 * 255 -> open 50 x 50 -> any pixel left) on the device,
    wsi_segmentation_pipeline_amd.regions.slide_positive - and 'regions', the regions of that opened mask with the heat map as weight;
    with save, rank 0 also writes <key>_<stride>_heatmap_regions.csv in level-0 coordinates.  Unset, results and files are what they were.
    bed_size: the result gains 'bed_size', the two dimensions d1 x d2 of the tumour bed of the heat map (save_xml's bed) in pixels of the
    map and, where the slide states an mpp, millimetres (wsi_segmentation_pipeline_amd.regions.bed_size: the hull's largest diameter and
    the extent at right angles to it; None without a bed), 'bed_size_gt' likewise where the entry has `tb_gt`, and one printed line per
    slide; the regions CSV then also holds the hull columns.  Unset, results, printed lines and files are what they were."""
    if mode not in ('cls', 'seg'):
        raise ValueError("mode must be 'cls' or 'seg'")
    out_dir = '{}/{}'.format(args.val_save_pth, ep)
    if save and rank == 0:
        os.makedirs(out_dir, exist_ok=True)
    dev = _device_of(model)
    was_training = model.training
    model.eval()
    results = {}
    with torch.no_grad():
        for key in list(dataset.wsis):
            entry = dataset.wsis[key]
            it = entry['iterator']
            ds, scan = it.dataset, entry['scan']
            ref_level = min(2, len(scan.level_dimensions) - 1)
            map_hw = scan.level_dimensions[ref_level][::-1]
            m = scan.level_downsamples[args.scan_level] / scan.level_downsamples[ref_level]
            # (pinned staging + asynchronous copy: a pageable-memory copy would block the host until everything enqueued so far has run)
            def upload_mask():
                return S._upload(entry['mask'], torch.as_tensor(entry['mask']).dtype, dev) if entry.get('mask') is not None else None
            # (mode 'seg' uploads its mask - the size of the scan level there - AFTER the tile loop is enqueued: pinning 35 MB of host
            # memory costs the host 5-13 ms, during which the GPU would sit idle at the head of the call; r05 profiles/r05_api_seg_breakdown.txt)
            mask = upload_mask() if mode == 'cls' else None
            if mode == 'cls' and isinstance(model, SlideClassifierModel):
                # fused fast path: the stem kernel reads the HBM-resident slide directly
                level = scan.device_level(args.scan_level, dev)
                r = S.infer_slide_cls(model.fused_engine(dev), level, ds.tile_xy, ds.params.ph, ds.params.pw, m, map_hw,
                                      args.num_classes, args.class_probs, mask, rank, world, want_probs=False)
            elif mode == 'cls':
                # generic loop over the iterator API (any model exposing .encoder/.classifier on the GPU)
                pred = torch.zeros((args.num_classes,) + tuple(map_hw), dtype=torch.float64, device=dev)
                all_logits = []
                for batch_x, batch_y, batch_image in it:
                    logits = model.classifier(model.encoder(batch_image.to(dev))[0])
                    xy = np.stack((batch_x.numpy(), batch_y.numpy()), 1)
                    E.stitch_add(pred, logits, torch.from_numpy(S.map_coords(xy, m)), int(m * ds.params.ph), int(m * ds.params.pw))
                    all_logits.append(logits)
                classes, _, heat = E.softmax_threshold_argmax(pred, args.class_probs, mask, 'cls', want_probs=False)
                r = {'logits': torch.cat(all_logits), 'pred': pred, 'classes': classes, 'heatmap': heat}
            else:
                # mode 'seg' (the reference's default, utils/eval.py:196-215): pred_src = model.decoder(model.encoder(x)) is a
                # (B, C, ph, pw) block per tile, optionally nearest-resized to (tile_h * r, tile_w * r), added at int(m * x),
                # int(m * y) over a (dy, dx) = int(m * ph), int(m * pw) footprint - which therefore has to equal the block size
                pred = torch.zeros((args.num_classes,) + tuple(map_hw), dtype=torch.float64, device=dev)
                dy, dx = int(m * ds.params.ph), int(m * ds.params.pw)
                # world > 1 (seg mode): every rank runs a contiguous share of the raster-order tile list into its
                # own map and sends the band its tiles touch to rank 0 (slide.gather_map_bands: a direct gather, no all-reduce);
                # rank 0 sums the bands - exact, hence identical to the single-rank map, inside the exponent-span bound of the
                # stitch - thresholds, and broadcasts the two u8 maps
                my_it = it
                if world > 1:
                    lo, hi = S.shard_range(len(ds), rank, world)
                    my_it = it.shard(lo, hi)
                span_lo, span_hi = None, None                 # exponent range of every addend: the exactness guard of the float64 sums
                my_txy = []

                for xy, pred_src in _dense_batches(model, my_it, scan, dev, lambda x: model.decoder(model.encoder(x))):
                    if args.scan_resize != 1:
                        pred_src = E.resize_nearest(pred_src, (int(args.tile_h * args.scan_resize), int(args.tile_w * args.scan_resize)))
                    if tuple(pred_src.shape[2:]) != (dy, dx):
                        raise ValueError("mode='seg': the decoder output %s does not match the stitch footprint (%d, %d) = int(m * tile); "
                                         "scan at the map's level or set scan_resize (utils/eval.py:202-215)" % (tuple(pred_src.shape[2:]), dy, dx))
                    txy = S.map_coords(xy, m)
                    my_txy.append(np.asarray(txy))
                    E.stitch_add_dense(pred, pred_src, S._upload(txy, torch.int32, dev))      # (pinned + asynchronous: a pageable copy blocks the host)
                    sp = E.exponent_span(pred_src)
                    span_lo = sp[0:1] if span_lo is None else torch.minimum(span_lo, sp[0:1])
                    span_hi = sp[1:2] if span_hi is None else torch.maximum(span_hi, sp[1:2])
                span = torch.cat((span_lo, span_hi)) if span_lo is not None else None
                mask = upload_mask()
                if world > 1:
                    txy_all = np.concatenate(my_txy) if my_txy else np.zeros((0, 2), np.int64)
                    pred = S.gather_map_bands(pred, txy_all, dy, dx, rank, world, dst=0)
                    span = S.allreduce_span(span, dev)
                if world == 1 or rank == 0:
                    classes, _, heat = E.softmax_threshold_argmax(pred, args.class_probs, mask, 'seg', want_probs=False)
                else:
                    classes, heat = (torch.empty(tuple(map_hw), dtype=torch.uint8, device=dev) for _ in range(2))
                if world > 1:
                    classes, heat = S.broadcast_from(classes, 0), S.broadcast_from(heat, 0)
                r = {'logits': None, 'pred': pred, 'classes': classes, 'heatmap': heat, 'exponent_span': span}
            stitch_exact = None
            if r.get('exponent_span') is not None:             # the float64 stitch is exact (order- and rank-independent) inside this
                over = (-(-ds.params.ph // ds.params.sh) + 1) * (-(-ds.params.pw // ds.params.sw) + 1)      # bound; outside it the map
                stitch_exact = E.stitch_is_exact(r['exponent_span'], over)                                   # is right to float64 rounding only
            heat, classes_np = _to_host(r['heatmap'], r['classes'])          # both u8 maps in one round trip through pinned memory
            results[key] = {'heatmap': heat, 'classes': classes_np, 'logits': r['logits'],
                            'precision': r.get('precision'),          # precision='auto': the mode this slide ran in, and why
                            'stitch_exact': stitch_exact}
            if region_table:
                from wsi_segmentation_pipeline_amd import regions as RG
                results[key]['slide_positive'], results[key]['regions'] = RG._slide_positive(r['heatmap'].contiguous(), 0.99, 50, 0.0,
                                                                                             **({'hulls': True} if bed_size else {}))
            if bed_size:
                from wsi_segmentation_pipeline_amd import postprocess as PP
                results[key].update(_bed_size(key, PP.tumor_bed_from_heatmap(r['heatmap'].contiguous(), 0.9, 30, 20).tb_pred, entry.get('tb_gt'), scan,
                                              ref_level, map_hw, dev))
            if save and rank == 0:
                _save_png(heat, '{}/{}_{}_heatmap.png'.format(out_dir, key, args.tile_stride_w))
                thumb = np.asarray(scan.read_region((0, 0), ref_level, scan.level_dimensions[ref_level]).convert('RGB'))
                over = thumb * 0.75 + 255 * np.repeat((heat > 255 * 0.99)[..., None], 3, -1) * 0.25
                _save_png(np.uint8(over), '{}/{}_{}_overlay.png'.format(out_dir, key, args.tile_stride_w))
                if save_tiff:
                    from wsi_segmentation_pipeline_amd import tiffwrite
                    tiffwrite.write_pyramid('{}/{}_{}_heatmap.tif'.format(out_dir, key, args.tile_stride_w), r['heatmap'].contiguous(), downsample=2)
                if save_xml:
                    from wsi_segmentation_pipeline_amd import annotations as AN, contours as CT, postprocess as PP
                    bed = (PP.tumor_bed_from_heatmap(r['heatmap'].contiguous(), 0.9, 30, 20).tb_pred > 0).to(torch.uint8)
                    traced = CT.trace(bed, [1], AN.level_step(scan, ref_level), bounds=scan.level_dimensions[0])
                    CT.write_imagescope('{}/{}_{}_tb.xml'.format(out_dir, key, args.tile_stride_w), traced, CT.slide_mpp(scan), {1: 'Invasive'})
                if region_table:
                    from wsi_segmentation_pipeline_amd import annotations as AN, contours as CT
                    RG.write_csv('{}/{}_{}_heatmap_regions.csv'.format(out_dir, key, args.tile_stride_w), results[key]['regions'],
                                 AN.level_step(scan, ref_level), (0, 0), CT.stated_mpp(scan), {1: 'Invasive'}, **({'hulls': True} if bed_size else {}))
            dataset.wsis[key] = None                       # the reference frees each slide after use (:282)
    if was_training:
        model.train()
    return results


def _bed_size(key, bed, tb_gt, scan, ref_level, map_hw, dev, scores=None):
    """the bed's two dimensions (regions.bed_size) of the predicted bed and, where there is one, of the annotated bed; `scores` gains
    the differences predicted - annotated.  One printed line per slide.  -> the entries to add to the slide's result"""
    from wsi_segmentation_pipeline_amd import annotations as AN, contours as CT, regions as RG
    step, mpp = AN.level_step(scan, ref_level), CT.stated_mpp(scan)
    out = {'bed_size': RG.bed_size((bed > 0).to(torch.uint8).contiguous(), step, mpp)}
    line = '{}, tb size: '.format(key) + ('none' if out['bed_size'] is None else '{:.1f} x {:.1f} px'.format(out['bed_size']['d1'], out['bed_size']['d2']))
    if out['bed_size'] is not None and mpp is not None:
        line += ' ({:.2f} x {:.2f} mm)'.format(out['bed_size']['d1_mm'], out['bed_size']['d2_mm'])
    if tb_gt is not None:
        out['bed_size_gt'] = RG.bed_size((_map_u8(tb_gt, map_hw, dev) > 0).to(torch.uint8).contiguous(), step, mpp)
        a, b = out['bed_size'], out['bed_size_gt']
        if scores is not None and a is not None and b is not None:
            for d in ('d1', 'd2'):
                scores['tb_%s_err' % d] = a[d] - b[d]
                if mpp is not None:
                    scores['tb_%s_err_mm' % d] = a[d + '_mm'] - b[d + '_mm']
        if b is not None:
            line += ', annotated {:.1f} x {:.1f} px'.format(b['d1'], b['d2'])
    print(line)
    return out


def _map_u8(arr, hw, dev):
    """Ground-truth image -> uint8 (H,W) device tensor at map resolution (nearest-neighbour when the size differs; the
    reference resizes with PIL's version-dependent default filter, utils/eval.py:77-78).  A GPU tensor (a map rasterised by
    wsi_segmentation_pipeline_amd.annotations) stays on the device: passed through at equal size, resized by the same rule otherwise."""
    if isinstance(arr, torch.Tensor) and arr.is_cuda:
        a = arr[..., 0] if arr.dim() == 3 else arr
        if tuple(a.shape) != tuple(hw):
            ys = (torch.arange(hw[0], device=a.device) * a.shape[0] // hw[0]).clamp(0, a.shape[0] - 1)
            xs = (torch.arange(hw[1], device=a.device) * a.shape[1] // hw[1]).clamp(0, a.shape[1] - 1)
            a = a[ys][:, xs]
        return a.to(dev, torch.uint8).contiguous()
    a = np.asarray(arr)
    if a.ndim == 3:
        a = a[..., 0]
    if tuple(a.shape) != tuple(hw):
        ys = (np.arange(hw[0]) * a.shape[0] // hw[0]).clip(0, a.shape[0] - 1)
        xs = (np.arange(hw[1]) * a.shape[1] // hw[1]).clip(0, a.shape[1] - 1)
        a = a[ys][:, xs]
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8))).to(dev)


def predict_wsis(model, dataset, ep, save=True, save_tiff=False, save_xml=False, boundary_scores=False, region_table=False, bed_size=False):
    """Dense per-pixel map prediction with the tumour-bed post-process (reference utils/eval.py:22-152).
    `model(batch_image)` must return (B, C, ph, pw) logits on the GPU (the reference drives an smp U-Net here; any GPU
    module works, e.g. wsi_segmentation_pipeline_amd.unet.UNetSeg).  Everything between the tile list and the colour
    mask stays on the device:
      :58-60    pred[:, y:y+ph, x:x+pw] += pred_src[b]      float64, scan-level resolution (wsi_stitch_add_dense)
      :66-71    cv2.resize of every class map to level-2     wsi_resize_bilinear_f64
      :82-96    argmax -> (p >= 2) -> open 20x20 -> convex hull -> perimeter -> dilate 20x20     wsi_tumor_bed
      :100-123  tumour-bed IoU, accuracy / score figures against `entry['gt']` / `entry['tb_gt']` (when the dataset
                entry carries them: the reference reads <wsipath>_mask.png / _tumor_bed.png)    wsi_score_counts, wsi_mask_iou_counts
      :138-145  colour mask (threshold_probs classes on the foreground mask, tumour-bed outline in white), saved at half size
    save_tiff (with save): additionally <key>_<stride>.tif, the colour mask at SCAN-LEVEL resolution - the scan-level `classes`, the
    foreground mask and the outline scaled up by nearest - as a JPEG-tiled pyramid encoded on the device (tiffwrite.write_pyramid).
    save_xml (with save): additionally <key>_<stride>.xml, ImageScope annotations in level-0 coordinates traced on the device
    (wsi_segmentation_pipeline_amd.contours): classes 1 - 3 of the thresholded map on the foreground mask, what the PNG shows, as
    Benign / In situ / Invasive regions, holes as NegativeROA regions, so annotations.read_imagescope(path, negative='erase') rasterised
    at the map's step restores that map; a second Annotation element, which neither reader visits, holds the tumour bed as 'Invasive'.
    MicronsPerPixel is the slide's where it states one (`scan.mpp`, or openslide's mpp-x property), else 1.0.
    boundary_scores: where the entry has `tb_gt`, `scores` gains how far the predicted bed's outline lies from the ground truth's
    (wsi_segmentation_pipeline_amd.distance.surface_distances on the device): 'hd_tb', 'hd95_tb', 'assd_tb' - Hausdorff, its 95th
    percentile by nearest rank, the mean surface distance - in pixels of the scoring level, and, where the slide states an mpp, the
    same three with the suffix '_um' (mpp times the level's step).  Unset, `scores` and the printed line are what they were.
    region_table: the result gains 'regions', the region table (wsi_segmentation_pipeline_amd.regions.label, connectivity 8) of classes
    1 - 3 of `classes_level2` on the foreground mask; with save also <key>_<stride>_regions.csv in level-0 coordinates, areas in square
    microns where the slide states an mpp; where the entry has `gt`, `scores` gains lesions as objects for classes (2, 3), the
    reference's own tumour rule p >= 2: 'lesions_pred', 'lesions_gt', 'lesion_precision', 'lesion_recall', 'lesion_f1'
    (regions.lesion_scores, IoU 0.5).  Unset, results, printed lines and files are what they were.
    bed_size: the result gains 'bed_size', the two dimensions d1 x d2 a pathologist reports for the tumour bed, of `tumor_bed`
    (wsi_segmentation_pipeline_amd.regions.bed_size: the hull's largest diameter and the extent at right angles to it, in pixels of the
    scoring level, d1_mm, d2_mm, area_mm2 where the slide states an mpp; None without a bed); where the entry has `tb_gt` also
    'bed_size_gt' and, in `scores`, 'tb_d1_err', 'tb_d2_err' (predicted minus annotated, pixels) with '_mm' variants where the slide
    states an mpp; one printed line per slide.  With region_table and save the regions CSV then also holds the hull columns.  Unset,
    results, printed lines and files are what they were.
    Returns {key: {'pred', 'pred_level2', 'classes' (scan level), 'classes_level2', 'tumor_bed', 'outline', 'scores'}}."""
    from wsi_segmentation_pipeline_amd import postprocess as PP
    out_dir = '{}/{}'.format(args.val_save_pth, ep)
    if save:
        os.makedirs(out_dir, exist_ok=True)
    dev = _device_of(model)
    was_training = model.training
    model.eval()
    results = {}
    ious_tb = 0.0
    with torch.no_grad():
        for key in list(dataset.wsis):
            entry = dataset.wsis[key]
            it = entry['iterator']
            ds, scan = it.dataset, entry['scan']
            iw, ih = scan.level_dimensions[args.scan_level]
            pred = torch.zeros((args.num_classes, ih, iw), dtype=torch.float64, device=dev)
            for xy, pred_src in _dense_batches(model, it, scan, dev, model):
                if pred_src.dim() != 4 or pred_src.shape[1] != args.num_classes:
                    raise ValueError('predict_wsis needs a dense model returning (B, %d, ph, pw)' % args.num_classes)
                E.stitch_add_dense(pred, pred_src, S._upload(xy, torch.int32, dev))        # int(batch_x[bj]): truncation
            classes = PP.argmax_classes(pred)
            ref_level = min(2, len(scan.level_dimensions) - 1)
            map_hw = tuple(scan.level_dimensions[ref_level][::-1])
            pred2 = PP.resize_bilinear(pred, map_hw)                           # :66-71
            p = PP.argmax_classes(pred2)                                       # :82
            tb = PP.tumor_bed(p, 2, 20, 20)                                    # :90-96
            mask = entry.get('mask')
            mask_dev = _map_u8(mask, map_hw, dev) if mask is not None else torch.ones(map_hw, dtype=torch.uint8, device=dev)
            scores = None
            if entry.get('gt') is not None:                                    # :74-135
                scores = PP.wsi_scores(p, _map_u8(entry['gt'], map_hw, dev), (mask_dev > 0).to(torch.uint8), args.epsilon)
                scores['iou_tb'] = -1
                if entry.get('tb_gt') is not None:
                    scores['iou_tb'] = PP.mask_iou((_map_u8(entry['tb_gt'], map_hw, dev) > 0).to(torch.uint8), tb.tb_pred, args.epsilon)
                    ious_tb += scores['iou_tb']
                print('{}, {:.3f}({:.3f}), {:.3f}({:.3f}), {:.3f}, tb iou: {:.3f} '.format(
                    key, scores['s_masked'], scores['s'], scores['acc_masked'], scores['acc'], scores['iou_fg'], scores['iou_tb']))
                if boundary_scores and entry.get('tb_gt') is not None:
                    from wsi_segmentation_pipeline_amd import annotations as AN, contours as CT, distance as DT
                    sd = DT.surface_distances((tb.tb_pred > 0).to(torch.uint8), (_map_u8(entry['tb_gt'], map_hw, dev) > 0).to(torch.uint8))
                    for name in ('hd', 'hd95', 'assd'):
                        scores[name + '_tb'] = sd[name]
                    if CT.stated_mpp(scan) is not None:
                        um = CT.stated_mpp(scan) * AN.level_step(scan, ref_level)
                        for name in ('hd', 'hd95', 'assd'):
                            scores[name + '_tb_um'] = sd[name] * um
                    print('{}, tb outline: hd {:.2f}, hd95 {:.2f}, assd {:.2f} px'.format(key, sd['hd'], sd['hd95'], sd['assd']))
                if region_table:
                    from wsi_segmentation_pipeline_amd import regions as RG
                    ls = RG.lesion_scores(p, _map_u8(entry['gt'], map_hw, dev), classes=(2, 3))
                    scores.update(lesions_pred=ls['n_pred'], lesions_gt=ls['n_gt'], lesion_precision=ls['precision'], lesion_recall=ls['recall'],
                                  lesion_f1=ls['f1'])
                    print('{}, lesions: {} predicted, {} annotated, precision {:.3f}, recall {:.3f}, f1 {:.3f}'.format(
                        key, ls['n_pred'], ls['n_gt'], ls['precision'], ls['recall'], ls['f1']))
            results[key] = {'pred': pred, 'pred_level2': pred2, 'classes': classes, 'classes_level2': p,
                            'tumor_bed': tb.tb_pred, 'outline': tb.outline, 'scores': scores}
            if region_table:
                from wsi_segmentation_pipeline_amd import annotations as AN, contours as CT, regions as RG
                results[key]['regions'] = RG.label((p * (mask_dev > 0)).to(torch.uint8).contiguous(), (1, 2, 3), 8, labels=False,
                                                   **({'hulls': True} if bed_size else {}))
                if save:
                    RG.write_csv('{}/{}_{}_regions.csv'.format(out_dir, key, args.tile_stride_w), results[key]['regions'],
                                 AN.level_step(scan, ref_level), (0, 0), CT.stated_mpp(scan), CT.DEFAULT_NAMES, **({'hulls': True} if bed_size else {}))
            if bed_size:
                results[key].update(_bed_size(key, tb.tb_pred, entry.get('tb_gt'), scan, ref_level, map_hw, dev, scores))
            if save:                                                           # :138-145
                cls_thr = E.softmax_threshold_argmax(pred2, args.class_probs, want_probs=False)[0]      # pred_to_mask
                rgb = torch.zeros(map_hw + (3,), dtype=torch.uint8, device=dev)
                for cj in range(min(args.num_classes - 1, 3)):                  # class k > 0 -> channel k - 1
                    rgb[..., cj] = (cls_thr == cj + 1).to(torch.uint8) * 255
                rgb = rgb * mask_dev[..., None]
                rgb[tb.outline > 0] = 255
                from PIL import Image
                img = Image.fromarray(rgb.cpu().numpy())
                img.resize((max(1, map_hw[1] // 2), max(1, map_hw[0] // 2))).save('{}/{}_{}.png'.format(out_dir, key, args.tile_stride_w))
                if save_tiff:
                    from wsi_segmentation_pipeline_amd import tiffwrite
                    ys = torch.arange(ih, device=dev) * map_hw[0] // ih          # nearest: scan-level row -> map row
                    xs = torch.arange(iw, device=dev) * map_hw[1] // iw
                    keep, edge = (mask_dev > 0)[ys][:, xs], (tb.outline > 0)[ys][:, xs]
                    full = torch.zeros((ih, iw, 3), dtype=torch.uint8, device=dev)
                    for cj in range(min(args.num_classes - 1, 3)):
                        full[..., cj] = ((classes == cj + 1) & keep).to(torch.uint8) * 255
                    full[edge] = 255
                    tiffwrite.write_pyramid('{}/{}_{}.tif'.format(out_dir, key, args.tile_stride_w), full, downsample=2)
                if save_xml:
                    from wsi_segmentation_pipeline_amd import annotations as AN, contours as CT
                    step, size0 = AN.level_step(scan, ref_level), scan.level_dimensions[0]
                    shown = (cls_thr * (mask_dev > 0)).to(torch.uint8).contiguous()
                    bed = CT.trace((tb.tb_pred > 0).to(torch.uint8), [1], step, bounds=size0)
                    CT.write_imagescope('{}/{}_{}.xml'.format(out_dir, key, args.tile_stride_w), CT.trace(shown, (1, 2, 3), step, bounds=size0),
                                        CT.slide_mpp(scan), layers=[(bed, {1: 'Invasive'})])
        if dataset.wsis:
            print('Average tb iou: {:.3f}'.format(ious_tb / len(dataset.wsis)))
    if was_training:
        model.train()
    return results


def tumor_bed_overlay(heat_u8, thumb_rgb=None):
    """The tumour-bed outline of a stitched u8 heat map (reference paper_tools/overlay_tb_wsi.py:46-64) on the device:
    (heat / 255 >= 0.9) -> open 30x30 -> convex hull -> perimeter -> dilate 20x20.  Returns the
    wsi_segmentation_pipeline_amd.postprocess.TumorBed (opened mask, hull image, outline, .outline_points(n) via esp) and,
    with a (H,W,3) u8 thumbnail on the GPU, the overlay 0.65 * wsi + 0.35 * (heat * opened) with the outline in black."""
    from wsi_segmentation_pipeline_amd import postprocess as PP
    tb = PP.tumor_bed_from_heatmap(heat_u8, 0.9, 30, 20)
    if thumb_rgb is None:
        return tb, None
    hm = (heat_u8 * tb.opened).to(torch.float64)[..., None].expand(-1, -1, 3)
    over = 0.65 * thumb_rgb.to(torch.float64) + 0.35 * hm
    over[tb.outline > 0] = 0
    return tb, over.to(torch.uint8)


def predict_regions(model, iterator, metadata, label_shape, class_probs=None, rank=0, world=1):
    """Region-proposal evaluation stage (reference scannet.py:145-155 / slic.py:93-99, with the documented fix: the
    ensemble logits are soft-maxed over the class axis): bags -> ResNet bag forward on the HIP path -> class per region ->
    painted label image (int64 ndarray).  With world > 1 (torch.distributed initialised) the bags are sharded over the ranks
    by greedy cost balance, each rank runs its share, ONE all-gather of the (R, C) ensemble logits follows and every rank
    paints the identical label image on its device (wsi_paint_regions).  `iterator`: a utils.dataset_hr.DeviceBagIterator
    (`.dataset`, `.shard`: needed for world > 1), or - single rank - any iterable of (images (B,16,3,64,64), tile_ids) batches
    like the reference's DataLoader (scannet.py:147-155)."""
    from wsi_segmentation_pipeline_amd import bags as B
    class_probs = args.class_probs if class_probs is None else class_probs
    dev = _device_of(model)
    was_training = model.training
    model.eval()
    data = getattr(iterator, 'dataset', None)
    if world > 1 and (data is None or not hasattr(iterator, 'shard')):
        raise ValueError('predict_regions over several ranks needs a shardable iterator (utils.dataset_hr.DeviceBagIterator)')
    R = len(data) if data is not None else None
    shards = B.shard_bags(np.full(R, 16.0), world) if world > 1 else None
    mine = iterator.shard(shards[rank]) if world > 1 else iterator
    seen_ids = []                                             # plain iterables: the tile ids come with the batches
    with torch.no_grad():
        parts = []
        eng = model.hip_engine(dev) if world > 1 and hasattr(model, 'hip_engine') else None
        if hasattr(eng, 'probe_f32'):
            # precision='auto' over several ranks: ONE mode for every rank.  The probe is a stratified sample over this rank's
            # WHOLE shard of bags (r03 advisor finding: probing the first batch only is the first-tiles blind spot the per-slide
            # stratified probe was introduced to remove): up to `eng.probe` bags spread evenly over the shard, their crops
            # sub-sampled by probe_f32; a rank without bags still takes part in the collective
            mine_idx = list(shards[rank])
            eng.reset()
            err = 0.0
            if mine_idx:
                nb = min(int(getattr(eng, 'probe', 32)), len(mine_idx))
                pick = sorted({mine_idx[int(round(v))] for v in np.linspace(0, len(mine_idx) - 1, nb)})
                sample = torch.cat([im.to(dev).reshape(-1, *im.shape[2:]) for im, _ in iterator.shard(pick)])
                err = eng.probe_f32(sample)
            eng.decide(S.allreduce_max(err, dev, world), scope='regions')
        for images, tile_ids in mine:
            if data is None:
                seen_ids.extend(int(t) for t in tile_ids)
            parts.append(model(images.to(dev))[1])
        num_classes = len(class_probs)
        local = torch.cat(parts) if parts else torch.zeros((0, num_classes), dtype=torch.float32, device=dev)
        ens = B.gather_rows(local, shards, rank, world) if world > 1 else local
        if R is None:
            R = len(seen_ids)
        if R:
            # (R,C) logits as a (C,R,1) "map": softmax over classes / threshold / argmax in one HIP kernel
            as_map = ens.t().to(torch.float64).contiguous().view(ens.shape[1], -1, 1)
            cls = E.softmax_threshold_argmax(as_map, class_probs, want_probs=False)[0].view(-1)
            ids = [int(r['tile_id']) for r in data.datalist] if data is not None else seen_ids
            index_lists = [metadata[t]['foreground_indices'] for t in ids]
            pred_mask = B.paint_regions(tuple(label_shape), index_lists, cls, dev).cpu().numpy()
        else:
            pred_mask = np.zeros(label_shape, dtype=np.int64)
    if was_training:
        model.train()
    return pred_mask


# ---------------------------------------------------------------------------------------------- patch scoring drivers
def torch_view(image, v):
    """View `v` (include/wsi_hip.h: T = 1, FY = 2, FX = 4) of an (N, C, H, W) tensor with torch ops; ids 0, 1, 2, 5 are the reference's
    image, image.transpose(2, 3), image.flip(2), image.transpose(2, 3).flip(3) (utils/eval.py:308-313)."""
    if v & E.VIEW_T:
        image = image.transpose(2, 3)
    if v & E.VIEW_FY:
        image = image.flip(2)
    if v & E.VIEW_FX:
        image = image.flip(3)
    return image


def module_loop_views(model, head, image, views=E.VIEWS_REFERENCE):
    """The reference's loop as it writes it (utils/eval.py:307-321, :336): `head(model.encoder(view)[0])` per view with torch views,
    summed in view order and divided by their number.  The path of any GPU model exposing .encoder and the head, and the baseline
    the fused path is measured against."""
    acc = None
    for v in views:
        pred = head(model.encoder(torch_view(image, v).contiguous())[0])
        acc = pred.clone() if acc is None else acc.add_(pred)
    return acc / len(views)


def _fused_head(model, name):
    from models import models as M
    return isinstance(model, SlideClassifierModel) and isinstance(getattr(model, name), M.Regressor if name == 'regressor' else M.Classifier)


def _score_views(model, name, views, clamp=None, **source):
    """Mean head output (N, K) over `views`: the fused HIP path for a SlideClassifierModel with models.models heads, the module loop
    for any other model (fp32 input only)."""
    if _fused_head(model, name):
        return (model.regress_views if name == 'regressor' else model.classify_views)(views=views, clamp=clamp, **source)
    out = module_loop_views(model, getattr(model, name), source['x'], views)
    return out.clamp(clamp[0], clamp[1]) if clamp is not None else out


def cls_scores(gts, preds):
    """(accuracy, F1 of class 1) of integer labels: what the reference prints from np.mean(preds == gts) and sklearn's
    f1_score(gts, preds) (binary default: 2 TP / (2 TP + FP + FN), 0 where that is undefined), restated in NumPy."""
    gts, preds = np.asarray(gts).reshape(-1), np.asarray(preds).reshape(-1)
    if gts.shape != preds.shape:
        raise ValueError('%d labels for %d predictions' % (gts.size, preds.size))
    tp = int(np.sum((preds == 1) & (gts == 1)))
    fp = int(np.sum((preds == 1) & (gts != 1)))
    fn = int(np.sum((preds != 1) & (gts == 1)))
    acc = float(np.mean(preds == gts)) if gts.size else float('nan')
    return acc, (2.0 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)


def predict_reg(model, dataset, ep):
    """Cellularity regression over a patch iterator (reference utils/eval.py:289-351).  `dataset` yields (image, label, is_cls, is_reg,
    is_seg, cls_code) batches (utils.dataset.GenerateIterator); every image is scored as the mean of `model.regressor` over the
    reference's four views.  Prints the reference's l1 / mse line and returns {'preds', 'gts', 'l1', 'mse'}; the model's
    train / eval state is restored.  A SlideClassifierModel with a models.models.Regressor runs the fused path
    (engine.forward_views); any other GPU model with .encoder / .regressor runs the reference's module loop.
    Out of scope: the segmentation overlay PNGs the reference writes to a hard-coded data/cell_seg/ (:323-334) - no decoder runs."""
    dev = _device_of(model)
    was_training = model.training
    model.eval()
    preds, gts = [], []
    with torch.no_grad():
        for image, label, is_cls, is_reg, is_seg, cls_code in dataset:
            pred = _score_views(model, 'regressor', E.VIEWS_REFERENCE, x=image.to(dev))
            preds.extend(pred.reshape(-1).cpu().numpy())
            gts.extend(np.asarray(cls_code).reshape(-1))
    preds, gts = np.asarray(preds), np.asarray(gts)
    l1, mse = float(np.mean(np.abs(preds - gts))), float(np.mean((preds - gts) ** 2))
    print('Ep. {}, l1 {:.3f}, mse {:.3f}, '.format(ep, l1, mse))
    if was_training:
        model.train()
    return {'preds': preds, 'gts': gts, 'l1': l1, 'mse': mse}


def predict_cls(model, dataset, ep):
    """Patch classification over the same iterator (reference utils/eval.py:415-449): arg-max of `model.classifier` on the items
    flagged is_cls, accuracy and the binary F1 of class 1 (`cls_scores`).  Prints the reference's line and returns {'preds', 'gts',
    'acc', 'f1'}.
    Deviation from the reference: `preds` and `gts` both hold the is_cls items only.  The reference extends `gts` with EVERY item's
    code and, for a batch without any is_cls item, extends `preds` with the previous batch's stale predictions, so its two lists
    only line up when every item is a classification item - the case in which both agree."""
    dev = _device_of(model)
    was_training = model.training
    model.eval()
    preds, gts = [], []
    with torch.no_grad():
        for image, label, is_cls, is_reg, is_seg, cls_code in dataset:
            keep = torch.as_tensor(is_cls).to(torch.bool)
            if not bool(keep.any()):
                continue
            logits = _score_views(model, 'classifier', (0,), x=image[keep].to(dev))
            preds.extend(torch.argmax(logits, 1).cpu().numpy())
            gts.extend(np.asarray(cls_code)[keep.numpy()])
    preds, gts = np.asarray(preds), np.asarray(gts)
    acc, f1 = cls_scores(gts, preds)
    print('Ep. {}, acc {:.3f},f1 {:.3f}'.format(ep, acc, f1))
    if was_training:
        model.train()
    return {'preds': preds, 'gts': gts, 'acc': acc, 'f1': f1}


def breastpathq_rows(label_csv_path):
    """[(image id, region id)] of the label file in its row order (header skipped), as the reference reads it (:373-381)."""
    import csv
    with open(label_csv_path) as f:
        reader = csv.reader(f, delimiter=',')
        next(reader)
        return [(int(row[0]), int(row[1])) for row in reader if row]


def breastpathq_image(dataset_path, image_id, region_id):
    """<dataset_path>/<image>_<region>.tif as RGB u8 (tile_h, tile_w, 3): Pillow's Image.resize((tile_w, tile_h), Image.BILINEAR), which
    is what torchvision.transforms.Resize((tile_h, tile_w)) does to a PIL image (:358, :385-386)."""
    from PIL import Image
    image = Image.open('{}/{}_{}.tif'.format(dataset_path, image_id, region_id)).convert('RGB')
    return np.asarray(image.resize((args.tile_w, args.tile_h), Image.BILINEAR))


def predict_breastpathq(model, ep, dataset_path, label_csv_path, out_csv=None, batch=None, score=None, stain=None):
    """BreastPathQ submission table (reference utils/eval.py:354-412): every <image>_<region>.tif of the label file, in its row order,
    resized to (tile_h, tile_w), scored as the mean of `model.regressor` over the reference's four views and clamped to [0, 1];
    writes Ozan_Results_<ep>.csv (or `out_csv`) with the header slide,rid,p and returns the rows [(image id, region id, p)].
    The regions travel as u8: `batch` of them (default: what fills the engine's batch with four views each) are uploaded as one
    packed-RGB stack and scored through the u8 view path, the clamp inside wsi_mlp_views; a model without the fused heads gets the
    normalised fp32 batch and the module loop.  `score(u8 (B, tile_h, tile_w, 3) ndarray) -> B scores` replaces the scoring (tests).
    stain: a wsi_segmentation_pipeline_amd.stain.Normalizer; every uploaded u8 batch is stain-normalised on the device, each region fitted
    on itself, ahead of the view path (a region whose fit fails is scored as it is)."""
    import csv
    views = E.VIEWS_REFERENCE
    was_training = model.training if model is not None else False
    if score is None:
        dev = _device_of(model)
        model.eval()
        fused = _fused_head(model, 'regressor')
        if batch is None and fused:
            eng = model.encoder.net.hip_engine(dev)
            batch = getattr(eng, '_par', eng)._views_chunk(args.tile_h, args.tile_w, len(views))
        lut = torch.from_numpy(E.normalize_lut(args.dataset_mean, args.dataset_std)).to(dev)

        def score(u8):
            b, h, w, _ = u8.shape
            stack = S._upload(u8.reshape(b * h, w, 3), torch.uint8, dev)
            if stain is not None:
                stain.apply(stack.view(b, h, w, 3), out=stack.view(b, h, w, 3))
            xy = torch.zeros((b, 2), dtype=torch.int32, device=dev)
            xy[:, 1] = torch.arange(b, dtype=torch.int32, device=dev) * h
            if fused:
                out = model.regress_views(slide_u8=stack, tile_xy=xy, ph=h, pw=w, views=views, clamp=(0.0, 1.0))
            else:
                out = _score_views(model, 'regressor', views, clamp=(0.0, 1.0), x=E.tile_gather(stack, xy, h, w, lut))
            return out.reshape(-1).cpu().numpy()
    batch = int(batch) if batch else 64
    ids = breastpathq_rows(label_csv_path)
    rows = []
    with torch.no_grad():
        for i in range(0, len(ids), batch):
            part = ids[i:i + batch]
            u8 = np.stack([breastpathq_image(dataset_path, a, b) for a, b in part])
            p = np.asarray(score(u8), dtype=np.float32).reshape(-1)
            if p.shape[0] != len(part):
                raise ValueError('the scoring function returned %d scores for %d regions' % (p.shape[0], len(part)))
            rows.extend((a, b, v) for (a, b), v in zip(part, p))
    with open(out_csv if out_csv is not None else 'Ozan_Results_{}.csv'.format(ep), 'w', newline='') as f:
        writer = csv.DictWriter(f, fieldnames=['slide', 'rid', 'p'])
        writer.writeheader()
        for a, b, v in rows:
            writer.writerow({'slide': a, 'rid': b, 'p': v})
    if was_training:
        model.train()
    return rows
