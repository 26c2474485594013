"""Host side of the HIP inference path: weight prepack, workspaces and launch wrappers.

PyTorch is used only as plumbing (device memory, streams); all compute goes through
libwsi_hip.so (include/wsi_hip.h).  There is no CPU fallback: tensors must live on a GPU.
"""
import collections
import ctypes as C
import weakref

import numpy as np
import torch

from . import native

BN_EPS = 1e-5                                   # nn.BatchNorm2d default (reference resnets_shift.py:117)
PARITY, SPEED, MX = 2, 1, 3                     # planes: fp16 hi + fp16 lo pair (3 passes; r01-r04: bf16 pair) / single bf16 / fp16 + MX-fp6 cross terms
AUTO = 'auto'                                   # AutoTrunkEngine: mx unless a stratified two-mode probe of the slide says parity
# View ids (include/wsi_hip.h): transpose first if T, then reverse the rows of the result if FY, then its columns if FX.
VIEW_T, VIEW_FY, VIEW_FX = 1, 2, 4
VIEWS_REFERENCE = (0, 1, 2, 5)                  # image, transpose(2, 3), flip(2), transpose(2, 3).flip(3) (reference utils/eval.py:308-313)


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(st=None):
    return C.c_void_p((st or torch.cuda.current_stream()).cuda_stream)


def _np32(t):
    return np.ascontiguousarray(torch.as_tensor(t).detach().to('cpu', torch.float32).numpy())


def _f32(sd, key):
    return _np32(sd[key])


BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var')      # the four vectors of a BatchNorm, in the order every prepack entry takes them


def _bn(sd, prefix):
    return [_f32(sd, '%s.%s' % (prefix, s)) for s in BN_KEYS]


def _slide_args(slide):
    """(pointer, row pitch, height, width) of an optional (SH,SW,3) u8 slide, as the forward entries take them"""
    if slide is None:
        return None, 0, 0, 0
    return _ptr(slide), slide.stride(0), slide.shape[0], slide.shape[1]


def pack_conv(lib, w, bn, planes, tconv=False):
    """A conv weight (cout, cin, k, k) - or, with `tconv`, a ConvTranspose2d(c, c, 4, stride 2, padding 1) weight (c in, c out, 4, 4) as
    torch keeps it - with its BatchNorm folded in: fp32 numpy `w`, `bn` = [gamma, beta, mean, var] fp32 numpy or None -> (packed uint8
    array, bias fp32 array) as wsi_prepack_conv / wsi_prepack_tconv write them.  Host work only: no device, no engine."""
    w = np.ascontiguousarray(w, np.float32)
    if tconv:
        if w.ndim != 4 or w.shape[0] != w.shape[1] or w.shape[2:] != (4, 4):
            raise ValueError('expected a (c, c, 4, 4) transposed-conv weight, got %s' % (w.shape,))
        cout, dims, entry = w.shape[0], (w.shape[0],), 'wsi_prepack_tconv'
    else:
        cout, dims, entry = w.shape[0], w.shape[:3], 'wsi_prepack_conv'
    nbytes = getattr(lib, entry + '_bytes')(*dims, planes)
    if nbytes == 0:
        if tconv:
            raise ValueError('unsupported transposed-conv width %d for planes %d (a multiple of 64; planes 1 or 2)' % (cout, planes))
        raise ValueError('unsupported conv shape %s' % (w.shape,))
    bn = [] if bn is None else [np.ascontiguousarray(a, np.float32) for a in bn]
    pk, bias = np.empty(nbytes, np.uint8), np.empty(cout, np.float32)
    native.check(getattr(lib, entry)(_np_ptr(w), *([_np_ptr(a) for a in bn] or [None] * 4), BN_EPS, *dims, planes, _np_ptr(pk),
                                     _np_ptr(bias)), entry)
    return pk, bias


def normalize_lut(mean, std):
    """3x256 fp32 table of the eval transform (reference utils/preprocessing.py:209-212)."""
    lib = native.load()
    m = np.asarray(mean, np.float32)
    s = np.asarray(std, np.float32)
    out = np.empty((3, 256), np.float32)
    native.check(lib.wsi_normalize_u8_lut(_np_ptr(m), _np_ptr(s), _np_ptr(out)), 'wsi_normalize_u8_lut')
    return out


def _require_gpu(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('%s must be a GPU tensor: the WSI inference path runs on HIP kernels only '
                           '(no CPU fallback)' % what)


def batch_sizes(n, cap, h=256, w=256):
    """Batch sizes (each <= cap) for n images of h x w.  Several batches are sized in whole ROUNDS of the chip where that fits the
    cap: a batch of q = 512 * 256^2 / (h w) images gives every trunk launch a whole number of workgroup rounds (layer 4: one
    workgroup per 256^2-pixel image and channel block, 512 resident), so all batches but the last are multiples of q and the last
    takes the rest (24 648 tiles, cap 6 656: 3 x 6 144 + 6 216 - a 12.04-round launch runs 13 rounds; measured r03: +0.2 % on cfg3, inside the
    run-to-run noise - the nearly empty thirteenth round is short).
    Otherwise equal sizes without a short tail, as before."""
    n, cap = int(n), max(1, int(cap))
    k = max(1, -(-n // cap))
    if k == 1:
        return [n] if n else []
    q = max(1, 512 * 65536 // max(h * w, 1))
    base = int(round(n / k / q)) * q
    if base >= q and n - base * (k - 1) <= cap and n - base * (k - 1) > 0 and base <= cap:
        return [base] * (k - 1) + [n - base * (k - 1)]
    mb = -(-n // k)                                        # equal-sized batches: ceil(n / ceil(n / cap))
    return [min(mb, n - i) for i in range(0, n, mb)]


def view_ids(views):
    """The view list as 1 to 8 ints of 0 to 7 (repeats allowed); ValueError otherwise."""
    ids = [int(v) for v in views]
    if not 1 <= len(ids) <= 8 or any(not 0 <= v <= 7 for v in ids):
        raise ValueError('a view list has 1 to 8 ids of 0 to 7 (T = 1, FY = 2, FX = 4), got %r' % (views,))
    return ids


def view_groups(ids, h, w):
    """Positions of `ids` grouped by output shape: one group for square patches, else the untransposed and the transposed views."""
    if h == w:
        return [list(range(len(ids)))]
    return [g for g in ([k for k, v in enumerate(ids) if not v & VIEW_T], [k for k, v in enumerate(ids) if v & VIEW_T]) if g]


def _view_shape(ids, h, w):
    if h != w and len({v & VIEW_T for v in ids}) > 1:
        raise ValueError('views %r of a %d x %d patch have two shapes: pass the transposed and the untransposed ones separately' % (ids, h, w))
    return (w, h) if ids[0] & VIEW_T else (h, w)


def tile_views(slide_u8, tile_xy, ph, pw, views):
    """wsi_tile_views_u8: the views `views` of the n tiles of ph x pw at tile_xy (N,2) int32 of the (SH,SW,3) u8 slide -> (atlas,
    atlas_xy): an (V * n * hv, wv, 3) u8 "slide" of dense oriented tiles, view-major, and their corners (V * n, 2) int32 =
    (0, (k * n + i) * hv), ready for forward_tiles."""
    lib = native.load()
    _require_gpu(slide_u8, 'slide')
    _require_gpu(tile_xy, 'tile list')
    if slide_u8.dtype != torch.uint8 or slide_u8.dim() != 3 or slide_u8.shape[2] != 3 or slide_u8.stride(2) != 1 or slide_u8.stride(1) != 3:
        raise ValueError('slide must be (H,W,3) uint8 with packed RGB pixels')
    ids = view_ids(views)
    hv, wv = _view_shape(ids, ph, pw)
    tile_xy = tile_xy.to(torch.int32).contiguous()
    n = int(tile_xy.shape[0])
    rows = len(ids) * n
    atlas = torch.empty((rows * hv, wv, 3), dtype=torch.uint8, device=slide_u8.device)
    arr = (C.c_int * len(ids))(*ids)
    native.check(lib.wsi_tile_views_u8(_ptr(slide_u8), slide_u8.stride(0), slide_u8.shape[0], slide_u8.shape[1], _ptr(tile_xy), n, ph, pw,
                                       arr, len(ids), _ptr(atlas), _stream()), 'wsi_tile_views_u8')
    atlas_xy = torch.zeros((rows, 2), dtype=torch.int32, device=slide_u8.device)
    atlas_xy[:, 1] = torch.arange(rows, dtype=torch.int32, device=slide_u8.device) * hv
    return atlas, atlas_xy


def views_f32(x, views):
    """wsi_views_f32: (N,3,H,W) fp32 on the GPU -> the stacked views (V * N, 3, hv, wv), view-major."""
    lib = native.load()
    _require_gpu(x, 'input batch')
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError('expected (N,3,H,W), got %s' % (tuple(x.shape),))
    x = x.to(torch.float32).contiguous()
    ids = view_ids(views)
    n, _, h, w = x.shape
    hv, wv = _view_shape(ids, h, w)
    out = torch.empty((len(ids) * n, 3, hv, wv), dtype=torch.float32, device=x.device)
    arr = (C.c_int * len(ids))(*ids)
    native.check(lib.wsi_views_f32(_ptr(x), n, h, w, arr, len(ids), _ptr(out), _stream()), 'wsi_views_f32')
    return out


def mlp_views(feat, n, nviews, mlp, clamp=None, per_view=False):
    """wsi_mlp_views: feat (V * n, F) fp32 view-major -> (mean (n, K), per-view outputs (V * n, K) or None).  mlp = (w1, b1, w2, b2)
    (Regressor.fc: Linear, ReLU, Linear) or (w, b) (Classifier.fc: one Linear); clamp = (lo, hi) or None."""
    lib = native.load()
    _require_gpu(feat, 'features')
    feat = feat.to(torch.float32).contiguous()
    t = [torch.as_tensor(a).detach().to(feat.device, torch.float32).contiguous() for a in mlp]
    if len(t) == 4:
        w1, b1, w2, b2 = t
        j = int(w1.shape[0])
        ok = w1.dim() == 2 and w1.shape[1] == feat.shape[1] and b1.shape == (j,) and w2.dim() == 2 and w2.shape[1] == j
    elif len(t) == 2:
        (w2, b2), w1, b1, j = t, None, None, 0
        ok = w2.dim() == 2 and w2.shape[1] == feat.shape[1]
    else:
        raise ValueError('mlp is (w1, b1, w2, b2) or (w, b)')
    if not ok or b2.shape != (w2.shape[0],) or feat.dim() != 2 or feat.shape[0] != nviews * n:
        raise ValueError('mlp shapes do not match features %s of %d views x %d patches' % (tuple(feat.shape), nviews, n))
    k = int(w2.shape[0])
    mean = torch.empty((n, k), dtype=torch.float32, device=feat.device)
    pv = torch.empty((nviews * n, k), dtype=torch.float32, device=feat.device) if per_view else None
    lo, hi = (float(clamp[0]), float(clamp[1])) if clamp is not None else (0.0, 0.0)
    native.check(lib.wsi_mlp_views(_ptr(feat), n, nviews, int(feat.shape[1]), _ptr(w1), _ptr(b1), j, _ptr(w2), _ptr(b2), k,
                                   int(clamp is not None), lo, hi, _ptr(pv), _ptr(mean), _stream()), 'wsi_mlp_views')
    return mean, pv


# What the host layer knows of an architecture: convs per block and their kernel sizes, the width factor of a block's output, the first
# layer whose block 0 has a downsample branch (slot 0 of the C struct's down_w / down_b), the C struct, the prefix of its entry points
# (include/wsi_hip.h) and the planes values its kernels take.
Arch = collections.namedtuple('Arch', 'convs ksizes expansion first_down weights entry planes_ok')
ARCHS = {'basic': Arch(2, (3, 3), 1, 2, native.WsiTrunkWeights, 'wsi_trunk', (1, 2, 3)),
         'bottleneck': Arch(3, (1, 3, 1), 4, 1, native.WsiBneckWeights, 'wsi_bneck', (1, 2))}


def _block_keys(state_dict):
    """(key, layer 1..4, block, rest of the key as a list) of every ``layerL.B.<...>`` key; ValueError for a layer outside 1..4."""
    for key in state_dict:
        parts = key.split('.')
        if len(parts) < 4 or not parts[0].startswith('layer') or not parts[0][5:].isdigit() or not parts[1].isdigit():
            continue
        L = int(parts[0][5:])
        if not 1 <= L <= 4:
            raise ValueError('state dict key %r: a ResNet trunk has layer1 ... layer4' % key)
        yield key, L, int(parts[1]), parts[2:]


def trunk_arch(state_dict):
    """('basic' | 'bottleneck', blocks per stage) of a ResNet state dict with the reference's key names: the count of
    ``layerL.B.conv1.weight`` keys per layer.  A trunk whose every block has a ``conv3`` key is a Bottleneck net (ResNet-50:
    [3, 4, 6, 3], ResNet-101: [3, 4, 23, 3]), one without any is a BasicBlock net ([2, 2, 2, 2] for ResNet-18, [3, 4, 6, 3] for
    ResNet-34); ValueError for a mixture, for gaps in the block numbers, for a stage without blocks and for more than
    native.TRUNK_MAX_BLOCKS blocks (ResNet-152 has 50)."""
    found = [set(), set(), set(), set()]
    third = [set(), set(), set(), set()]
    for _, L, B, rest in _block_keys(state_dict):
        if rest == ['conv1', 'weight']:
            found[L - 1].add(B)
        if rest == ['conv3', 'weight']:
            third[L - 1].add(B)
    if any(third) and third != found:
        raise ValueError('state dict mixes blocks with and without conv3 (blocks with conv1: %s, with conv3: %s): neither a BasicBlock '
                         'nor a Bottleneck ResNet' % ([sorted(b) for b in found], [sorted(b) for b in third]))
    layers = []
    for L, blocks in enumerate(found, start=1):
        if not blocks:
            raise ValueError('state dict has no layer%d.0.conv1.weight: not a ResNet trunk' % L)
        if blocks != set(range(len(blocks))):
            raise ValueError('state dict has gaps in the blocks of layer%d: found %s' % (L, sorted(blocks)))
        layers.append(len(blocks))
    if sum(layers) > native.TRUNK_MAX_BLOCKS:
        raise ValueError('%s = %d blocks: the C ABI carries at most %d (include/wsi_hip.h WSI_TRUNK_MAX_BLOCKS; ResNet-152 is not '
                         'supported)' % (layers, sum(layers), native.TRUNK_MAX_BLOCKS))
    return ('bottleneck' if any(third) else 'basic'), layers


def trunk_layers(state_dict):
    """Blocks per stage of a BasicBlock ResNet state dict, e.g. [2, 2, 2, 2] for ResNet-18 and [3, 4, 6, 3] for ResNet-34: `trunk_arch`
    with a ValueError of its own for a Bottleneck checkpoint (any ``conv3`` key)."""
    for key, _, _, rest in _block_keys(state_dict):
        if rest[0] == 'conv3':
            raise ValueError('state dict key %r belongs to a Bottleneck block (ResNet-50 and deeper): the HIP trunk runs BasicBlock '
                             'ResNets (resnet18, resnet34, any [n1, n2, n3, n4] of two-conv blocks) only' % key)
    return trunk_arch(state_dict)[1]


def conv_table(arch, layers):
    """The conv tables of a net's C struct, from the state dict's side: ([(index, weight key, bn prefix, kernel size)] in network order,
    the index block-major as include/wsi_hip.h states it; [(downsample slot, weight key, bn prefix)])."""
    a = ARCHS[arch]
    convs, downs = [], []
    for L in range(1, 5):
        for B in range(layers[L - 1]):
            for K, ksize in enumerate(a.ksizes, start=1):
                convs.append((a.convs * (sum(layers[:L - 1]) + B) + (K - 1), 'layer%d.%d.conv%d.weight' % (L, B, K),
                              'layer%d.%d.bn%d' % (L, B, K), ksize))
        if L >= a.first_down:
            downs.append((L - a.first_down, 'layer%d.0.downsample.0.weight' % L, 'layer%d.0.downsample.1' % L))
    return convs, downs


def tap_shape(arch, layers, tap, h, w):
    """(channels, height, width) of tap `tap` (0 = pool, 1.. = blocks in network order) of an h x w input."""
    stage = sum(tap > sum(layers[:L]) for L in range(4))                   # 0 = pool, 1..4 = layer of block `tap`
    if stage == 0:
        return 64, h >> 2, w >> 2
    return (64 << (stage - 1)) * ARCHS[arch].expansion, h >> (1 + stage), w >> (1 + stage)


class TrunkEngine:
    """BasicBlock ResNet trunk (stem + layer1..4; ResNet-18, ResNet-34 or any other depth: `trunk_layers`) of the reference
    ``resnets_shift.ResNet`` on HIP kernels, with an optional Linear(512->K) head fused after the average pool (``fc0`` or
    ``Classifier``).

    state_dict: reference key names (conv1.weight, bn1.*, layerL.B.convK.weight, ...); the depth is read from it (`.layers`).
    """

    ARCH = 'basic'                               # the row of ARCHS this engine runs
    FEAT_C = 512 * ARCHS[ARCH].expansion         # channels of the last stage (the head's input width)
    PLANES_OK = ARCHS[ARCH].planes_ok

    def __init__(self, state_dict, device, planes=MX, head=None, max_batch=None,
                 mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), streams=2):
        self.lib = native.load()
        arch = ARCHS[self.ARCH]
        self._ws_bytes, self._ws_init, self._forward, self._forward_tap = (
            getattr(self.lib, arch.entry + s) for s in ('_workspace_bytes', '_workspace_init', '_forward', '_forward_tap'))
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('TrunkEngine needs a GPU device, got %s' % device)
        if planes not in (1, 2, 3):
            raise ValueError('planes must be 1 (speed), 2 (parity, fp16 pair) or 3 (mx, fp16 + MX-fp6)')
        if planes not in self.PLANES_OK:
            raise NotImplementedError('%s has no mx mode (planes 3): there is no pointwise-conv kernel in that mode; use parity (2) '
                                      'or speed (1)' % type(self).__name__)
        self.planes = planes
        # images per trunk call; None = the tuned size (6200 patches of 256 x 256, scaled by patch area: what bench.py measures) as far
        # as the free HBM allows - the workspace is ~8.3 MB per 256 x 256 patch, one per stream slot (`_auto_cap`; r01-r04: 2000 and
        # one stream, i.e. a caller of the drop-in modules did not get the benchmarked configuration)
        self.max_batch = None if max_batch is None else int(max_batch)
        # batches of one call are spread round-robin over `streams` HIP streams (own workspace each), so a
        # memory-bound stage of one batch overlaps an MFMA-bound stage of another and grid tails get filled
        self._streams = [torch.cuda.Stream(device=self.device) for _ in range(max(1, int(streams)))] if streams > 1 else []
        self._keep = []                          # device tensors referenced by raw pointers
        self._ws = {}
        self.wt = arch.weights()
        self.wt.planes = planes
        sd = state_dict
        self.layers = self._layers_of(sd)
        for L in range(4):
            self.wt.blocks[L] = self.layers[L]

        def dev(a):
            t = torch.from_numpy(a).to(self.device)
            self._keep.append(t)
            return t

        # stem
        w = _f32(sd, 'conv1.weight')
        pk = np.empty(self.lib.wsi_prepack_stem_bytes(planes), np.uint8)
        bias = np.empty(64, np.float32)
        g, b, m, v = _bn(sd, 'bn1')
        native.check(self.lib.wsi_prepack_stem(_np_ptr(w), _np_ptr(g), _np_ptr(b), _np_ptr(m), _np_ptr(v), BN_EPS,
                                               planes, _np_ptr(pk), _np_ptr(bias)), 'wsi_prepack_stem')
        self.wt.stem_w = dev(pk).data_ptr()
        self.wt.stem_b = dev(bias).data_ptr()
        if planes >= 2:                          # u8 slide input: transform folded into the weights (exact integer pixels)
            pk8 = np.empty(self.lib.wsi_prepack_stem_bytes(2), np.uint8)
            bias8 = np.empty(64, np.float32)
            mean_a, std_a = np.asarray(mean, np.float32), np.asarray(std, np.float32)
            native.check(self.lib.wsi_prepack_stem_u8(_np_ptr(w), _np_ptr(g), _np_ptr(b), _np_ptr(m), _np_ptr(v), BN_EPS,
                                                      _np_ptr(mean_a), _np_ptr(std_a), planes, _np_ptr(pk8), _np_ptr(bias8)),
                         'wsi_prepack_stem_u8')
            self.wt.stem_w_u8 = dev(pk8).data_ptr()
            self.wt.stem_b_u8 = dev(bias8).data_ptr()
            for i in range(3):
                self.wt.norm[i], self.wt.norm[3 + i] = float(mean_a[i]), float(std_a[i])

        def conv(wkey, bnkey, k):
            w = _f32(sd, wkey)
            if w.shape[2] != k:
                raise ValueError('%s: expected a %d x %d conv, got %s' % (wkey, k, k, w.shape))
            pk, bias = pack_conv(self.lib, w, _bn(sd, bnkey), planes)
            return dev(pk).data_ptr(), dev(bias).data_ptr()

        convs, downs = conv_table(self.ARCH, self.layers)
        for i, wkey, bnkey, k in convs:
            self.wt.conv_w[i], self.wt.conv_b[i] = conv(wkey, bnkey, k)
        for i, wkey, bnkey in downs:
            self.wt.down_w[i], self.wt.down_b[i] = conv(wkey, bnkey, 1)
        self.set_head(head)
        self.lut = dev(normalize_lut(mean, std))

    def _layers_of(self, sd):
        if self.ARCH == 'basic':
            return trunk_layers(sd)                         # (refuses a Bottleneck checkpoint in its own words)
        arch, layers = trunk_arch(sd)
        if arch != self.ARCH:
            raise ValueError('BottleneckEngine needs a Bottleneck state dict (layerL.B.conv3 keys); this one is a BasicBlock net: use TrunkEngine')
        return layers

    def _tap_shape(self, tap, h, w):
        return tap_shape(self.ARCH, self.layers, tap, h, w)

    # ------------------------------------------------------------------ configuration
    def set_head(self, head):
        """head = (weight (K, FEAT_C), bias (K,)) tensors/arrays or None (FEAT_C = 512; Bottleneck nets: 2048)."""
        if head is None:
            self.wt.head_w, self.wt.head_b, self.wt.head_k = None, None, 0
            self.head_k = 0
            return
        w = torch.as_tensor(head[0]).detach().to(self.device, torch.float32).contiguous()
        b = torch.as_tensor(head[1]).detach().to(self.device, torch.float32).contiguous()
        if w.dim() != 2 or w.shape[1] != self.FEAT_C or b.shape[0] != w.shape[0]:
            raise ValueError('head must be Linear(%d -> K)' % self.FEAT_C)
        self._head = (w, b)
        self.wt.head_w, self.wt.head_b, self.wt.head_k = w.data_ptr(), b.data_ptr(), int(w.shape[0])
        self.head_k = int(w.shape[0])

    def _workspace(self, n, h, w, slot=0):
        """(workspace, capacity): one workspace per (patch shape, stream slot), planned for the largest batch seen so far; it
        serves every smaller batch as is (wsi_trunk_forward's workspace_n), so ragged last batches and variable bag
        counts neither allocate nor re-zero ~8 MB per patch."""
        key = (h, w, slot)
        ent = self._ws.get(key)
        if ent is None or ent[1] < n:
            nbytes = self._ws_bytes(n, h, w, self.planes)
            if nbytes == 0:
                raise ValueError('unsupported patch shape %dx%d (need multiples of 32) or batch %d' % (h, w, n))
            self._drop_workspace(key)                       # a smaller plan of the same shape is released first
            if len(self._ws) >= 4 * max(1, len(self._streams)):   # keep the plan cache small
                self._drop_workspace(next(iter(self._ws)))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            native.check(self._ws_init(_ptr(ws), n, h, w, self.planes, _stream()), self._ws_init.__name__)
            ent = self._ws[key] = (ws, n)
        return ent

    def _drop_workspace(self, key):
        ent = self._ws.pop(key, None)
        if ent is not None:                                 # the library forgets the address before the allocator can reuse it (a no-op for
                                                            # a Bottleneck workspace, which carries no layout tag)
            self.lib.wsi_trunk_workspace_release(_ptr(ent[0]))

    def release_workspaces(self):
        """Free every planned workspace (they are re-planned on the next forward)."""
        for key in list(self._ws):
            self._drop_workspace(key)

    def __del__(self):
        try:
            for key in list(getattr(self, '_ws', {})):
                self._drop_workspace(key)
        except Exception:                                   # interpreter shutdown: the library may be gone
            pass

    # ------------------------------------------------------------------ forward passes
    def _run(self, n, h, w, in_f32, slide, tile_xy, want_feat, want_logits, want_fmap, tap=None, slot=0):
        ws, cap = self._workspace(n, h, w, slot)
        dev = self.device
        feat = torch.empty((n, self.FEAT_C), dtype=torch.float32, device=dev) if want_feat else None
        logits = torch.empty((n, self.head_k), dtype=torch.float32, device=dev) if want_logits else None
        fmap = torch.empty((n, self.FEAT_C, h // 32, w // 32), dtype=torch.float32, device=dev) if want_fmap else None
        sp, pitch, sh, sw = _slide_args(slide)
        if tap is not None:
            if not 0 <= tap <= sum(self.layers):
                raise ValueError('tap must be 0 (pool) ... %d (the last block), got %r' % (sum(self.layers), tap))
            c, hh, ww = self._tap_shape(tap, h, w)
            out = torch.empty((n, c, hh, ww), dtype=torch.float32, device=dev)
            native.check(self._forward_tap(C.byref(self.wt), _ptr(in_f32), sp, pitch, sh, sw, _ptr(tile_xy), _ptr(self.lut), n, h, w,
                                           _ptr(ws), cap, tap, _ptr(out), _stream()), self._forward_tap.__name__)
            return out
        native.check(self._forward(C.byref(self.wt), _ptr(in_f32), sp, pitch, sh, sw, _ptr(tile_xy), _ptr(self.lut), n, h, w, _ptr(ws), cap,
                                   _ptr(feat), _ptr(logits), _ptr(fmap), _stream()), self._forward.__name__)
        return feat, logits, fmap

    def forward_f32(self, x, feat=False, logits=False, fmap=False, tap=None):
        """x: (N,3,H,W) normalised fp32 on the GPU.  Returns (feat, logits, fmap) (None where not asked)."""
        _require_gpu(x, 'input batch')
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError('expected (N,3,H,W), got %s' % (tuple(x.shape),))
        if logits and not self.head_k:
            raise RuntimeError('no head set')
        x = x.to(torch.float32).contiguous()
        n, _, h, w = x.shape
        if tap is not None:
            return self._run(n, h, w, x, None, None, False, False, False, tap)
        return self._batched(n, lambda i, m, slot: self._run(m, h, w, x[i:i + m], None, None, feat, logits, fmap, slot=slot), h, w)

    def forward_tiles(self, slide_u8, tile_xy, ph, pw, feat=False, logits=True, fmap=False, tap=None):
        """slide_u8: (SH,SW,3) uint8 GPU tensor (last two dims contiguous); tile_xy: (N,2) int32 GPU tensor of
        top-left corners in slide pixels.  Tile read + transform are fused into the stem kernel."""
        _require_gpu(slide_u8, 'slide')
        _require_gpu(tile_xy, 'tile list')
        if slide_u8.dtype != torch.uint8 or slide_u8.dim() != 3 or slide_u8.shape[2] != 3 or slide_u8.stride(2) != 1 \
                or slide_u8.stride(1) != 3:
            raise ValueError('slide must be (H,W,3) uint8 with packed RGB pixels')
        if logits and not self.head_k:
            raise RuntimeError('no head set')
        tile_xy = tile_xy.to(torch.int32).contiguous()
        n = tile_xy.shape[0]
        if tap is not None:
            return self._run(n, ph, pw, None, slide_u8, tile_xy, False, False, False, tap)
        return self._batched(n, lambda i, m, slot: self._run(m, ph, pw, None, slide_u8, tile_xy[i:i + m], feat, logits, fmap,
                                                             slot=slot), ph, pw)

    TUNED_BATCH_256 = 6200                                   # images of 256 x 256 per trunk call (bench.py --batch default)

    def _auto_cap(self, h, w):
        """Default images per trunk call: the tuned batch scaled by patch area, limited so that the workspaces of all stream slots
        stay inside 60 % of the memory that is free now (plus what this engine already holds)."""
        want = max(1, int(self.TUNED_BATCH_256 * 65536 // max(h * w, 1)))
        per = self._ws_bytes(64, h, w, self.planes) / 64.0
        if per <= 0:
            return want
        try:                                                 # free = what the driver reports + what torch's caching allocator holds unused
            free = torch.cuda.mem_get_info(self.device)[0] + max(0, torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device))
        except Exception:
            return want
        held = sum(int(ws.numel()) for ws, _ in self._ws.values())
        slots = max(1, len(self._streams))
        return max(1, min(want, int(0.6 * (free + held) / (slots * per))))

    def _batched(self, n, run, h=256, w=256):
        """Split n images into max_batch chunks; with several chunks, alternate them over the side streams."""
        cap = self.max_batch if self.max_batch else self._auto_cap(h, w)
        sizes = batch_sizes(n, cap, h, w)
        starts = [sum(sizes[:j]) for j in range(len(sizes))]
        if len(sizes) > 1:                                  # plan every slot's workspace for the largest batch once (the last one)
            for slot in range(max(1, len(self._streams)) if self._streams else 1):
                self._workspace(max(sizes), h, w, slot)
        if len(starts) == 1 or not self._streams:
            outs = [run(i, m, 0) for i, m in zip(starts, sizes)]
        else:
            cur = torch.cuda.current_stream()
            ready = torch.cuda.Event()
            ready.record(cur)
            outs = []
            for j, i in enumerate(starts):
                st = self._streams[j % len(self._streams)]
                st.wait_event(ready)
                with torch.cuda.stream(st):
                    outs.append(run(i, sizes[j], j % len(self._streams)))
            for st in self._streams:
                cur.wait_stream(st)
            for o in outs:                                  # tensors were allocated on side streams
                for t in o:
                    if t is not None:
                        t.record_stream(cur)
        return tuple(None if o[0] is None else (o[0] if len(o) == 1 else torch.cat(o)) for o in zip(*outs))

    # ------------------------------------------------------------------ test-time views
    def _views_input(self, x, slide_u8, tile_xy, ph, pw):
        """(n, h, w) of a forward_views input: either x (N,3,H,W) fp32 or a u8 slide with tile corners and the patch shape."""
        if (x is None) == (slide_u8 is None):
            raise ValueError('forward_views takes either x= or slide_u8=, tile_xy=, ph=, pw=')
        if x is not None:
            _require_gpu(x, 'input batch')
            if x.dim() != 4 or x.shape[1] != 3:
                raise ValueError('expected (N,3,H,W), got %s' % (tuple(x.shape),))
            return int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
        if tile_xy is None or ph is None or pw is None:
            raise ValueError('the u8 path needs tile_xy, ph and pw')
        _require_gpu(slide_u8, 'slide')
        _require_gpu(tile_xy, 'tile list')
        return int(tile_xy.shape[0]), int(ph), int(pw)

    def _views_chunk(self, h, w, nviews):
        """Patches per chunk of forward_views: all views of a patch in one chunk, V * chunk within the trunk's batch."""
        cap = self.max_batch if self.max_batch else self._auto_cap(h, w)
        return max(1, cap // nviews)

    def views_features(self, ids, x, slide_u8, tile_xy, h, w):
        """Pooled features (V * m, FEAT_C), view-major, of the views `ids` of m patches: the view producer, then the existing
        forward with feat=True.  Non-square patches: one trunk pass for the untransposed and one for the transposed views, the
        features put back in view order."""
        groups = view_groups(ids, h, w)
        m = int(x.shape[0]) if x is not None else int(tile_xy.shape[0])
        parts = [None] * len(ids)
        for g in groups:
            gv = [ids[k] for k in g]
            if x is not None:
                f = self.forward_f32(views_f32(x, gv), feat=True)[0]
            else:
                atlas, axy = tile_views(slide_u8, tile_xy, h, w, gv)
                hv, wv = _view_shape(gv, h, w)
                f = self.forward_tiles(atlas, axy, hv, wv, feat=True, logits=False)[0]
            if len(groups) == 1:
                return f
            for i, k in enumerate(g):
                parts[k] = f[i * m:(i + 1) * m]
        return torch.cat(parts)

    def forward_views(self, x=None, slide_u8=None, tile_xy=None, ph=None, pw=None, views=VIEWS_REFERENCE, mlp=None, clamp=None,
                      per_view=False):
        """The reference's test-time augmentation loop (utils/eval.py:307-336, :391-410) on the HIP path: the views `views` of every
        patch - x (N,3,H,W) normalised fp32, or the N tiles of ph x pw at tile_xy of a u8 slide - through the trunk, the MLP head
        `mlp` = (w1, b1, w2, b2) or (w, b) over the pooled features of every view, and their mean over the views (wsi_mlp_views),
        clamped to `clamp` = (lo, hi) if given.  Returns mean (N, K); with per_view, (mean, outputs (N, V, K))."""
        if mlp is None:
            raise ValueError('forward_views needs mlp=(w1, b1, w2, b2) or (w, b)')
        n, h, w = self._views_input(x, slide_u8, tile_xy, ph, pw)
        ids = view_ids(views)
        step = self._views_chunk(h, w, len(ids))
        means, pvs = [], []
        for i in range(0, n, step):
            m = min(step, n - i)
            f = self.views_features(ids, None if x is None else x[i:i + m], slide_u8, None if tile_xy is None else tile_xy[i:i + m], h, w)
            mean, pv = mlp_views(f, m, len(ids), mlp, clamp, per_view)
            means.append(mean)
            if per_view:
                pvs.append(pv.view(len(ids), m, -1).permute(1, 0, 2))
        if not means:
            raise ValueError('forward_views needs at least one patch')
        mean = means[0] if len(means) == 1 else torch.cat(means)
        if not per_view:
            return mean
        return mean, (pvs[0] if len(pvs) == 1 else torch.cat(pvs)).contiguous()

    # ------------------------------------------------------------------ small ops
    def linear(self, x, weight, bias, relu=False):
        _require_gpu(x, 'linear input')
        x = x.to(torch.float32).contiguous()
        weight = weight.detach().to(self.device, torch.float32).contiguous()
        bias = bias.detach().to(self.device, torch.float32).contiguous() if bias is not None else None
        y = torch.empty((x.shape[0], weight.shape[0]), dtype=torch.float32, device=self.device)
        native.check(self.lib.wsi_linear(_ptr(x), _ptr(weight), _ptr(bias), _ptr(y), x.shape[0], x.shape[1],
                                         weight.shape[0], int(relu), _stream()), 'wsi_linear')
        return y


class BottleneckEngine(TrunkEngine):
    """Bottleneck ResNet trunk (ResNet-50, ResNet-101, any [n1, n2, n3, n4] of three-conv blocks up to native.TRUNK_MAX_BLOCKS in all) of
    the reference ``resnets_shift.ResNet(Bottleneck, layers)`` on HIP kernels: wsi_bneck_forward, whose 1x1 convs run on the
    pointwise kernel.  Same surface as TrunkEngine; features and heads are 2048 wide; planes 2 (parity) or 1 (speed) - mx is refused.
    `_auto_cap` sizes the batch from wsi_bneck_workspace_bytes (30.8 MB per 256 x 256 patch in parity mode)."""
    ARCH = 'bottleneck'
    FEAT_C = 512 * ARCHS[ARCH].expansion
    PLANES_OK = ARCHS[ARCH].planes_ok


class AutoTrunkEngine:
    """TrunkEngine that picks its precision mode per checkpoint AND data, so a caller cannot silently leave the 1e-3 logit
    contract (BASELINE.json north_star).  mx (fp16 + MX-fp6 cross terms) is ~1.35x faster than parity (bf16x2 split); both
    hold the contract on every reference-generated weight / input family (tests/test_gpu_margin.py: mx <= 6.3e-4, parity
    <= 4.0e-4 at |logit| = 16), but every finite-precision error grows with the logit magnitude, so the choice is guarded:
      * at load: the folded weights must be representable (finite, inside the fp16 range) or mx is refused outright;
      * per slide (forward_tiles) / per head (forward_f32): `probe` images - a STRATIFIED sample over the whole tile list,
        never its first tiles: a slide's first raster tiles are one corner of the tissue - run in BOTH modes; |mx - parity|
        on the head logits (without a head: on the pooled features relative to their size) decides: mx if <= `tol`
        (default 5e-4: half the contract), parity otherwise;
      * with several ranks the decision must be ONE decision: callers that shard a slide (slide.infer_slide_cls) take the
        local `probe_tiles` error, all-reduce its maximum and hand it to `decide`, so no rank mixes modes into a gathered map.
    The decision and the measured value are kept in `.report` (utils.eval.predict_tumorbed returns it per slide)."""

    def __init__(self, state_dict, device, head=None, tol=5e-4, probe=32, **kw):
        self._kw = dict(kw)
        self._sd, self._dev, self.tol, self.probe = state_dict, device, float(tol), int(probe)
        self.report = {'mode': None, 'reason': 'not probed yet', 'probe_error': None}
        self._par = TrunkEngine(state_dict, device, planes=PARITY, head=head, **kw)
        self._mx = None
        reason = self._static_check(state_dict)
        if reason is None:
            self._mx = TrunkEngine(state_dict, device, planes=MX, head=head, **kw)
        else:
            self.report = {'mode': 'parity', 'reason': reason, 'probe_error': None}
        self._chosen = None if self._mx is not None else self._par
        self._slide_key, self._slide_ref, self._probed = None, None, None

    @staticmethod
    def _static_check(sd):
        """mx needs every BN-folded conv weight finite and well inside the fp16 range."""
        for key, w in sd.items():
            if not key.endswith('.weight') or getattr(w, 'dim', lambda: 0)() != 4:
                continue
            bn = key.replace('conv1.weight', 'bn1.weight').replace('conv2.weight', 'bn2.weight').replace('downsample.0.weight', 'downsample.1.weight')
            scale = 1.0
            if bn != key and bn in sd:
                var = sd[bn.replace('.weight', '.running_var')].detach().to('cpu', torch.float64)
                scale = (sd[bn].detach().to('cpu', torch.float64) / torch.sqrt(var + BN_EPS)).abs().max().item()
            m = float(w.detach().abs().max()) * scale
            if not np.isfinite(m) or m > 3.0e4:
                return 'folded weights of %s reach %.3g (outside the fp16 range of the mx mode)' % (key, m)
        return None

    # the TrunkEngine surface
    @property
    def planes(self):
        return (self._chosen or self._mx or self._par).planes

    @property
    def head_k(self):
        return self._par.head_k

    @property
    def lut(self):
        return self._par.lut

    def set_head(self, head):
        self._par.set_head(head)
        if self._mx is not None:
            self._mx.set_head(head)
            self._chosen = None                               # a new head changes the logit scale: probe again

    def linear(self, *a, **k):
        return self._par.linear(*a, **k)

    def reset(self):
        """Forget the decision: the next forward (or probe_tiles / decide pair) probes again."""
        if self._mx is not None:
            self._chosen, self._slide_key, self._slide_ref = None, None, None

    def _key_of(self, slide_u8, slide_id):
        """Identity of a slide for the one-decision-per-slide rule.  A caller-supplied `slide_id` (any hashable) wins; without one
        the slide is the TENSOR OBJECT the caller passes (held by weak reference), never its address: the caching allocator hands a
        new slide of the same shape the block the previous one just freed, and a (data_ptr, shape) key would then silently reuse the
        previous slide's mode without a probe."""
        if slide_id is not None:
            return ('id', slide_id)
        return ('obj', id(slide_u8))

    def _same_slide(self, slide_u8, key):
        if key != self._slide_key:
            return False
        if key[0] == 'id':
            return True
        ref = self._slide_ref
        return ref is not None and ref() is slide_u8            # a dead or different object with a recycled id() is a new slide

    def _stratified(self, total):
        n = min(self.probe, int(total))
        return torch.linspace(0, max(int(total) - 1, 0), n, device=self._dev).round().long()

    def _probe(self, run):
        """run(engine) -> (feat, logits, fmap) on the probe images.  Returns (error, what, n): |mx - parity| as described above."""
        fm, lm, _ = run(self._mx)
        fp, lp, _ = run(self._par)
        if lm is not None:
            return float((lm - lp).abs().max()), 'max |logit_mx - logit_parity|', int(lp.shape[0])
        return (float((fm - fp).abs().max() / fp.abs().max().clamp_min(1e-30)) * 2.0, '2 x max |feat_mx - feat_parity| / max |feat|',
                int(fp.shape[0]))

    def probe_tiles(self, slide_u8, tile_xy, ph, pw, slide_id=None):
        """Local probe error of mx on a stratified sample of `tile_xy` (0.0 without tiles or without an mx engine); the caller
        all-reduces the maximum over its ranks and calls decide().  The slide probed here is the slide the following decide()
        fixes the mode for: forward_tiles on it (same tensor object, or same `slide_id`) does not probe again."""
        self._probed = (self._key_of(slide_u8, slide_id), weakref.ref(slide_u8))
        if self._mx is None or int(tile_xy.shape[0]) == 0:
            return 0.0
        xy = tile_xy[self._stratified(tile_xy.shape[0])].contiguous()
        err, self._what, self._n = self._probe(lambda e: e.forward_tiles(slide_u8, xy, ph, pw, feat=True, logits=bool(e.head_k)))
        return err

    def probe_f32(self, x):
        """probe_tiles for the tensor-input path: local probe error on a stratified sample of the batch x (N, 3, H, W)."""
        if self._mx is None or int(x.shape[0]) == 0:
            return 0.0
        idx = self._stratified(x.shape[0])
        err, self._what, self._n = self._probe(lambda e: e.forward_f32(x[idx], feat=True, logits=bool(e.head_k)))
        return err

    def decide(self, err, scope='slide'):
        """Fix the mode for the coming forwards from a (rank-global) probe error.  After a probe_tiles() the decision belongs to
        THAT slide (r03 advisor finding: decide() used to leave the previous slide's key in place, so the first forward_tiles of
        every slide but the first probed again locally and could override the all-reduced decision on some ranks only)."""
        probed, self._probed = getattr(self, '_probed', None), None
        if probed is not None:
            self._slide_key, self._slide_ref = probed
        if self._mx is None:
            return
        ok = bool(np.isfinite(err)) and err <= self.tol
        self._chosen = self._mx if ok else self._par
        self.report = {'mode': 'mx' if ok else 'parity', 'probe_error': float(err), 'scope': scope,
                       'reason': '%s = %.2e %s tol %.1e on %d stratified probe images' %
                                 (getattr(self, '_what', 'probe error'), err, '<=' if ok else '>', self.tol, getattr(self, '_n', 0))}

    def forward_tiles_verified(self, slide_u8, tile_xy, ph, pw, reduce_max=None):
        """One slide (or one rank's shard of it), mx FIRST and checked afterwards: the whole tile list runs in mx, the stratified sample of
        probe_tiles once more in parity, and max |logit_mx - logit_parity| on the sample - reduced over the ranks by `reduce_max` (a
        collective: every rank must call, shards without tiles contribute 0) - decides whether the mx logits stand or the list is run
        again in parity.  Same sample, same rule and same report as probe_tiles + decide, but the mx forward of the sample and the host
        synchronisation BEFORE the slide's main pass are gone (r05: the drop-in API ran 3-4 % behind the bare engine); the price is a
        second pass over the slide in the rare case the answer is 'parity'.  Needs a head (logits).  Returns (feat=None, logits, None)."""
        n = int(tile_xy.shape[0])
        if self._mx is None:                                  # (the static weight check refused mx: report says why)
            if reduce_max is not None:
                reduce_max(0.0)                               # the other ranks' collective
            self.report['order'] = 'parity only'
            return self._par.forward_tiles(slide_u8, tile_xy, ph, pw, logits=True) if n else \
                (None, torch.zeros((0, self.head_k), dtype=torch.float32, device=tile_xy.device), None)
        out = self._mx.forward_tiles(slide_u8, tile_xy, ph, pw, logits=True) if n else None
        err, nprobe = 0.0, 0
        if n:
            idx = self._stratified(n)
            lp = self._par.forward_tiles(slide_u8, tile_xy[idx].contiguous(), ph, pw, logits=True)[1]
            err, nprobe = float((out[1][idx] - lp).abs().max()), int(idx.shape[0])
        if reduce_max is not None:
            err = float(reduce_max(err))
        self._what, self._n = 'max |logit_mx - logit_parity|', nprobe
        self._probed = None
        self.decide(err)
        self.report['order'] = 'mx first, verified on the sample afterwards'
        if self._chosen is self._par and n:
            out = self._par.forward_tiles(slide_u8, tile_xy, ph, pw, logits=True)
        if out is None:
            out = (None, torch.zeros((0, self.head_k), dtype=torch.float32, device=tile_xy.device), None)
        return out

    def forward_f32(self, x, feat=False, logits=False, fmap=False, tap=None):
        if self._chosen is None:
            self.decide(self.probe_f32(x), scope='head')
        return self._chosen.forward_f32(x, feat=feat, logits=logits, fmap=fmap, tap=tap)

    def forward_tiles(self, slide_u8, tile_xy, ph, pw, feat=False, logits=True, fmap=False, tap=None, slide_id=None):
        # one decision per slide: a slide this engine has not decided for (or a reset) probes first; chunks of the same slide - the
        # same tensor object or the same caller-supplied slide_id - reuse the decision, including one made by probe_tiles + decide
        key = self._key_of(slide_u8, slide_id)
        if self._mx is not None and (self._chosen is None or not self._same_slide(slide_u8, key)):
            self.decide(self.probe_tiles(slide_u8, tile_xy, ph, pw, slide_id=slide_id))
        return self._chosen.forward_tiles(slide_u8, tile_xy, ph, pw, feat=feat, logits=logits, fmap=fmap, tap=tap)


    def forward_views(self, x=None, slide_u8=None, tile_xy=None, ph=None, pw=None, views=VIEWS_REFERENCE, **kw):
        """TrunkEngine.forward_views in the mode decided ONCE: without a decision, the views of the first chunk are probed in both
        modes on the pooled features (the feature-relative probe, whatever fused head is set: the MLP reads the features), under the
        constant slide id 'forward_views' - every call builds a new atlas tensor, which must not probe again.  The decision holds
        until reset()."""
        if self._mx is not None and self._chosen is None:
            n, h, w = self._par._views_input(x, slide_u8, tile_xy, ph, pw)
            ids = view_ids(views)
            m = min(n, self._par._views_chunk(h, w, len(ids)))
            idx = self._stratified(m)                         # a stratified sample of the chunk's patches, all their views
            sub = None if x is None else x[:m][idx]
            xy = None if tile_xy is None else tile_xy[:m][idx].contiguous()
            run = lambda e: (e.views_features(ids, sub, slide_u8, xy, h, w), None, None)
            err, self._what, self._n = self._probe(run)
            self._probed = (('id', 'forward_views'), None)
            self.decide(err, scope='views')
        return self._chosen.forward_views(x=x, slide_u8=slide_u8, tile_xy=tile_xy, ph=ph, pw=pw, views=views, **kw)


def trunk_engine(state_dict, device, precision=AUTO, head=None, **kw):
    """The engine for a net (`trunk_arch` of its state dict) and a precision name: BasicBlock nets 'auto' (AutoTrunkEngine), 'parity',
    'mx' or 'speed' (TrunkEngine); Bottleneck nets 'parity' or 'speed' (BottleneckEngine), 'auto' resolving to parity with a `report`
    that says why.  **kw goes to the engine's constructor."""
    if trunk_arch(state_dict)[0] == 'basic':
        if precision == AUTO:
            return AutoTrunkEngine(state_dict, device, head=head, **kw)
        return TrunkEngine(state_dict, device, planes={'parity': PARITY, 'mx': MX, 'speed': SPEED}[precision], head=head, **kw)
    if precision not in (AUTO, 'parity', 'speed'):
        raise NotImplementedError("Bottleneck nets run in 'parity', 'speed' or 'auto' precision, not %r" % (precision,))
    eng = BottleneckEngine(state_dict, device, planes=SPEED if precision == 'speed' else PARITY, head=head, **kw)
    if precision == AUTO:
        eng.report = {'mode': 'parity', 'probe_error': None,
                      'reason': 'Bottleneck nets have no mx mode (no pointwise-conv kernel in planes 3): auto resolves to parity'}
    return eng


# ---------------------------------------------------------------------- standalone device ops
def pf_pack(x, planes):
    """f32 NCHW GPU tensor -> zero-initialised padded-flat buffer (uint8 tensor)."""
    lib = native.load()
    _require_gpu(x, 'pf_pack input')
    x = x.to(torch.float32).contiguous()
    n, c, h, w = x.shape
    buf = torch.zeros(lib.wsi_pf_bytes(n, h, w, c, planes), dtype=torch.uint8, device=x.device)
    native.check(lib.wsi_pf_pack(_ptr(x), _ptr(buf), n, c, h, w, planes, _stream()), 'wsi_pf_pack')
    return buf


def pf_unpack(buf, n, c, h, w, planes):
    lib = native.load()
    _require_gpu(buf, 'pf_unpack input')
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=buf.device)
    native.check(lib.wsi_pf_unpack(_ptr(buf), _ptr(out), n, c, h, w, planes, _stream()), 'wsi_pf_unpack')
    return out


def pf_zeros(n, c, h, w, planes, device):
    lib = native.load()
    return torch.zeros(lib.wsi_pf_bytes(n, h, w, c, planes), dtype=torch.uint8, device=device)


def _prepack(weight, bn, planes, device, tconv):
    pk, bias = pack_conv(native.load(), _np32(weight), None if bn is None else [_np32(t) for t in bn], planes, tconv)
    return torch.from_numpy(pk).to(device), torch.from_numpy(bias).to(device)


def prepack_conv(weight, bn, planes, device):
    """weight (cout,cin,k,k) fp32; bn = (gamma, beta, mean, var) or None -> (wpk, bias) device tensors."""
    return _prepack(weight, bn, planes, device, False)


def prepack_tconv(weight, bn, planes, device):
    """ConvTranspose2d(c, c, 4, stride 2, padding 1) weight (c in, c out, 4, 4) fp32 as torch keeps it; bn = (gamma, beta, mean, var)
    of the output channels or None -> (wpk, bias) device tensors (wsi_prepack_tconv; c a multiple of 64)."""
    return _prepack(weight, bn, planes, device, True)


def tconv4x4s2_bn_relu(x_pf, n, h, w, c, wpk, bias, planes=2):
    """wsi_tconv4x4s2_bn_relu: PF (n, h, w, c) -> a new zeroed PF buffer (n, 2h, 2w, c) = relu(bn(conv_transpose2d(x)))."""
    lib = native.load()
    out = pf_zeros(n, c, 2 * h, 2 * w, planes, x_pf.device)
    native.check(lib.wsi_tconv4x4s2_bn_relu(_ptr(x_pf), _ptr(out), _ptr(wpk), _ptr(bias), n, h, w, c, planes, _stream()), 'wsi_tconv4x4s2_bn_relu')
    return out


def conv1x1_bn_relu_add(x_pf, skip_pf, n, h, w, cin, cout, wpk, bias, planes=2):
    """wsi_conv1x1_bn_relu_add: relu(bn(conv1x1(x))) + skip (the ReLU before the add) into a new zeroed PF buffer."""
    lib = native.load()
    out = pf_zeros(n, cout, h, w, planes, x_pf.device)
    native.check(lib.wsi_conv1x1_bn_relu_add(_ptr(x_pf), _ptr(out), _ptr(skip_pf), _ptr(wpk), _ptr(bias), n, h, w, cin, cout, planes, _stream()),
                 'wsi_conv1x1_bn_relu_add')
    return out


def groupnorm_relu_up2(x_pf, gn_weight, gn_bias, n, h, w, up2, planes=2, c=128, groups=32, eps=1e-5):
    """wsi_groupnorm_relu_up2: PF (n, h, w, 128) -> a new zeroed PF buffer = relu(group_norm(x)), bilinearly upsampled x2 (align_corners=True)
    to (n, 2h, 2w, 128) when `up2`.  gn_weight / gn_bias: fp32 GPU tensors of 128."""
    lib = native.load()
    k = 2 if up2 else 1
    out = pf_zeros(n, c, k * h, k * w, planes, x_pf.device)
    scratch = torch.empty(max(1, lib.wsi_groupnorm_scratch_bytes(n, h, w)), dtype=torch.uint8, device=x_pf.device)
    native.check(lib.wsi_groupnorm_relu_up2(_ptr(x_pf), _ptr(out), _ptr(gn_weight), _ptr(gn_bias), n, h, w, c, groups, eps, int(bool(up2)), planes,
                                            _ptr(scratch), _stream()), 'wsi_groupnorm_relu_up2')
    return out


def fpn_merge_head_up4(maps_pf, head_w, head_b, n, h, w, planes=2, c=128, with_quarter=False):
    """wsi_fpn_merge_head_up4: four PF maps (n, h, w, 128), head_w (classes, 128) and head_b fp32 GPU tensors -> logits (n, classes, 4h, 4w)
    fp32 = bilinear x4 (align_corners=True) of the 1x1 head over the maps' sum; with_quarter: (logits, the (n, classes, h, w) map before
    the upsample)."""
    lib = native.load()
    classes = int(head_w.shape[0])
    quarter = torch.empty((n, classes, h, w), dtype=torch.float32, device=head_w.device)
    out = torch.empty((n, classes, 4 * h, 4 * w), dtype=torch.float32, device=head_w.device)
    ptrs = (C.c_void_p * 4)(*[t.data_ptr() for t in maps_pf])
    native.check(lib.wsi_fpn_merge_head_up4(C.byref(ptrs), _ptr(head_w.contiguous()), _ptr(head_b.contiguous()), n, h, w, c, classes,
                                            _ptr(quarter), _ptr(out), planes, _stream()), 'wsi_fpn_merge_head_up4')
    return (out, quarter) if with_quarter else out


def upsample2_nearest(x_pf, n, h, w, c, planes=2):
    """wsi_upsample2_nearest: PF (n, h, w, c) -> a new zeroed PF buffer (n, 2h, 2w, c), every pixel repeated 2 x 2."""
    lib = native.load()
    out = pf_zeros(n, c, 2 * h, 2 * w, planes, x_pf.device)
    native.check(lib.wsi_upsample2_nearest(_ptr(x_pf), _ptr(out), n, h, w, c, planes, _stream()), 'wsi_upsample2_nearest')
    return out


def pyramid_pool(x_pf, n, h, w, c, planes=2):
    """wsi_pyramid_pool: PF (n, h, w, c) -> fp32 (n, 50, c), the adaptive average pools of sizes 1, 2, 3, 6 (bins row-major within a size)."""
    lib = native.load()
    out = torch.empty((n, 50, c), dtype=torch.float32, device=x_pf.device)
    native.check(lib.wsi_pyramid_pool(_ptr(x_pf), _ptr(out), n, h, w, c, planes, _stream()), 'wsi_pyramid_pool')
    return out


def pspnet_stage_project(pooled, stage_w, stage_b, proj_w):
    """wsi_pspnet_stage_project: pooled fp32 (n, 50, c) and per stage stage_w (c, c / 4), stage_b (c / 4,), proj_w (c / 4, 512) fp32 GPU
    tensors (the transposed matrices of `unet.pspnet_fold`) -> fp32 (n, 50, 512)."""
    lib = native.load()
    n, _, c = pooled.shape
    mats = [[t.to(torch.float32).contiguous() for t in group] for group in (stage_w, stage_b, proj_w)]
    mid = torch.empty((n, 50, c // 4), dtype=torch.float32, device=pooled.device)
    out = torch.empty((n, 50, 512), dtype=torch.float32, device=pooled.device)
    ptrs = [(C.c_void_p * 4)(*[t.data_ptr() for t in group]) for group in mats]
    native.check(lib.wsi_pspnet_stage_project(_ptr(pooled.contiguous()), *[C.byref(p) for p in ptrs], _ptr(mid), _ptr(out), n, c, _stream()),
                 'wsi_pspnet_stage_project')
    return out


def pyramid_expand(proj, n, h, w, planes=2, out=None):
    """wsi_pyramid_expand: fp32 (n, 50, 512) -> PF (n, h, w, 512) in `out` (a zeroed PF buffer is made when None): per pixel the sum of the
    bilinear samples (align_corners=True) of the four grids."""
    lib = native.load()
    if out is None:
        out = pf_zeros(n, 512, h, w, planes, proj.device)
    native.check(lib.wsi_pyramid_expand(_ptr(proj.contiguous()), _ptr(out), n, h, w, 512, planes, _stream()), 'wsi_pyramid_expand')
    return out


def pspnet_head_up8(x_pf, wpk, bias, n, h, w, classes, planes=2):
    """wsi_pspnet_head_up8: PF (n, h, w, 512), the packed 3x3 head (output channels padded to one line) and its padded bias -> fp32 logits
    (n, classes, 8h, 8w), bilinear x8 with align_corners=True."""
    lib = native.load()
    scratch = pf_zeros(n, 64 if planes == 1 else 32, h, w, planes, x_pf.device)
    out = torch.empty((n, classes, 8 * h, 8 * w), dtype=torch.float32, device=x_pf.device)
    native.check(lib.wsi_pspnet_head_up8(_ptr(x_pf), _ptr(wpk), _ptr(bias), _ptr(scratch), _ptr(out), n, h, w, 512, classes, planes, _stream()),
                 'wsi_pspnet_head_up8')
    return out


def conv1x1_bn_act(x_pf, n, h, w, cin, cout, wpk, bias, stride=1, resid_pf=None, relu=True, planes=2, out=None, check=True):
    """wsi_conv1x1_bn_act (the Bottleneck 1x1 convs: pointwise kernel at stride 1 unless ConvMode.PW_GATHER) into `out` (a zeroed PF
    buffer is made when None).  check=False returns (out, return code) instead of raising."""
    lib = native.load()
    if out is None:
        out = pf_zeros(n, cout, h // stride, w // stride, planes, x_pf.device)
    rc = lib.wsi_conv1x1_bn_act(_ptr(x_pf), _ptr(out), _ptr(resid_pf), _ptr(wpk), _ptr(bias), n, h, w, cin, cout, stride, int(relu), planes,
                                _stream())
    if not check:
        return out, rc
    native.check(rc, 'wsi_conv1x1_bn_act')
    return out


def conv_bn_act(x_pf, n, h, w, cin, cout, wpk, bias, stride=1, ksize=3, resid_pf=None, relu=True, planes=2):
    lib = native.load()
    out = pf_zeros(n, cout, h // stride, w // stride, planes, x_pf.device)
    if ksize == 3:
        rc = lib.wsi_conv3x3_bn_act(_ptr(x_pf), _ptr(out), _ptr(resid_pf), _ptr(wpk), _ptr(bias), n, h, w, cin, cout, stride,
                                    int(relu), planes, _stream())
    else:
        rc = lib.wsi_conv1x1_bn(_ptr(x_pf), _ptr(out), _ptr(wpk), _ptr(bias), n, h, w, cin, cout, stride, planes, _stream())
    native.check(rc, 'wsi_conv')
    return out


def tile_gather(slide_u8, tile_xy, ph, pw, lut):
    """(SH,SW,3) u8 slide + (N,2) int32 corners -> normalised (N,3,ph,pw) fp32 (reference
    utils/dataset.py:171-185 with the eval transform)."""
    lib = native.load()
    _require_gpu(slide_u8, 'slide')
    tile_xy = tile_xy.to(slide_u8.device, torch.int32).contiguous()
    n = tile_xy.shape[0]
    out = torch.empty((n, 3, ph, pw), dtype=torch.float32, device=slide_u8.device)
    native.check(lib.wsi_tile_gather(_ptr(slide_u8), slide_u8.stride(0), slide_u8.shape[0], slide_u8.shape[1],
                                     _ptr(tile_xy), _ptr(lut), _ptr(out), n, ph, pw, _stream()), 'wsi_tile_gather')
    return out


def stitch_add(pred, tile_logits, map_xy, dy, dx):
    """pred (C,MH,MW) float64 GPU += per-tile logits over dy x dx footprints at map_xy (T,2) int32."""
    lib = native.load()
    _require_gpu(pred, 'prediction map')
    if pred.dtype != torch.float64 or not pred.is_contiguous():
        raise ValueError('pred must be a contiguous float64 tensor')
    tile_logits = tile_logits.to(torch.float32).contiguous()
    map_xy = map_xy.to(pred.device, torch.int32).contiguous()
    t, c = tile_logits.shape
    native.check(lib.wsi_stitch_add(_ptr(tile_logits), _ptr(map_xy), t, c, dy, dx, _ptr(pred), pred.shape[1], pred.shape[2],
                                    _stream()), 'wsi_stitch_add')
    return pred


def exponent_span(values):
    """Device tensor of 2 ints: {smallest, largest} biased fp32 exponent of the nonzero finite values (stitch guard)."""
    lib = native.load()
    _require_gpu(values, 'values')
    v = values.to(torch.float32).contiguous()
    out = torch.empty(2, dtype=torch.int32, device=v.device)
    if v.numel() == 0:
        out[0], out[1] = 255, 0
        return out
    native.check(lib.wsi_exponent_span(_ptr(v), v.numel(), _ptr(out), _stream()), 'wsi_exponent_span')
    return out


def stitch_is_exact(span, addends_per_pixel):
    """True when float64 sums of the guarded fp32 values are provably exact, hence independent of the order of the tiles and
    of how ranks split them: exponent span + log2(addends per pixel) <= 29 (a 53-bit significand holds every partial sum).
    Outside the bound the map is still correct to float64 rounding (<= 2^-52 relative per addition), just not bit-reproducible."""
    lo, hi = (int(v) for v in span.cpu())
    return not (hi >= lo and (hi - lo) + int(np.ceil(np.log2(max(1, addends_per_pixel)))) > 29)


def check_stitch_exact(span, addends_per_pixel):
    """Raise if float64 sums of the guarded fp32 values could be inexact (order-dependent): see wsi_exponent_span."""
    lo, hi = (int(v) for v in span.cpu())
    if not stitch_is_exact(span, addends_per_pixel):
        raise RuntimeError('stitch: the per-tile values span 2^%d with up to %d addends per pixel: float64 sums are no longer exact, '
                           'so the accumulated map would depend on the order of the tiles' % (hi - lo, addends_per_pixel))


def stitch_add_dense(pred, tile_pred, map_xy):
    """pred (C,MH,MW) float64 GPU += tile_pred (T,C,ph,pw) fp32 blocks at map_xy (T,2) int32 (clipped at the border)."""
    lib = native.load()
    _require_gpu(pred, 'prediction map')
    if pred.dtype != torch.float64 or not pred.is_contiguous():
        raise ValueError('pred must be a contiguous float64 tensor')
    tile_pred = tile_pred.to(pred.device, torch.float32).contiguous()
    map_xy = map_xy.to(pred.device, torch.int32).contiguous()
    t, c, ph, pw = tile_pred.shape
    native.check(lib.wsi_stitch_add_dense(_ptr(tile_pred), _ptr(map_xy), t, c, ph, pw, _ptr(pred), pred.shape[1], pred.shape[2],
                                          _stream()), 'wsi_stitch_add_dense')
    return pred


def resize_nearest(x, size):
    """F.interpolate(x, size) in its default 'nearest' mode on a (B,C,H,W) fp32 GPU tensor (reference utils/eval.py:202-206)."""
    lib = native.load()
    _require_gpu(x, 'tensor')
    x = x.to(torch.float32).contiguous()
    b, c, h, w = x.shape
    out = torch.empty((b, c, int(size[0]), int(size[1])), dtype=torch.float32, device=x.device)
    native.check(lib.wsi_resize_nearest_f32(_ptr(x), b * c, h, w, _ptr(out), out.shape[2], out.shape[3], _stream()), 'wsi_resize_nearest_f32')
    return out


def softmax_threshold_argmax(pred, class_probs, mask=None, heat_mode=None, want_probs=True):
    """pred (C,H,W) float64 GPU -> (classes u8 (H,W), probs f64 (C,H,W) or None, heat u8 (H,W) or None)."""
    lib = native.load()
    _require_gpu(pred, 'prediction map')
    pred = pred.contiguous()
    c, h, w = pred.shape
    th = torch.tensor([float(v) for v in class_probs][:c], dtype=torch.float64, device=pred.device)
    probs = torch.empty_like(pred) if want_probs else None
    classes = torch.empty((h, w), dtype=torch.uint8, device=pred.device)
    heat = torch.empty((h, w), dtype=torch.uint8, device=pred.device) if heat_mode is not None else None
    m = mask.to(pred.device, torch.uint8).contiguous() if mask is not None else None
    native.check(lib.wsi_softmax_threshold_argmax(_ptr(pred), c, h * w, _ptr(th), _ptr(probs), _ptr(classes), _ptr(m),
                                                  0 if heat_mode in (None, 'cls') else 1, _ptr(heat), _stream()),
                 'wsi_softmax_threshold_argmax')
    return classes, probs, heat
