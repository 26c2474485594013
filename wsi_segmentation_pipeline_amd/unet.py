"""U-Net segmentation model on the HIP path: the dense per-pixel ('seg') counterpart of the reference's
``smp.Unet('resnet18', classes=C)`` (/root/reference/eval_tumorbed.py:21-28, /root/reference/eval.py:22-27), driven by
``predict_wsis`` (utils/eval.py:51 ``model(batch_image)``) and ``predict_tumorbed(mode='seg')`` (:196-200
``model.decoder(model.encoder(batch_image))``).

segmentation_models_pytorch is third-party, absent here and un-pinned in the reference, so the architecture
and the state-dict key names are restated from its published 0.0.x source - **parity unpinned**; the numerical spec is
oracle/unet_oracle.py (torch fp32 CPU) and the HIP path is held to it:
  encoder  ResNet-18 or ResNet-34 (``encoder='resnet18' | 'resnet34'``; torchvision key names ``encoder.layerL.B.*``); forward
           returns [x4, x3, x2, x1, x0] (deepest first): x1..x4 = the LAST block of layer1..4, x0 = relu(bn1(conv1(x))) at half
           resolution.  Both depths give the same channels (512, 256, 128, 64, 64), so the decoder does not depend on the choice
  decoder  ``decoder.layer{1..5}.block.{0,1}.block.0.weight`` (3x3 conv, no bias) + ``.block.1.*`` (BatchNorm) + ReLU, each block
           preceded by nearest x2 upsampling and (blocks 1-4) concatenation of the next skip; channels 256/128/64/32/16;
           ``decoder.final_conv.{weight,bias}`` (1x1 to `classes`)
Bottleneck encoders (``Unet('resnet50' | 'resnet101', classes=C)``, the smp factory signature; class UNetSegBottleneck): the same decoder on
the maps of ``ResNet(Bottleneck, layers)`` - 2048 / 1024 / 512 / 256 / 64 channels - so only the first conv of decoder blocks 1-4 is wider
(``cat([up2(x), skip])`` of (2048, 1024), (256, 512), (128, 256), (64, 64)); key names as above; 'parity' and 'speed' only.
Eval-mode forwards run on libwsi_hip.so only (conv3x3 MFMA kernels + upsample/concat, head kernels: csrc/unet.hip); training
mode uses torch ops so ``train.py``-style callers still run.
The reference picks the model family by name (``eval('smp.' + args.model_name)``, ``--model_name``): this module serves 'Unet' (above) and
'Linknet' (`Linknet`, `LinknetSeg`, `LinknetEngine` below: smp's transposed-conv decoder, csrc/linknet.hip), so
``import wsi_segmentation_pipeline_amd.unet as smp`` keeps that line working.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import native
from .engine import BN_EPS, MX, PARITY, SPEED, BottleneckEngine, TrunkEngine, _np_ptr, _ptr, _require_gpu, _stream, trunk_arch

DEC_CH = (256, 128, 64, 32, 16)
ENC_CH = {'basic': (512, 256, 128, 64, 64), 'bottleneck': (2048, 1024, 512, 256, 64)}     # channels of [x4, x3, x2, x1, x0] per block type
SKIP_CH = ENC_CH['basic'][1:] + (0,)
ENCODER_LAYERS = {'resnet18': [2, 2, 2, 2], 'resnet34': [3, 4, 6, 3]}      # smp encoder names -> BasicBlocks per stage
BOTTLENECK_ENCODER_LAYERS = {'resnet50': [3, 4, 6, 3], 'resnet101': [3, 4, 23, 3]}      # ... -> Bottleneck blocks per stage


def encoder_layers(encoder):
    if encoder not in ENCODER_LAYERS:
        raise ValueError('encoder must be one of %s (BasicBlock ResNets), got %r' % (sorted(ENCODER_LAYERS), encoder))
    return ENCODER_LAYERS[encoder]


def _pad64(c):
    return (c + 63) // 64 * 64


def equal_batches(n, cap):
    """[(start, stop)] of the U-Net calls for n tiles at a tuned batch of `cap`: ceil(n / cap - 0.25) equal batches (no short last
    one; a quarter over `cap` still runs as ONE call, so a call holds at most ceil(1.25 cap) tiles).  [] for n = 0."""
    n, cap = int(n), max(1, int(cap))
    if n <= 0:
        return []
    mb = -(-n // max(1, int(np.ceil(n / cap - 0.25))))
    return [(i, min(i + mb, n)) for i in range(0, n, mb)]


def bottleneck_encoder_layers(encoder):
    if encoder not in BOTTLENECK_ENCODER_LAYERS:
        raise ValueError('encoder must be one of %s (Bottleneck ResNets), got %r' % (sorted(BOTTLENECK_ENCODER_LAYERS), encoder))
    return BOTTLENECK_ENCODER_LAYERS[encoder]


def _skip_ch(enc_ch):
    """channels of the skip each decoder block concatenates: encoder maps x3, x2, x1, x0, and none for the last block"""
    return tuple(enc_ch[1:]) + (0,)


def decoder_key_shapes(classes, enc_ch=ENC_CH['basic']):
    """[(key, shape, kind)] of the decoder in state-dict order, on an encoder whose maps [x4, x3, x2, x1, x0] have `enc_ch` channels."""
    out, cprev, skip = [], enc_ch[0], _skip_ch(enc_ch)
    for L in range(5):
        cin, cout = cprev + skip[L], DEC_CH[L]
        for j, ci in enumerate((cin, cout)):
            p = 'decoder.layer%d.block.%d.block' % (L + 1, j)
            out.append((p + '.0.weight', (cout, ci, 3, 3), 'conv'))
            for suffix, kind in (('weight', 'bn_w'), ('bias', 'bn_b'), ('running_mean', 'bn_m'), ('running_var', 'bn_v')):
                out.append(('%s.1.%s' % (p, suffix), (cout,), kind))
            out.append((p + '.1.num_batches_tracked', (), 'bn_n'))
        cprev = cout
    out.append(('decoder.final_conv.weight', (classes, DEC_CH[4], 1, 1), 'conv'))
    out.append(('decoder.final_conv.bias', (classes,), 'lin_b'))
    return out


class UNetEngine:
    """ResNet encoder + smp-style decoder on HIP kernels.  state_dict: ``encoder.*`` + ``decoder.*`` keys.  The encoder's block type and
    depth are read from the state dict (`engine.trunk_arch`): BasicBlock nets run on a TrunkEngine and wsi_unet_*, Bottleneck nets on a
    BottleneckEngine and wsi_unet_bneck_* (parity and speed only).  `encoder` (an smp name), when given, must agree with the state dict."""

    ENTRY = {'basic': 'wsi_unet', 'bottleneck': 'wsi_unet_bneck'}      # prefix of the four C entries, per encoder architecture

    def __init__(self, state_dict, device, planes=PARITY, classes=None, max_batch=None, encoder=None):
        self._ws = {}
        self.lib = native.load()
        self.device = torch.device(device)
        enc_sd = {k[len('encoder.'):]: v for k, v in state_dict.items() if k.startswith('encoder.')}
        self.arch = trunk_arch(enc_sd)[0]
        if self.arch == 'bottleneck':
            if planes == MX:
                raise ValueError("a U-Net on a Bottleneck encoder runs in precision 'parity' or 'speed': there is no mx mode")
            self.trunk = BottleneckEngine(enc_sd, device, planes=planes)
        else:
            self.trunk = TrunkEngine(enc_sd, device, planes=planes)
        if encoder is not None:
            named = BOTTLENECK_ENCODER_LAYERS.get(encoder) or encoder_layers(encoder)
            if self.trunk.layers != named or (encoder in BOTTLENECK_ENCODER_LAYERS) != (self.arch == 'bottleneck'):
                raise ValueError('state dict holds a %s %s encoder, not %s' % (self.arch, self.trunk.layers, encoder))
        self.enc_ch = ENC_CH[self.arch]
        entry = self.ENTRY[self.arch]
        self._ws_bytes, self._ws_init, self._forward, self._decoder = (
            getattr(self.lib, entry + s) for s in ('_workspace_bytes', '_workspace_init', '_forward', '_decoder'))
        self.planes = planes
        self.classes = int(classes if classes is not None else state_dict['decoder.final_conv.weight'].shape[0])
        self.max_batch = max_batch
        self._keep, self._ws = [], {}

        def f32(key):
            return np.ascontiguousarray(state_dict[key].detach().to('cpu', torch.float32).numpy())

        def dev(a):
            t = torch.from_numpy(a).to(self.device)
            self._keep.append(t)
            return t

        self._pack_decoder(f32, dev)

    def _pack_decoder(self, f32, dev):
        """Fill self.dw from the decoder.* keys: f32(key) -> contiguous fp32 array, dev(array) -> device tensor kept alive."""
        planes = self.planes
        skip_ch = _skip_ch(self.enc_ch)
        self.dw = native.WsiUnetDecoderWeights()
        cprev_real, cprev_pad = self.enc_ch[0], self.enc_ch[0]
        for L in range(5):
            cout = DEC_CH[L]
            cout_pad = _pad64(cout) if planes == 1 else -(-cout // 32) * 32        # whole 128-byte lines: 64 channels in speed mode, 32 otherwise
            for j in range(2):
                p = 'decoder.layer%d.block.%d.block' % (L + 1, j)
                w = f32(p + '.0.weight')
                if j == 0:                                     # input = [upsampled x (real cprev of cprev_pad) | skip]
                    cin_pad = cprev_pad + skip_ch[L]
                    wp = np.zeros((cout_pad, cin_pad, 3, 3), np.float32)
                    wp[:cout, :cprev_real] = w[:, :cprev_real]
                    wp[:cout, cprev_pad:cprev_pad + skip_ch[L]] = w[:, cprev_real:]
                else:
                    cin_pad = cout_pad
                    wp = np.zeros((cout_pad, cin_pad, 3, 3), np.float32)
                    wp[:cout, :cout] = w
                bn = []
                for suffix, fill in (('weight', 1.0), ('bias', 0.0), ('running_mean', 0.0), ('running_var', 1.0)):
                    a = np.full(cout_pad, fill, np.float32)    # padding channels: scale ~1, shift 0 -> relu(0) = 0
                    a[:cout] = f32('%s.1.%s' % (p, suffix))
                    bn.append(a)
                pk = np.empty(self.lib.wsi_prepack_conv_bytes(cout_pad, cin_pad, 3, planes), np.uint8)
                bias = np.empty(cout_pad, np.float32)
                native.check(self.lib.wsi_prepack_conv(_np_ptr(wp), *[_np_ptr(a) for a in bn], BN_EPS, cout_pad, cin_pad, 3, planes,
                                                       _np_ptr(pk), _np_ptr(bias)), 'wsi_prepack_conv')
                i = 2 * L + j
                self.dw.conv_w[i], self.dw.conv_b[i] = dev(pk).data_ptr(), dev(bias).data_ptr()
                self.dw.cin[i], self.dw.cout[i] = cin_pad, cout_pad
            cprev_real, cprev_pad = cout, cout_pad
        hw = f32('decoder.final_conv.weight').reshape(self.classes, DEC_CH[4])
        self.dw.head_w = dev(np.ascontiguousarray(hw)).data_ptr()
        self.dw.head_b = dev(f32('decoder.final_conv.bias')).data_ptr()
        self.dw.head_cin, self.dw.classes = DEC_CH[4], self.classes
        self.dw.tail_w = None
        if planes == PARITY and DEC_CH[3] == 32 and DEC_CH[4] <= 16 and self.classes <= 4:
            # r05: the last block + head as one kernel (csrc/tail.hip) on the block's REAL channels
            p0, p1 = ('decoder.layer5.block.%d.block' % j for j in range(2))
            bn = [[f32('%s.1.%s' % (p, sfx)) for sfx in ('weight', 'bias', 'running_mean', 'running_var')] for p in (p0, p1)]
            blob = np.empty(self.lib.wsi_unet_tail_prepack_bytes(), np.uint8)
            hb = f32('decoder.final_conv.bias')
            native.check(self.lib.wsi_unet_tail_prepack(_np_ptr(f32(p0 + '.0.weight')), *[_np_ptr(a) for a in bn[0]],
                                                        _np_ptr(f32(p1 + '.0.weight')), *[_np_ptr(a) for a in bn[1]], BN_EPS,
                                                        _np_ptr(np.ascontiguousarray(hw)), _np_ptr(hb), DEC_CH[3], DEC_CH[4], self.classes,
                                                        _np_ptr(blob)), 'wsi_unet_tail_prepack')
            self.dw.tail_w = dev(blob).data_ptr()

    def _workspace(self, n, h, w):
        key = (h, w)
        ent = self._ws.get(key)
        if ent is None or ent[1] < n:
            nbytes = self._ws_bytes(C.byref(self.dw), n, h, w, self.planes)
            if nbytes == 0:
                raise ValueError('unsupported patch shape %dx%d (need multiples of 32)' % (h, w))
            self.release_workspaces()                          # the library forgets the addresses before the allocator can reuse them
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            native.check(self._ws_init(C.byref(self.dw), _ptr(ws), n, h, w, self.planes, _stream()), self._ws_init.__name__)
            ent = self._ws[key] = (ws, n)
        return ent

    def release_workspaces(self):
        """Free every planned workspace and make the library forget its layout tag (trunk.hip g_ws_layout; a Bottleneck workspace has none)."""
        for ws, _ in self._ws.values():
            self.lib.wsi_trunk_workspace_release(_ptr(ws))
        self._ws.clear()

    def __del__(self):
        try:
            self.release_workspaces()
        except Exception:                                   # interpreter shutdown: the library may be gone
            pass

    TUNED_BATCH_256 = 512                                    # tiles of 256 x 256 per U-Net call (bench.py --seg-batch default)

    def _batch(self, h, w):
        """Tiles per U-Net call: `max_batch`, else the tuned size scaled by patch area (r05 sweep at 256 x 256, parity: 128 / 256 / 512
        tiles -> 28.1 / 31.2 / 33.1 k patches/s: at 128 the 8 x 8 and 16 x 16 levels launch fewer workgroups than the chip has CUs)
        as far as half of the free HBM allows - ~77 MB of workspace per 256 x 256 tile, 39 GB of the 288 GB at 512.  A Bottleneck encoder
        keeps the same rule with its own workspace size (wsi_unet_bneck_workspace_bytes, ~94 MB per tile); ResNet-50 sweep at 256 x 256,
        parity, u8 tiles: 128 / 256 / 512 tiles -> 10.3 / 11.1 / 11.7 k patches/s (profiles/unet_resnet50_bench.json), so it keeps 512."""
        if self.max_batch:
            return self.max_batch
        want = max(1, int(self.TUNED_BATCH_256 * 65536 // max(h * w, 1)))
        per = self._ws_bytes(C.byref(self.dw), 16, h, w, self.planes) / 16.0
        if per <= 0:
            return want
        try:
            free = torch.cuda.mem_get_info(self.device)[0] + max(0, torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device))
        except Exception:
            return want
        held = sum(int(ws.numel()) for ws, _ in self._ws.values())
        return max(1, min(want, int(0.5 * (free + held) / per)))

    def _run(self, n, h, w, in_f32, slide, tile_xy, want_logits, want_enc):
        ws, cap = self._workspace(n, h, w)
        logits = torch.empty((n, self.classes, h, w), dtype=torch.float32, device=self.device) if want_logits else None
        enc = None
        enc_ptrs = None
        if want_enc:
            shapes = [(c, h >> k, w >> k) for c, k in zip(self.enc_ch, (5, 4, 3, 2, 1))]
            enc = [torch.empty((n,) + s, dtype=torch.float32, device=self.device) for s in shapes]
            enc_ptrs = (C.c_void_p * 5)(*[t.data_ptr() for t in enc])
        if slide is not None:
            sp, pitch, sh, sw = _ptr(slide), slide.stride(0), slide.shape[0], slide.shape[1]
        else:
            sp, pitch, sh, sw = None, 0, 0, 0
        native.check(self._forward(C.byref(self.trunk.wt), C.byref(self.dw), _ptr(in_f32), sp, pitch, sh, sw, _ptr(tile_xy),
                                   _ptr(self.trunk.lut), n, h, w, _ptr(ws), cap, _ptr(logits),
                                   C.byref(enc_ptrs) if enc_ptrs is not None else None, _stream()), self._forward.__name__)
        return logits, enc

    def forward_f32(self, x, logits=True, enc=False):
        """x (N,3,H,W) normalised fp32 GPU -> logits (N,classes,H,W) [, the five encoder maps deepest first]."""
        _require_gpu(x, 'input batch')
        x = x.to(torch.float32).contiguous()
        n, _, h, w = x.shape
        mb = self._batch(h, w)
        outs = [self._run(min(mb, n - i), h, w, x[i:i + mb], None, None, logits, enc) for i in range(0, n, mb)]
        lg = torch.cat([o[0] for o in outs]) if logits else None
        en = [torch.cat([o[1][k] for o in outs]) for k in range(5)] if enc else None
        return lg, en

    def forward_tiles(self, slide_u8, tile_xy, ph, pw):
        """Tiles read straight from an HBM-resident u8 slide -> logits (N,classes,ph,pw)."""
        _require_gpu(slide_u8, 'slide')
        tile_xy = tile_xy.to(self.device, torch.int32).contiguous()
        n = tile_xy.shape[0]
        if n == 0:
            return torch.empty((0, self.classes, ph, pw), dtype=torch.float32, device=self.device)
        parts = [self._run(b - a, ph, pw, None, slide_u8, tile_xy[a:b], True, False)[0] for a, b in equal_batches(n, self._batch(ph, pw))]
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def decode(self, enc):
        """`model.decoder(encoding)`: five fp32 NCHW GPU maps (deepest first) -> logits."""
        for t in enc:
            _require_gpu(t, 'encoder map')
        enc = [t.to(torch.float32).contiguous() for t in enc]
        n, h, w = enc[0].shape[0], enc[0].shape[2] * 32, enc[0].shape[3] * 32
        ws, cap = self._workspace(n, h, w)
        logits = torch.empty((n, self.classes, h, w), dtype=torch.float32, device=self.device)
        ptrs = (C.c_void_p * 5)(*[t.data_ptr() for t in enc])
        native.check(self._decoder(C.byref(self.dw), C.byref(ptrs), n, h, w, self.planes, _ptr(ws), cap, _ptr(logits), _stream()),
                     self._decoder.__name__)
        return logits


# ---------------------------------------------------------------------------------------------- nn.Module surface
class _Conv2dReLU(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.block = nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))

    def forward(self, x):
        return self.block(x)


class _DecoderBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.block = nn.Sequential(_Conv2dReLU(cin, cout), _Conv2dReLU(cout, cout))

    def forward(self, x, skip=None):
        x = F.interpolate(x, scale_factor=2, mode='nearest')
        if skip is not None:
            x = torch.cat([x, skip], 1)
        return self.block(x)


class UNetDecoder(nn.Module):
    def __init__(self, classes, owner=None, enc_ch=ENC_CH['basic']):
        super().__init__()
        cprev, skip = enc_ch[0], _skip_ch(enc_ch)
        for L in range(5):
            setattr(self, 'layer%d' % (L + 1), _DecoderBlock(cprev + skip[L], DEC_CH[L]))
            cprev = DEC_CH[L]
        self.final_conv = nn.Conv2d(DEC_CH[4], classes, 1)
        self._owner = [owner]                                  # list: not registered as a sub-module

    def forward(self, enc):
        if not self.training:
            return self._owner[0].hip_engine(enc[0].device).decode(list(enc))
        x = enc[0]
        skips = list(enc[1:]) + [None]
        for L in range(5):
            x = getattr(self, 'layer%d' % (L + 1))(x, skips[L])
        return self.final_conv(x)


class UNetEncoder(nn.Module):
    """ResNet-18 / ResNet-34 trunk with the smp encoder surface: forward(x) -> [x4, x3, x2, x1, x0]; ``out_shapes``."""

    ARCH = 'basic'

    def __init__(self, owner=None, encoder='resnet18'):
        super().__init__()
        net = self._net(encoder)
        for name in ('conv1', 'bn1', 'relu', 'maxpool', 'layer1', 'layer2', 'layer3', 'layer4'):
            setattr(self, name, getattr(net, name))
        self.out_shapes = ENC_CH[self.ARCH]
        self._owner = [owner]

    @staticmethod
    def _net(encoder):
        import resnets_shift
        return resnets_shift.ResNet(resnets_shift.BasicBlock, encoder_layers(encoder))

    def forward(self, x):
        if not self.training:
            return self._owner[0].hip_engine(x.device).forward_f32(x, logits=False, enc=True)[1]
        x0 = self.relu(self.bn1(self.conv1(x)))
        x1 = self.layer1(self.maxpool(x0))
        x2 = self.layer2(x1)
        x3 = self.layer3(x2)
        x4 = self.layer4(x3)
        return [x4, x3, x2, x1, x0]


class UNetBottleneckEncoder(UNetEncoder):
    """ResNet-50 / ResNet-101 trunk with the same surface; ``out_shapes`` = (2048, 1024, 512, 256, 64)."""
    ARCH = 'bottleneck'

    @staticmethod
    def _net(encoder):
        """conv1 ... layer4 of ``resnets_shift.ResNet(Bottleneck, layers)``, built as its __init__ / _make_layer build them (same modules,
        same initialisation) but without the bag heads, which are no part of an encoder: fc.0 alone is 32768 x 16384 at expansion 4."""
        import resnets_shift as rs
        net = nn.Module()
        net.conv1, net.bn1, net.relu, net.maxpool = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for i, (planes, stride, blocks) in enumerate(zip((64, 128, 256, 512), (1, 2, 2, 2), bottleneck_encoder_layers(encoder)), start=1):
            width = planes * rs.Bottleneck.expansion
            down = nn.Sequential(rs.conv1x1(inplanes, width, stride), nn.BatchNorm2d(width))
            seq = [rs.Bottleneck(inplanes, planes, stride, down)] + [rs.Bottleneck(width, planes) for _ in range(1, blocks)]
            setattr(net, 'layer%d' % i, nn.Sequential(*seq))
            inplanes = width
        for mod in net.modules():
            if isinstance(mod, nn.Conv2d):
                nn.init.kaiming_normal_(mod.weight, mode='fan_out', nonlinearity='relu')
        return net


class UNetSeg(nn.Module):
    """Drop-in for ``smp.Unet(encoder, classes=C, activation=None)`` with encoder 'resnet18' (default) or 'resnet34' as the reference
    uses it: ``model(x)`` -> (B,C,H,W) logits; ``model.encoder`` / ``model.decoder`` callable separately; ``classifier`` /
    ``regressor`` heads attachable."""

    ENCODER = UNetEncoder
    ENGINE = UNetEngine
    PRECISIONS = ('parity', 'mx', 'speed')

    def __init__(self, classes=4, precision='parity', encoder='resnet18'):
        super().__init__()
        if precision not in self.PRECISIONS:
            raise ValueError('precision must be one of %s for a %s encoder, got %r' % (' / '.join(self.PRECISIONS), encoder, precision))
        self.encoder = self.ENCODER(self, encoder)
        self.decoder = self._make_decoder(classes)
        self.classes, self.precision, self.encoder_name = classes, precision, encoder
        self._engine, self._engine_sig = None, None

    def _make_decoder(self, classes):
        return UNetDecoder(classes, self, self.encoder.out_shapes)

    def hip_engine(self, device=None):
        device = torch.device(device) if device is not None else self.decoder.final_conv.weight.device
        sig = (str(device), self.precision) + tuple((p.data_ptr(), p._version) for p in self.parameters()) \
            + tuple((b.data_ptr(), b._version) for b in self.buffers())
        if self._engine is None or sig != self._engine_sig:
            self._engine = self.ENGINE(self.state_dict(), device, planes={'parity': PARITY, 'mx': MX, 'speed': SPEED}[self.precision],
                                       classes=self.classes, encoder=self.encoder_name)
            self._engine_sig = sig
        return self._engine

    def forward(self, x):
        if self.training:
            return self.decoder(self.encoder(x))
        if not x.is_cuda:
            raise RuntimeError('UNetSeg eval forward runs on HIP kernels only: move the model and the input to the GPU')
        return self.hip_engine(x.device).forward_f32(x)[0]


class UNetSegBottleneck(UNetSeg):
    """``smp.Unet('resnet50' | 'resnet101', classes=C, activation=None)``: UNetSeg on a Bottleneck encoder (``model.encoder.out_shapes`` =
    (2048, 1024, 512, 256, 64)); precision 'parity' or 'speed'.  A UNetSeg to every caller that asks (utils.eval's fused tile path)."""
    ENCODER = UNetBottleneckEncoder
    PRECISIONS = ('parity', 'speed')

    def __init__(self, classes=4, precision='parity', encoder='resnet50'):
        super().__init__(classes, precision, encoder)


# ---------------------------------------------------------------------------------------------- Linknet
# smp's light decoder (``--model_name Linknet``, the reference's myargs.py:9; built by ``eval('smp.' + args.model_name)(...)`` at
# eval.py:22, eval_tumorbed.py:21).  Restated from the published 0.0.x source like the U-Net above - parity unpinned, the numerical spec is
# tests/linknet_oracle.py.  ``decoder.layer{1..5}`` = DecoderBlock(cin, cout) with mid = cin // 4:
#   block.0  1x1 conv cin -> mid (no bias) + BN + ReLU
#   block.1  ConvTranspose2d(mid, mid, kernel 4, stride 2, padding 1, bias=False) + BN + ReLU     weight [mid in][mid out][4][4]
#   block.2  1x1 conv mid -> cout (no bias) + BN + ReLU
# and ``x = block(x) + skip`` (no ReLU after the add) with skips x3, x2, x1, x0 for layers 1-4, none for layer 5; ``decoder.final_conv``
# 1x1 32 -> classes + bias.  BasicBlock encoders only ('resnet18', 'resnet34'); precision 'parity' or 'speed'.
LINKNET_CH = ((512, 128, 256), (256, 64, 128), (128, 32, 64), (64, 16, 64), (64, 16, 32))      # (cin, mid, cout) of layer1..5


def linknet_decoder_key_shapes(classes):
    """[(key, shape, kind)] of the Linknet decoder in state-dict order: 92 keys.  kind 'tconv' = the transposed-conv weight [in][out][4][4]."""
    out = []
    for L, (cin, mid, cout) in enumerate(LINKNET_CH):
        for j, (shape, kind, c) in enumerate((((mid, cin, 1, 1), 'conv', mid), ((mid, mid, 4, 4), 'tconv', mid), ((cout, mid, 1, 1), 'conv', cout))):
            p = 'decoder.layer%d.block.%d.block' % (L + 1, j)
            out.append((p + '.0.weight', shape, kind))
            for suffix, bn_kind in (('weight', 'bn_w'), ('bias', 'bn_b'), ('running_mean', 'bn_m'), ('running_var', 'bn_v')):
                out.append(('%s.1.%s' % (p, suffix), (c,), bn_kind))
            out.append((p + '.1.num_batches_tracked', (), 'bn_n'))
    out.append(('decoder.final_conv.weight', (classes, LINKNET_CH[4][2], 1, 1), 'conv'))
    out.append(('decoder.final_conv.bias', (classes,), 'lin_b'))
    return out


class LinknetEngine(UNetEngine):
    """BasicBlock ResNet encoder + Linknet decoder on HIP kernels (wsi_linknet_*; csrc/linknet.hip): the surface of UNetEngine -
    forward_f32, forward_tiles, decode, release_workspaces - with the batch sized by the Linknet workspace (~70 MB per 256 x 256 tile in
    parity mode).  Every stored tensor is at least 64 channels wide: layers narrower than that carry zero weights in the padding."""

    ENTRY = {'basic': 'wsi_linknet'}

    def __init__(self, state_dict, device, planes=PARITY, classes=None, max_batch=None, encoder=None):
        if planes not in (PARITY, SPEED):
            raise ValueError("a Linknet runs in precision 'parity' or 'speed': there is no mx mode")
        if encoder is not None:
            encoder_layers(encoder)
        if trunk_arch({k[len('encoder.'):]: v for k, v in state_dict.items() if k.startswith('encoder.')})[0] != 'basic':
            raise ValueError('a Linknet runs on BasicBlock encoders only (%s)' % sorted(ENCODER_LAYERS))
        super().__init__(state_dict, device, planes, classes, max_batch, encoder)

    def _pack_decoder(self, f32, dev):
        planes = self.planes
        self.dw = native.WsiLinknetDecoderWeights()

        def pad(c):
            return max(64, c)

        for L, (cin, mid, cout) in enumerate(LINKNET_CH):
            cin_s = cin if L == 0 else pad(LINKNET_CH[L - 1][2])           # stored width of the block's input
            for j, (co, ci, co_s, ci_s) in enumerate(((mid, cin, pad(mid), cin_s), (mid, mid, pad(mid), pad(mid)), (cout, mid, pad(cout), pad(mid)))):
                p = 'decoder.layer%d.block.%d.block' % (L + 1, j)
                w = f32(p + '.0.weight')
                k = 4 if j == 1 else 1
                wp = np.zeros((ci_s, co_s, 4, 4) if j == 1 else (co_s, ci_s, 1, 1), np.float32)
                if j == 1:
                    wp[:ci, :co] = w                                   # ConvTranspose2d keeps [in][out][ky][kx]
                else:
                    wp[:co, :ci] = w
                bn = []
                for suffix, fill in (('weight', 1.0), ('bias', 0.0), ('running_mean', 0.0), ('running_var', 1.0)):
                    a = np.full(co_s, fill, np.float32)                # padding channels: scale ~1, shift 0 -> relu(0) = 0
                    a[:co] = f32('%s.1.%s' % (p, suffix))
                    bn.append(a)
                bias = np.empty(co_s, np.float32)
                if k == 4:
                    pk = np.empty(self.lib.wsi_prepack_tconv_bytes(co_s, planes), np.uint8)
                    native.check(self.lib.wsi_prepack_tconv(_np_ptr(wp), *[_np_ptr(a) for a in bn], BN_EPS, co_s, planes, _np_ptr(pk), _np_ptr(bias)),
                                 'wsi_prepack_tconv')
                else:
                    pk = np.empty(self.lib.wsi_prepack_conv_bytes(co_s, ci_s, 1, planes), np.uint8)
                    native.check(self.lib.wsi_prepack_conv(_np_ptr(wp), *[_np_ptr(a) for a in bn], BN_EPS, co_s, ci_s, 1, planes, _np_ptr(pk),
                                                           _np_ptr(bias)), 'wsi_prepack_conv')
                i = 3 * L + j
                self.dw.conv_w[i], self.dw.conv_b[i] = dev(pk).data_ptr(), dev(bias).data_ptr()
                self.dw.cin[i], self.dw.cout[i] = ci_s, co_s
        head_cin = LINKNET_CH[4][2]
        hw = f32('decoder.final_conv.weight').reshape(self.classes, head_cin)
        self.dw.head_w = dev(np.ascontiguousarray(hw)).data_ptr()
        self.dw.head_b = dev(f32('decoder.final_conv.bias')).data_ptr()
        self.dw.head_cin, self.dw.classes = head_cin, self.classes
        self.dw.tail_w = None
        if planes == PARITY and self.classes <= 4:
            # the last block + head as one kernel (csrc/linknet.hip linknet_tail_kernel) on the block's REAL channels
            cin, mid, cout = LINKNET_CH[4]
            ps = ['decoder.layer5.block.%d.block' % j for j in range(3)]
            args = []
            for p in ps:
                args.append(_np_ptr(f32(p + '.0.weight')))
                args += [_np_ptr(f32('%s.1.%s' % (p, sfx))) for sfx in ('weight', 'bias', 'running_mean', 'running_var')]
            blob = np.empty(self.lib.wsi_linknet_tail_prepack_bytes(), np.uint8)
            native.check(self.lib.wsi_linknet_tail_prepack(*args, BN_EPS, _np_ptr(np.ascontiguousarray(hw)), _np_ptr(f32('decoder.final_conv.bias')),
                                                           cin, mid, cout, self.classes, _np_ptr(blob)), 'wsi_linknet_tail_prepack')
            self.dw.tail_w = dev(blob).data_ptr()


class _ConvBnReLU(nn.Module):
    """``.block`` = Sequential(conv, BatchNorm2d, ReLU): the state-dict keys ``block.0.weight``, ``block.1.*``."""

    def __init__(self, conv, c):
        super().__init__()
        self.block = nn.Sequential(conv, nn.BatchNorm2d(c), nn.ReLU(inplace=True))

    def forward(self, x):
        return self.block(x)


class _LinknetBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        mid = cin // 4
        self.block = nn.Sequential(_ConvBnReLU(nn.Conv2d(cin, mid, 1, bias=False), mid),
                                   _ConvBnReLU(nn.ConvTranspose2d(mid, mid, 4, stride=2, padding=1, bias=False), mid),
                                   _ConvBnReLU(nn.Conv2d(mid, cout, 1, bias=False), cout))

    def forward(self, x, skip=None):
        x = self.block(x)
        return x if skip is None else x + skip


class LinknetDecoder(nn.Module):
    def __init__(self, classes, owner=None):
        super().__init__()
        for L, (cin, _mid, cout) in enumerate(LINKNET_CH):
            setattr(self, 'layer%d' % (L + 1), _LinknetBlock(cin, cout))
        self.final_conv = nn.Conv2d(LINKNET_CH[4][2], classes, 1)
        self._owner = [owner]                                  # list: not registered as a sub-module

    def forward(self, enc):
        if not self.training:
            return self._owner[0].hip_engine(enc[0].device).decode(list(enc))
        x = enc[0]
        skips = list(enc[1:]) + [None]
        for L in range(5):
            x = getattr(self, 'layer%d' % (L + 1))(x, skips[L])
        return self.final_conv(x)


class LinknetSeg(UNetSeg):
    """Drop-in for ``smp.Linknet(encoder, classes=C, activation=None)`` with encoder 'resnet18' (default) or 'resnet34': the surface of
    UNetSeg (``model(x)``, ``model.encoder``, ``model.decoder``, ``hip_engine``), so every caller that takes a UNetSeg - utils.eval's
    fused tile path, multi-rank stitching - takes it too.  Precision 'parity' or 'speed'."""
    PRECISIONS = ('parity', 'speed')
    ENGINE = LinknetEngine

    def _make_decoder(self, classes):
        return LinknetDecoder(classes, self)


def Linknet(encoder_name='resnet34', encoder_weights=None, classes=1, activation=None, precision='parity'):
    """smp's factory signature for the Linknet, so with ``import wsi_segmentation_pipeline_amd.unet as smp`` the reference's
    ``getattr(smp, args.model_name)(args.arch_encoder, encoder_weights=None, classes=C, activation=None)`` serves 'Unet' and 'Linknet'.
    Refusals as `Unet`; encoders 'resnet18' and 'resnet34' only."""
    if encoder_weights is not None:
        raise ValueError('encoder_weights must be None (got %r): pretrained weights are not downloaded; load a state dict' % (encoder_weights,))
    if activation is not None:
        raise ValueError('activation must be None (got %r): the model returns logits, as the reference builds it' % (activation,))
    if encoder_name not in ENCODER_LAYERS:
        raise ValueError('encoder_name must be one of %s for a Linknet, got %r' % (list(ENCODER_LAYERS), encoder_name))
    return LinknetSeg(classes, precision, encoder_name)


def Unet(encoder_name='resnet34', encoder_weights=None, classes=1, activation=None, precision='parity'):
    """The factory with smp's own signature, so the reference's ``smp.Unet(args.arch_encoder, encoder_weights=None, classes=C,
    activation=None)`` becomes ``unet.Unet(...)``: UNetSeg for 'resnet18' / 'resnet34', UNetSegBottleneck for 'resnet50' / 'resnet101'.
    The model returns logits: `activation` must be None, as the reference passes it; `encoder_weights` must be None (nothing is
    downloaded: load a checkpoint with ``load_state_dict``)."""
    if encoder_weights is not None:
        raise ValueError('encoder_weights must be None (got %r): pretrained weights are not downloaded; load a state dict' % (encoder_weights,))
    if activation is not None:
        raise ValueError('activation must be None (got %r): the model returns logits, as the reference builds it' % (activation,))
    if encoder_name in ENCODER_LAYERS:
        return UNetSeg(classes, precision, encoder_name)
    if encoder_name in BOTTLENECK_ENCODER_LAYERS:
        return UNetSegBottleneck(classes, precision, encoder_name)
    raise ValueError('encoder_name must be one of %s, got %r' % (list(ENCODER_LAYERS) + list(BOTTLENECK_ENCODER_LAYERS), encoder_name))
