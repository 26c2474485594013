"""What the host layers over resident u8 maps share (contours.py, distance.py, regions.py): the checks of a map, of an int32 output and
of a caller's workspace, the small coercions, and the stage timer.  Every refusal is a ValueError and comes before anything asks for a
device, so the callers' `_require_gpu` follows these checks."""
import numpy as np
import torch


def check_map(m, what, limit=None):
    """a 2-D uint8 tensor with unit column stride and a row stride >= its width (any alignment), 1 .. limit pixels each way where a
    limit is given -> (h, w, pitch in bytes)"""
    if not isinstance(m, torch.Tensor) or m.dim() != 2 or m.dtype != torch.uint8:
        raise ValueError('%s must be a 2-D uint8 tensor' % what)
    h, w = int(m.shape[0]), int(m.shape[1])
    if limit is not None and not (1 <= w <= limit and 1 <= h <= limit):
        raise ValueError('%s of %d x %d pixels is outside 1 .. %d each way' % (what, w, h, limit))
    if (w > 1 and m.stride(1) != 1) or (h > 1 and m.stride(0) < w):
        raise ValueError('%s must have unit column stride and a row stride >= its width' % what)
    return h, w, (m.stride(0) if h > 1 else w)


def check_out_i32(out, h, w, dev):
    """an int32 (h, w) tensor on `dev` with unit column stride and a row stride >= w"""
    if not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or tuple(out.shape) != (h, w) or out.device != dev:
        raise ValueError('out must be an int32 (%d, %d) tensor on the map\'s device' % (h, w))
    if (w > 1 and out.stride(1) != 1) or (h > 1 and out.stride(0) < w):
        raise ValueError('out must have unit column stride and a row stride >= its width')


def take_workspace(workspace, need, dev):
    """the caller's workspace where it is a contiguous uint8 tensor of at least `need` bytes on `dev`, a fresh one where there is none"""
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.device != dev
            or not workspace.is_contiguous()):
        raise ValueError('the workspace must be a contiguous uint8 tensor of at least %d bytes on the map\'s device' % need)
    return workspace


def as_u8(mask, what):
    """a bool tensor as uint8; anything but a 2-D uint8 tensor after that is refused"""
    if isinstance(mask, torch.Tensor) and mask.dtype == torch.bool:
        mask = mask.to(torch.uint8)
    if not isinstance(mask, torch.Tensor) or mask.dim() != 2 or mask.dtype != torch.uint8:
        raise ValueError('%s must be a 2-D uint8 tensor' % what)
    return mask


def step2(step):
    """a step or an (sx, sy) pair -> (sx, sy), each >= 1"""
    sx, sy = (int(step), int(step)) if np.isscalar(step) else (int(step[0]), int(step[1]))
    if sx < 1 or sy < 1:
        raise ValueError('step %r must be >= 1 each way' % (step,))
    return sx, sy


def stage_marker(stages):
    """mark(name) records a torch.cuda.Event on the current stream and appends it to stages[name]: called before and after a stage's
    entry it leaves the stage's [begin, end] pair.  Nothing is recorded where stages is None."""
    def mark(name):
        if stages is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            stages.setdefault(name, []).append(ev)
    return mark
