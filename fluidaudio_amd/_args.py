"""What the wrappers of the C ABI do to their arguments before the library sees them: plain functions, each of them here once.  The texts
of the refusals stay with the entries that raise them."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def invalid(where: str, detail: str):
    return L.FluidAudioHipError(L.INVALID_ARGUMENT, where, detail)


def ragged(arrays, offsets, dtype, where: str = "", detail: str | None = None):
    """A batch of unequal arrays as the entries take it: a list of arrays (offsets None) — or one flat array with its batch + 1 offsets —
    becomes (contiguous flat array of dtype, int64 offsets).  A flat torch tensor is handed through for the caller to judge.  Offsets
    that are not a one-dimensional array of at least one entry are refused with `detail`; detail None leaves their shape to the caller."""
    if offsets is None:
        arrays = [np.ascontiguousarray(x, dtype).reshape(-1) for x in arrays]
        offsets = np.concatenate([[0], np.cumsum([x.size for x in arrays])]).astype(np.int64)
        arrays = np.concatenate(arrays) if arrays else np.zeros(0, dtype)
    offsets = np.ascontiguousarray(offsets, np.int64)
    if detail is not None and (offsets.ndim != 1 or offsets.size < 1):
        raise invalid(where, detail)
    return (arrays if hasattr(arrays, "data_ptr") else np.ascontiguousarray(arrays, dtype)), offsets


def context_beside(ctx, like) -> L.Context:
    """The caller's context, or the default one: of a torch tensor's device, or of the process."""
    return ctx or L.default_context(like.device.index if hasattr(like, "data_ptr") else None)


def is_dev(t, dtype_name: str, ndim: int | None = None, contiguous: bool = True) -> bool:
    """A torch tensor of that dtype (and rank) on a CUDA device, contiguous unless the entry takes strides."""
    import torch
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == getattr(torch, dtype_name) and (not contiguous or t.is_contiguous())
            and (ndim is None or t.dim() == ndim))


def ptr(a):
    """What ctypes takes for a numpy array, a torch tensor or None."""
    if a is None:
        return None
    return C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a.ctypes.data


def cfg_ref(cfg):
    return None if cfg is None else C.byref(cfg)


def beside(like, shape, dtype_name: str, torch_empty: bool = False):
    """An output next to an input: a zero-filled numpy array beside a numpy array; beside a torch tensor one on its device, zero-filled
    or, where the entry writes all of it, empty."""
    if hasattr(like, "data_ptr"):
        import torch
        return (torch.empty if torch_empty else torch.zeros)(shape, dtype=getattr(torch, dtype_name), device=like.device)
    return np.zeros(shape, getattr(np, dtype_name))


def device_tensor(x, ctx: L.Context, dtype=None):
    """x as a contiguous torch tensor (of dtype) for a _dev entry of ctx: it has to be a CUDA tensor, and on the context's device — a
    pointer into another device's memory is not valid there."""
    if not (hasattr(x, "data_ptr") and x.is_cuda):
        raise TypeError("a torch CUDA tensor is required")
    if x.device.index != ctx.device:
        raise ValueError(f"tensor on {x.device}, context on cuda:{ctx.device}")
    x = x.contiguous()
    return x if dtype is None or x.dtype == dtype else x.to(dtype)


def placed(x, ctx: L.Context):
    """Where an input goes: a torch CUDA tensor on the context's device -> (contiguous fp32 tensor, True) for a _dev entry; a CPU tensor
    or any array -> (contiguous fp32 numpy array, False) for the host entry.  A CUDA tensor on another device is refused."""
    if hasattr(x, "data_ptr"):
        if x.is_cuda:
            import torch
            return device_tensor(x, ctx, torch.float32), True
        x = x.detach().float().numpy()
    return np.ascontiguousarray(x, np.float32), False


def to_device(v, dtype, device, shape=None):
    """Host values as a torch tensor of the numpy dtype (and of that shape) on the device; None stays None.  A contiguous CUDA tensor of that
    dtype on the device is handed through: nothing is uploaded, and the host does not wait for torch's stream as an upload from pageable
    memory makes it."""
    import torch
    if v is None:
        return None
    if isinstance(v, torch.Tensor) and v.is_cuda:
        d = torch.device(device)
        if v.dtype != getattr(torch, np.dtype(dtype).name) or v.device.type != d.type or d.index not in (None, v.device.index) or not v.is_contiguous():
            raise TypeError(f"a contiguous {np.dtype(dtype).name} tensor on {device} is required, not {v.dtype} on {v.device}")
        return v if shape is None else v.reshape(shape)
    v = np.ascontiguousarray(v, dtype)
    return torch.from_numpy(v if shape is None else v.reshape(shape)).to(device)


def dense_strides(x, dense_last: int | None = None) -> list:
    """The element strides of every dimension of a torch tensor but its last, contiguous, one, outermost first: [matrix, row] of a
    [B, T, W] batch.  A dimension of size 1 reports whatever stride its producer left, so the dense one stands in for it (dense_last:
    what a lone row counts as, default W)."""
    out, dense = [], int(x.shape[-1]) if dense_last is None else dense_last
    for d in range(x.dim() - 2, -1, -1):
        out.append(int(x.stride(d)) if x.shape[d] > 1 else dense)
        dense = int(x.shape[d]) * out[-1]
    return out[::-1]
