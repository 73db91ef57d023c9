"""What the fused SuGaR stages (sugar_field, sugar_mesh, sugar_dynamic, sugar_arap, sugar_spline) share on the Python
side: argument checks, the buffers of a call and the incidence tables of the bindings.  No public API."""
from __future__ import annotations

import torch

from diff_gaussian_rasterization import _C as _gsr

INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def float_tensor(t, name, shape):
    """t, a float32 tensor of the given shape (None: any size)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 tensor")
    if t.dim() != len(shape) or any(s is not None and int(t.shape[i]) != s for i, s in enumerate(shape)):
        want = ", ".join("*" if s is None else str(s) for s in shape)
        raise ValueError(f"{name} must have shape ({want}), got {tuple(t.shape)}")
    return t


def aligned(t, alignment=16):
    """t contiguous and aligned (a view at an odd storage offset is copied)."""
    t = t.contiguous()
    return t if t.data_ptr() % alignment == 0 else t.clone()


def on_gpu(fn, first, others, error=ValueError):
    """The device of ``first``, a GPU that every tensor of ``others`` ((name, tensor or None) pairs) is on too."""
    dev = first.device
    if dev.type != "cuda":
        raise error(f"{fn} requires tensors on a ROCm GPU (device 'cuda'): there is no CPU path")
    for name, t in others:
        if t is not None and t.device != dev:
            raise error(f"{name} is on {t.device}, expected {dev}")
    return dev


def workspace(nbytes, dev):
    return torch.empty((int(nbytes),), dtype=torch.uint8, device=dev)


def ups(grads, dev):
    """The upstream gradients as contiguous, aligned float32 tensors on dev (None stays None)."""
    out = (None if g is None else _gsr._f32(g, "upstream gradient", dev) for g in grads)
    return [None if g is None else aligned(g) for g in out]


def incidence(flat, n):
    """Of a flat int64 index with entries in [0, n): ``(order, offsets)``, both int32: the positions grouped by entry,
    ascending within an entry (a stable sort), and entry j owning ``order[offsets[j]:offsets[j + 1]]``."""
    order = torch.sort(flat, stable=True)[1].to(torch.int32).contiguous()
    return order, row_offsets(torch.bincount(flat, minlength=n))


def row_offsets(counts):
    """(n + 1,) int32 offsets of rows with the given (n,) counts."""
    offsets = torch.zeros(int(counts.shape[0]) + 1, dtype=torch.int64, device=counts.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets.to(torch.int32).contiguous()


class Binding:
    """A binding's ``device`` and ``to(device)``: a copy whose tensors named in ``_TENSORS`` are moved."""

    _TENSORS = ()

    @property
    def device(self):
        return getattr(self, self._TENSORS[0]).device

    def to(self, device):
        other = object.__new__(type(self))
        other.__dict__.update(self.__dict__)
        for name in self._TENSORS:
            setattr(other, name, getattr(self, name).to(device))
        return other
