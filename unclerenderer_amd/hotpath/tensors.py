"""The torch plumbing of the binding: addresses, sizes, host <-> device copies and the one path from a caller's payload to a device tensor."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np
import torch

from ..payload import host_bytes  # noqa: F401  (re-exported)


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA/HIP tensors"
    return C.c_void_p(t.data_ptr())


def nbytes(t) -> int:
    """Bytes of a tensor's elements."""
    return t.numel() * t.element_size()


def on_stream(hp):
    """`with on_stream(hp):` around the torch work a wrapper does on the caller's behalf - allocations, fills, uploads - so that it is
    queued on the context's stream like the launches that use it, whatever torch's current stream is; and torch's allocator, which hands a
    freed block out again in the order of the stream it was allocated on, then orders the reuse of a dropped scratch buffer behind the
    launches still in flight. Nothing changes where the context's stream is the current one, or for a stand-in context without a stream."""
    stream = getattr(hp, "stream", None)
    if stream is None or stream == torch.cuda.current_stream(stream.device):
        return contextlib.nullcontext()
    return torch.cuda.stream(stream)


def to_device(a: np.ndarray, device=0) -> torch.Tensor:
    """numpy -> device tensor, reinterpreting unsigned dtypes torch cannot hold (bit patterns are preserved)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(f"cuda:{device}")


def to_host(t: torch.Tensor, dtype) -> np.ndarray:
    return t.detach().cpu().numpy().view(dtype)


def device_bytes(x, need: int, device, what, reinterpret: bool = False):
    """A payload of exactly `need` bytes on the device: a tensor is passed through, anything else goes through host_bytes and, once its
    size is right, is uploaded (a copy of it) by tensors.to_device(array, device) - the one upload of every payload. A wrong size raises
    ValueError(what(bytes the payload has)) before anything is uploaded."""
    tensor = isinstance(x, torch.Tensor)  # (looked up in the module at call time)
    if not tensor:
        x = host_bytes(x, reinterpret)
    have = nbytes(x) if tensor else x.size
    if have != need:
        raise ValueError(what(have))
    return x if tensor else to_device(x.copy(), device)  # (a module global: patched in one place)
