"""A caller's payload as bytes on the host (numpy only: hostmath uses it and stays importable without torch; hotpath.tensors uploads it)."""
from __future__ import annotations

import numpy as np


def host_bytes(x, reinterpret: bool = False) -> np.ndarray:
    """bytes, a bytearray, a memoryview or an array as a flat contiguous uint8 array. An array that is not uint8 is cast by value, or
    with reinterpret=True viewed as the bytes it holds. bytes-likes are copied; a contiguous uint8 array comes back as a view."""
    if isinstance(x, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(x), np.uint8)
    return (np.ascontiguousarray(x).view(np.uint8) if reinterpret else np.ascontiguousarray(x, np.uint8)).reshape(-1)
