"""The binding's one payload path without a GPU: payload.host_bytes over every kind of input it takes, hotpath.tensors.device_bytes with a
stand-in tensor class and a patched upload, and the device every HotPath method uploads to (the context's, not device 0)."""
import numpy as np
import pytest

from tests.test_mesh_abi import _prim


def test_host_bytes_over_its_inputs():
    from unclerenderer_amd.payload import host_bytes  # numpy only
    raw = bytes(range(1, 13))
    for x in (raw, bytearray(raw), memoryview(raw), memoryview(bytearray(raw)), np.frombuffer(raw, np.uint8), np.frombuffer(raw, np.uint8).reshape(3, 4)):
        for reinterpret in (False, True):
            got = host_bytes(x, reinterpret)
            assert got.dtype == np.uint8 and got.ndim == 1 and got.flags.c_contiguous and got.tobytes() == raw, type(x)
    a = np.arange(24, dtype=np.uint8)
    got = host_bytes(a[::2])  # a slice with a stride: gathered
    assert got.flags.c_contiguous and got.tobytes() == bytes(range(0, 24, 2)) and not np.shares_memory(got, a)
    assert host_bytes(a.reshape(4, 6)[:, ::3]).tobytes() == a.reshape(4, 6)[:, ::3].tobytes()
    assert host_bytes(b"").size == 0 and host_bytes(np.zeros(0, np.uint8)).size == 0


def test_host_bytes_casts_by_value_or_reinterprets():
    from unclerenderer_amd.payload import host_bytes
    h = np.array([0x0102, 0x00FF, 0xABCD, 7], np.uint16)
    viewed = host_bytes(h, reinterpret=True)
    assert viewed.dtype == np.uint8 and viewed.size == 2 * h.size and viewed.tobytes() == h.tobytes()  # the same bit patterns
    assert host_bytes(h.reshape(2, 2), reinterpret=True).tobytes() == h.tobytes()
    assert host_bytes(h[::2], reinterpret=True).tobytes() == h[::2].tobytes()
    cast = host_bytes(h)  # today's value cast, pinned and not judged
    want = np.ascontiguousarray(h, np.uint8).reshape(-1)
    assert cast.dtype == np.uint8 and cast.size == h.size and np.array_equal(cast, want)
    f = np.array([1.5, -2.0], np.float32)
    assert host_bytes(f, reinterpret=True).tobytes() == f.tobytes() and host_bytes(f, reinterpret=True).size == 8


def test_nothing_aliases_a_writable_buffer_of_the_caller(monkeypatch):
    """bytes-likes are copied by host_bytes; a contiguous uint8 array comes back as a view, and device_bytes copies it before the upload,
    as every call site did."""
    from unclerenderer_amd import hotpath
    from unclerenderer_amd.payload import host_bytes
    b = bytearray(b"abcdefgh")
    for x in (b, memoryview(b)):
        got = host_bytes(x)
        b[0] ^= 0xFF
        assert got.tobytes() == b"abcdefgh"
        b[0] ^= 0xFF
    a = np.arange(8, dtype=np.uint8)
    w = np.arange(4, dtype=np.uint16)
    uploaded = []
    monkeypatch.setattr(hotpath.tensors, "to_device", lambda array, device: uploaded.append(array) or "on the device")
    assert hotpath.tensors.device_bytes(a, 8, 0, None) == "on the device"
    assert hotpath.tensors.device_bytes(w, 8, 0, None, reinterpret=True) == "on the device"
    assert hotpath.tensors.device_bytes(b, 8, 0, None) == "on the device"
    assert len(uploaded) == 3 and not np.shares_memory(uploaded[0], a) and not np.shares_memory(uploaded[1], w)
    assert all(u.flags.writeable and u.dtype == np.uint8 for u in uploaded)
    assert uploaded[0].tobytes() == a.tobytes() and uploaded[1].tobytes() == w.tobytes() and uploaded[2].tobytes() == bytes(b)


class T:  # a stand-in for a device tensor: an address and a size (tests/test_env_cube_abi.py)
    is_cuda = True

    def __init__(self, address, nbytes):
        self.address, self.nbytes = address, nbytes

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.address

    def numel(self):
        return self.nbytes // 2

    def element_size(self):
        return 2


def test_device_bytes_checks_the_size_then_uploads_once(monkeypatch):
    from unclerenderer_amd import hotpath
    tensors = hotpath.tensors
    monkeypatch.setattr(hotpath.torch, "Tensor", T)
    calls = []
    monkeypatch.setattr(tensors, "to_device", lambda array, device: calls.append((array, device)) or ("uploaded", device))
    what = lambda have: f"the thing is 48 bytes, the payload has {have}"  # noqa: E731
    for bad in (bytes(47), bytearray(49), np.zeros(24, np.uint8), b"", T(0x1000, 46)):
        with pytest.raises(ValueError, match=r"the thing is 48 bytes, the payload has (47|49|24|0|46)$"):
            tensors.device_bytes(bad, 48, 5, what)
    with pytest.raises(ValueError, match="the payload has 24$"):
        tensors.device_bytes(np.zeros(24, np.uint16), 48, 5, what)  # 24 values, cast by value
    assert calls == []  # refused before the upload
    assert tensors.nbytes(T(0, 48)) == 48
    t = T(0x2000, 48)
    assert tensors.device_bytes(t, 48, 5, what) is t and calls == []  # a tensor is passed through, where it is
    assert tensors.device_bytes(bytes(range(48)), 48, 5, what) == ("uploaded", 5)
    assert len(calls) == 1 and calls[0][1] == 5 and calls[0][0].dtype == np.uint8 and calls[0][0].tobytes() == bytes(range(48))
    assert tensors.device_bytes(np.arange(24, dtype=np.uint16), 48, 2, what, reinterpret=True) == ("uploaded", 2)
    assert len(calls) == 2 and calls[1][1] == 2 and calls[1][0].tobytes() == np.arange(24, dtype=np.uint16).tobytes()


class Uploaded(Exception):
    pass


def test_every_upload_of_a_context_goes_to_its_device(urlib, monkeypatch):
    from unclerenderer_amd import hotpath, lib

    class NoDevice(hotpath.HotPath):
        def __init__(self):
            self._L, self._ctx, self.device = urlib, None, 3

    seen = []

    def upload(array, device=0):
        seen.append(device)
        raise Uploaded

    monkeypatch.setattr(hotpath.tensors, "to_device", upload)
    hp = NoDevice()
    calls = {
        "transcode_texture": lambda: hp.transcode_texture(bytes(8), 4, 4, 1, lib.UR_TEXTURE_BC1_UNORM),  # a 4 x 4 BC1 chain of 1 mip
        "build_mesh": lambda: hp.build_mesh(bytes(48), [_prim()]),  # one triangle: three positions, three u32 indices
        "build_env_cube": lambda: hp.build_env_cube(bytes(48), lib.UR_ENV_SOURCE_RGBA16F, 1, 1),  # base 1, 1 mip: six texels of 8 bytes
        "prefilter_env_cube": lambda: hp.prefilter_env_cube(bytes(48), 1, 16),  # a base-1 top level, 16 samples
        "draw_offsets_to_device": lambda: hp.draw_offsets_to_device([0, 1], 1),
    }
    for name, call in calls.items():
        seen.clear()
        with pytest.raises(Uploaded):
            call()
        assert seen == [3], name
