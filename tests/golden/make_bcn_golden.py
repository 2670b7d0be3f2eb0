#!/usr/bin/env python3
"""Mint tests/golden/bcn_pillow.npz: BC1, BC3 and BC5 blocks decoded by an INDEPENDENT third-party implementation (Pillow's DDS plugin /
BcnDecode.c). The reference hands these blocks to D3D12 and the texture unit decodes them (Source/Render/TextureLoader.cpp:178-315); it
ships no decoder, so Pillow is the one external pin available offline. DESIGN.md section 3.13's integer rule, restated in
tests/bcn_ref.py, is held to these bytes by tests/test_bcn_ref.py.

Every bit pattern is a valid block: the random blocks are random bytes. The structured ones (tests/bcn_ref.py::structured_blocks) are equal
endpoints, both orders of the endpoints under every index, and one index bit set at a time through all 32 and all 48 index bits.
Pillow gives BC1 and BC3 as RGBA and BC5 as RGB with B = 0. It does not know DXGI 72 and 78: the _SRGB forms share their twins' code words.

    python tests/golden/make_bcn_golden.py        # needs Pillow; writes the npz next to this script
"""
import io
import struct
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
from tests import bcn_ref  # noqa: E402

RANDOM_BLOCKS = 1024


def dds(blocks: np.ndarray, bw: int, bh: int, dxgi: int) -> bytes:
    """A DX10-header DDS of bw x bh blocks (row-major), one level."""
    per = blocks.shape[1]
    assert blocks.shape == (bw * bh, per)
    hdr = struct.pack("<4sIIIIIII44xIIIIIIIIIIII4x", b"DDS ", 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000, 4 * bh, 4 * bw, bw * bh * per, 0, 1,
                      32, 0x4, 0x30315844, 0, 0, 0, 0, 0, 0x1000, 0, 0, 0)
    assert len(hdr) == 128, len(hdr)
    return hdr + struct.pack("<IIIII", dxgi, 3, 0, 1, 0) + blocks.tobytes()


def pillow_decode(data: bytes) -> np.ndarray:
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


def untile(img: np.ndarray, bw: int, n: int) -> np.ndarray:
    """(4 bh, 4 bw, c) image -> (n, 16, c) per-block texels, row-major inside a block."""
    bh, c = img.shape[0] // 4, img.shape[2]
    return img.reshape(bh, 4, bw, 4, c).transpose(0, 2, 1, 3, 4).reshape(bh * bw, 16, c)[:n]


def main():
    import PIL
    rng = np.random.default_rng(0xBC135)
    out = {"pillow_version": np.array(PIL.__version__)}
    for name, fmt in (("bc1", bcn_ref.BC1), ("bc3", bcn_ref.BC3), ("bc5", bcn_ref.BC5)):
        per = bcn_ref.block_bytes(fmt)
        blocks = np.concatenate([rng.integers(0, 256, (RANDOM_BLOCKS, per), dtype=np.uint8), bcn_ref.structured_blocks(fmt)])
        n, bw = blocks.shape[0], 64
        bh = (n + bw - 1) // bw
        padded = np.zeros((bw * bh, per), np.uint8)
        padded[:n] = blocks
        img = pillow_decode(dds(padded, bw, bh, fmt))
        out[f"{name}_blocks"], out[f"{name}_texels"] = blocks, untile(img, bw, n)
        print(f"{name}: {n} blocks ({RANDOM_BLOCKS} random), Pillow gives {img.shape[2]} channels")
    np.savez_compressed(HERE / "bcn_pillow.npz", **out)
    print(f"Pillow {PIL.__version__}, {(HERE / 'bcn_pillow.npz').stat().st_size} bytes")


if __name__ == "__main__":
    sys.exit(main())
