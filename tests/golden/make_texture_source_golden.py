#!/usr/bin/env python3
"""Mint tests/golden/texture_source_pillow.npz: BC2, BC4 and BC7 blocks decoded by an INDEPENDENT third-party implementation (Pillow's DDS
plugin / BcnDecode.c), the one external pin available offline (the reference hands these blocks to D3D12 and ships no decoder).
DESIGN.md section 3.15's rule, restated in tests/texture_source_ref.py, is held to these bytes by tests/test_texture_source_ref.py.

BC7: 128 random blocks per mode with the mode bits forced (plain random bytes are mode 0 half the time and mode 7 once in 256), then
tests/texture_source_ref.py::structured_blocks: every partition of every partitioned mode (the row, and the anchors), every rotation
with both index selections in mode 4 and every rotation in mode 5, one index bit set at a time, and exactly four reserved-mode blocks
(byte 0 == 0) at the very end, which Pillow 12.2 gives as (0, 0, 0, 255) where the rule says (0, 0, 0, 0). BC2 and BC4: 256 random
blocks each, then the structured ones. Pillow gives BC4 as one channel; it does not know DXGI 75, which shares 74's code words.

    python tests/golden/make_texture_source_golden.py        # needs Pillow; writes the npz next to this script
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE))
from make_bcn_golden import dds, pillow_decode, untile  # noqa: E402
from tests import texture_source_ref as S  # noqa: E402

BC7_RANDOM_PER_MODE, RANDOM_BLOCKS = 128, 256


def main():
    import PIL
    rng = np.random.default_rng(0xBC7135)
    out = {"pillow_version": np.array(PIL.__version__)}
    for name, fmt in (("bc2", S.BC2), ("bc4", S.BC4), ("bc7", S.BC7)):
        per = S.block_bytes(fmt)
        if fmt == S.BC7:
            random = S.force_modes(rng.integers(0, 256, (8 * BC7_RANDOM_PER_MODE, per), dtype=np.uint8))
        else:
            random = rng.integers(0, 256, (RANDOM_BLOCKS, per), dtype=np.uint8)
        blocks = np.concatenate([random, S.structured_blocks(fmt)])
        n, bw = blocks.shape[0], 64
        bh = (n + bw - 1) // bw
        padded = np.zeros((bw * bh, per), np.uint8)
        padded[:, 0] = 0x40 if fmt == S.BC7 else 0  # (BC7 padding: mode 6, not the reserved mode)
        padded[:n] = blocks
        img = pillow_decode(dds(padded, bw, bh, fmt))
        if img.ndim == 2:
            img = img[:, :, None]
        out[f"{name}_blocks"], out[f"{name}_texels"] = blocks, untile(img, bw, n)
        print(f"{name}: {n} blocks ({random.shape[0]} random), Pillow gives {img.shape[2]} channel(s)")
    np.savez_compressed(HERE / "texture_source_pillow.npz", **out)
    print(f"Pillow {PIL.__version__}, {(HERE / 'texture_source_pillow.npz').stat().st_size} bytes")


if __name__ == "__main__":
    sys.exit(main())
