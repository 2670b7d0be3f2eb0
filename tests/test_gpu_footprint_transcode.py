"""Footprint rules (tests/footprint.py, run_rules unchanged) for ur_texture_transcode: it reads exactly the
source chain's bytes and writes exactly the destination chain's. Source and destination sit between guards; the write rule (hash
guards) and the read rule (0xFF and zero guards, plain tensors) hold for the 20 x 12 chain with its edge blocks, for destinations and
sources placed off a 16-byte boundary, and for a chain of one block."""
import numpy as np
import pytest

from tests import footprint as fp
from tests import texture_source_ref as S

pytestmark = pytest.mark.gpu

POISON = 0x5A


def _guarded_transcode(hotpath, urlib, fmt, shape, aligns=None):
    from unclerenderer_amd import lib
    w, h, mips = shape
    data = S.random_chain(fmt, w, h, mips, seed=fmt + 31 * w)
    size = S.rgba8_chain_bytes(w, h, mips)
    assert int(urlib.ur_texture_transcode_bytes(w, h, mips)) == size

    def call(b):
        lib.check(urlib.ur_texture_transcode(hotpath.ctx, fmt, b["blocks"].data_ptr(), w, h, mips, b["rgba8"].data_ptr(), None), "ur_texture_transcode")

    got = fp.run_rules(call, {"blocks": data}, {"rgba8": np.full(size, POISON, np.uint8)}, aligns=aligns, row_bytes={"rgba8": 4 * w, "blocks": S.block_bytes(fmt)},
                       what=f"ur_texture_transcode, format {fmt}, {shape}, aligns {aligns}")
    assert np.array_equal(got["rgba8"], S.transcode_chain(fmt, data, w, h, mips))


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_the_20_x_12_chain(hotpath, urlib, fmt):
    _guarded_transcode(hotpath, urlib, fmt, (20, 12, 5))


@pytest.mark.parametrize("fmt", [71, S.BC4, 77, S.BC7])
@pytest.mark.parametrize("dst_align", [4, 8, 16])
def test_misaligned_placements(hotpath, urlib, fmt, dst_align):
    """The destination 4, 8 and 16 bytes behind a 512-byte boundary; the source of an 8-byte format 8 bytes behind one, else 16."""
    _guarded_transcode(hotpath, urlib, fmt, (20, 12, 5), aligns={"rgba8": dst_align, "blocks": S.block_bytes(fmt)})


@pytest.mark.parametrize("fmt", [71, S.BC2, S.BC7_SRGB])
@pytest.mark.parametrize("shape", [(4, 4, 1), (1, 1, 1), (3, 2, 1)])
def test_a_chain_of_one_block(hotpath, urlib, fmt, shape):
    _guarded_transcode(hotpath, urlib, fmt, shape, aligns={"rgba8": 4})
