"""Materials of BC textures for the GPU tests of DESIGN.md section 3.13: every texture of a list of gbuffer_tex_ref materials is replaced by
random blocks (every bit pattern is a valid block) in a format that cycles per command and per map, RGBA8 among them, and its `levels`
become the decoded texels by tests/bcn_ref.py - the RGBA8 twin. The numpy restatements (gbuffer_tex_ref, gbuffer_mask_ref, forward_ref)
read the twin; the device gets the blocks (device_materials) or, for the comparison run, the twin itself (as_rgba8=True)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import bcn_ref as R
from tests import gbuffer_tex_ref as X

KINDS = ("bc1", "bc3", "rgba8", "bc5", "bc3", "bc1", "bc5")  # 7 entries against 5 shapes, 4 maps and 16 keys: every pairing comes up
SHAPES = [(1, 1, 1), (3, 5, 3), (20, 12, 5), (64, 64, 7), (1000, 600, 3)]  # (width, height, mips); 20 x 12 with its full chain


@dataclass
class BcTex(X.Tex):
    """A gbuffer_tex_ref.Tex whose levels are the decode of `data` (the chain's blocks) in `fmt`; fmt 28 / 29 with data None: plain RGBA8.
    With valid=False and how="misaligned" the device descriptor's address is moved by half a block (4 bytes for BC1, 8 for BC3 and BC5)."""
    fmt: int = 28
    data: np.ndarray = None


def bc_texture(kind: str, w: int, h: int, mips: int, srgb: bool, seed: int, punch_through: bool = False) -> BcTex:
    if kind == "rgba8":
        t = X.random_texture(w, h, mips, srgb, np.random.default_rng(seed))
        return BcTex(t.levels, srgb, fmt=29 if srgb else 28)
    fmt = {"bc1": R.BC1_SRGB if srgb else R.BC1, "bc3": R.BC3_SRGB if srgb else R.BC3, "bc5": R.BC5}[kind]
    data = R.random_chain(fmt, w, h, mips, seed, punch_through)
    return BcTex(R.decode_chain(fmt, data, w, h, mips), R.is_srgb(fmt), fmt=fmt, data=data)


def bc_materials(mats, seed: int, shapes=SHAPES, kinds=KINDS, masked_slots=()):
    """`mats` (keys and which maps exist are kept) with every texture replaced: shape (k + j) % len(shapes), kind (k + 3 j) % len(kinds) for
    map j of command k. The base colour of a slot in masked_slots is BC1 with punch-through blocks, or BC3 (random alpha), alternating."""
    out = []
    for k, m in enumerate(mats):
        rec = {"key": m["key"]}
        for j, (name, _, _) in enumerate(X.MAPS):
            if m.get(name) is None:
                continue
            w, h, mips = shapes[(k + j) % len(shapes)]
            kind = kinds[(k + 3 * j) % len(kinds)]
            punch = False
            if j == 0 and k in masked_slots:
                kind = "bc1" if (k // 3) % 2 == 0 else "bc3"
                punch = True
            rec[name] = bc_texture(kind, w, h, mips, m[name].srgb, seed * 1000 + 4 * k + j, punch)
        out.append(rec)
    return out


def formats_in(mats) -> set:
    return {m[name].fmt for m in mats for name, _, _ in X.MAPS if m.get(name) is not None}


def texture_bytes(t: BcTex) -> np.ndarray:
    """The device buffer's bytes of a texture: its blocks, or its packed RGBA8 levels."""
    return t.data if t.data is not None else np.concatenate([a.reshape(-1) for a in t.levels])


def descriptor(t: BcTex, address: int, as_rgba8: bool = False):
    from unclerenderer_amd import lib
    fmt = (29 if t.srgb else 28) if as_rgba8 else t.fmt
    if not t.valid:
        assert t.how == "misaligned" and not as_rgba8
        address += R.block_bytes(fmt) // 2
    return lib.Texture2D(address, t.width, t.height, len(t.levels), fmt, 0)


def device_materials(mats, as_rgba8: bool = False):
    """The ur_material table of bc_materials(...): the blocks as they are (hotpath.pack_texture_bc), or with as_rgba8 every twin uploaded as
    R8G8B8A8_UNORM[_SRGB] (hotpath.pack_texture). A misaligned texture gets 16 bytes of its own in front, so that the moved descriptor's
    chain still lies inside the allocation."""
    from unclerenderer_amd import hotpath
    packed = []
    for m in mats:
        rec = {"key": m["key"]}
        for name, _, _ in X.MAPS:
            t = m.get(name)
            if t is None:
                continue
            if as_rgba8 or t.data is None:
                assert t.valid
                rec[name] = hotpath.pack_texture(t.levels, t.srgb)
            elif t.valid:
                rec[name] = hotpath.pack_texture_bc(t.data, t.width, t.height, len(t.levels), t.fmt)
            else:
                buffer = hotpath.to_device(np.concatenate([t.data, np.zeros(16, np.uint8)]))
                rec[name] = hotpath.Texture(buffer, descriptor(t, buffer.data_ptr()))
        packed.append(rec)
    return hotpath.pack_materials(packed)
