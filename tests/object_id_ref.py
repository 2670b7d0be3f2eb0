"""The ObjectId rule restated in numpy: what ur_object_id_pass and ur_object_id_pick must compute, to the byte.

Nothing in the rule is new, so nothing is restated twice: the fragments that pass GREATER_EQUAL against a given depth - the vertex rule, the
near clip, the viewport, facing, coverage, the depth plane, D24 and the counters - are tests/gbuffer_mask_ref.py's `fragments` (section
3.11's rule 2, which is section 3.9's raster with every passing fragment kept), called as it is over ONE selection that holds the opaque and
the masked draws alike; the key's split and the selections are tests/gbuffer_ref.py's. This file adds what the pass does with them: no alpha
test, the greatest key per texel, the ObjectId word of that key's command, and for a pick the clamp of the point, the slot and the depth of
the winning key's fragment (the greatest, should two pieces of one cut triangle pass at one texel).

The planted errors of tests/test_object_id_ref.py are switches here, all off by default.
"""
from __future__ import annotations

import numpy as np

from tests import gbuffer_mask_ref as M
from tests import gbuffer_ref as G

NO_SLOT = 0xFFFFFFFF
MAX_POINTS = 64


def image(draws, view, proj, depth, w: int, h: int, flags: int = 0, select=None, key_triangle_bits: int = 0, command_count=None,
          wrong_nearest: bool = False, wrong_greater: bool = False, wrong_alpha=None):
    """ur_object_id_pass over the whole target (a band is rows of it). select: gbuffer_ref.selection(...), default every slot. Returns keys,
    object_id, slot (NO_SLOT for key 0) and depth_bits (the winning fragment's, 0 for key 0) as (h, w) uint32, and stats[0:6] (stats[3] is
    structural and stays 0). The planted errors: wrong_nearest takes the nearest passing fragment, not the greatest key; wrong_greater tests
    GREATER, not GREATER_EQUAL; wrong_alpha (a function (slot, texels) -> discarded) applies an alpha test."""
    command_count = len(draws) if command_count is None else command_count
    T = G.key_bits(command_count, key_triangle_bits)
    select = [(k, k) for k in range(len(draws))] if select is None else list(select)
    depth = np.asarray(depth, np.float32).reshape(h, w)
    texel, zbits, keys, stats = M.fragments(draws, view, proj, depth, w, h, flags, select, T)
    slot_of = dict(select)
    if wrong_greater:
        keep = zbits.view(np.float32) > depth.reshape(-1)[texel]
        texel, zbits, keys = texel[keep], zbits[keep], keys[keep]
    if wrong_alpha is not None:
        slots = np.array([slot_of[int(k >> T) - 1] for k in keys], np.int64)
        keep = np.ones(texel.size, bool)
        for s in np.unique(slots):
            keep[slots == s] = ~wrong_alpha(int(s), texel[slots == s])
        texel, zbits, keys = texel[keep], zbits[keep], keys[keep]
    hi, lo = (zbits, keys) if wrong_nearest else (keys, zbits)
    word = np.zeros(h * w, np.uint64)
    np.maximum.at(word, texel, (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64))
    hi, lo = (word >> np.uint64(32)).astype(np.uint32), (word & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    key_image, bits = (lo, hi) if wrong_nearest else (hi, lo)
    ids = np.array([d.constants().view(np.uint32)[148] for d in draws], np.uint32)
    slot = np.full(h * w, NO_SLOT, np.uint32)
    won = np.flatnonzero(key_image)
    slot[won] = [slot_of[int(k >> T) - 1] for k in key_image[won]]
    object_id = np.zeros(h * w, np.uint32)
    object_id[won] = ids[slot[won]]
    return {"keys": key_image.reshape(h, w), "object_id": object_id.reshape(h, w), "slot": slot.reshape(h, w), "depth_bits": bits.reshape(h, w),
            "stats": stats}


def clamp_points(points, w: int, h: int, wrong_unclamped: bool = False) -> np.ndarray:
    """(n, 2) of (min(x, w - 1), min(y, h - 1)) over unsigned 32-bit coordinates. The planted error wraps them into the frame instead."""
    p = np.asarray(points, np.int64).reshape(-1, 2) & 0xFFFFFFFF
    if wrong_unclamped:
        return np.stack([p[:, 0] % w, p[:, 1] % h], axis=1)
    return np.stack([np.minimum(p[:, 0], w - 1), np.minimum(p[:, 1], h - 1)], axis=1)


def pick(img, points, w: int, h: int, wrong_unclamped: bool = False) -> np.ndarray:
    """ur_object_id_pick's records, (n, 4) uint32 of (object_id, key, slot, depth_bits): an image(...) result at the clamped points."""
    p = clamp_points(points, w, h, wrong_unclamped)
    assert p.shape[0] <= MAX_POINTS
    return np.stack([img[k][p[:, 1], p[:, 0]] for k in ("object_id", "keys", "slot", "depth_bits")], axis=1).astype(np.uint32)


def every_texel(w: int, h: int, per_call: int = MAX_POINTS):
    """The texels of a w x h frame as lists of at most per_call (x, y) points, row-major."""
    pts = [(x, y) for y in range(h) for x in range(w)]
    return [pts[k:k + per_call] for k in range(0, len(pts), per_call)]
