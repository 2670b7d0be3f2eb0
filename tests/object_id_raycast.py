"""What the float64 ray casters (tests/raycast_ref.py, tests/raycast_tex.py) say the ObjectId pass must show, for
the restatement (tests/test_object_id_ref.py) and the kernels (tests/test_gpu_object_id.py) alike. Nothing of the raster rule is used.

Opaque scenes: on raycast_ref.classify's compared texels the id is the winner's draw's, 0 where no ray hits.

The masked scene: the pass has no alpha test and tests GREATER_EQUAL against the depth the masked G-buffer pass left, which is the depth of
the ray's winner (the nearest hit that survives the alpha test). So every hit at or in front of the winner passes - the winner and the
discarded hits in front of it, raycast_tex's `signature` - and the last drawn of them wins: the expected id is that of the greatest slot
among them; on a texel without a winner, of the greatest slot in the signature (every hit passes a clear depth); 0 when no ray hits.
A hit BEHIND the winner fails by its distance; where that distance is within what fp32 depth can confuse - depth_ref.DEPTH_ERROR_BOUND plus
the spread of the winner's depth over the texel's 9 rays - on any of the 9 rays, the texel is left out beside raycast_tex.classify's.
"""
from __future__ import annotations

import numpy as np

from tests import depth_ref as D
from tests import raycast_ref as R
from tests import raycast_tex as T

MASKED_ORDERS = {"ico, torus, grid": (0, 1, 2), "grid, ico, torus": (2, 0, 1)}  # the scene's draws in slot order; the first is the scene's own


def opaque_expectation(sc, rc):
    """(compared (h, w) bool, want (h, w) uint32, left-out share) of a raycast_ref camera scene."""
    compared, _, left_out = R.classify(rc)
    ids = np.array([d.object_id for d in sc.draws], np.uint32)
    want = np.where(rc["hit"][0], ids[np.maximum(rc["draw"][0], 0)], np.uint32(0)).astype(np.uint32)
    return compared, want, left_out


def reordered(sc, order):
    """The masked scene with its draws in the slots `order` names (order[s] = the scene's draw in slot s): (a raycast_tex.Scene over the
    reordered draws and materials, slot_of: the scene's draw -> its slot)."""
    slot_of = {int(d): s for s, d in enumerate(order)}
    moved = T.Scene(sc.name, [sc.draws[d] for d in order], [sc.mats[d] for d in order], sc.view, sc.proj, masked=tuple(sorted(slot_of[d] for d in sc.masked)), eye=sc.eye)
    return moved, slot_of


_HITS = {}


def _near_behind(sc, rc, w, h):
    """(h, w) bool: a ray of the texel has another hit at or behind its winner within DEPTH_ERROR_BOUND + the winner depth's 9-ray spread."""
    if (w, h) not in _HITS:
        _HITS[(w, h)] = R.hits(sc.draws, w, h, sc.view, sc.proj)  # (what raycast_tex.cast cast: rc["index"] counts its hits)
    H = _HITS[(w, h)]
    n = h * w
    winner = rc["index"].reshape(-1)[H["ray"]]
    with np.errstate(all="ignore"):
        spread = np.nan_to_num(R._spread(rc["depth"]).reshape(-1), nan=0.0)
        gap = H["z"][np.maximum(winner, 0)] - H["z"]
        close = (winner >= 0) & (np.arange(H["ray"].size) != winner) & (gap >= 0) & (gap <= D.DEPTH_ERROR_BOUND + spread[H["ray"] % n])
    out = np.zeros(n, bool)
    out[H["ray"][close] % n] = True
    return out.reshape(h, w)


def masked_expectation(sc, rc, w, h, slot_of):
    """(compared, want (h, w) uint32, left-out share, compared by raycast_tex.classify alone) of the masked scene with the scene's draw d in
    slot slot_of[d]. `want` is the ObjectId the module docstring derives; it is meaningful on `compared` only."""
    by_classify, any_hit, _ = T.classify(rc)
    compared = by_classify & ~_near_behind(sc, rc, w, h)
    slots = np.array([slot_of[d] for d in range(len(sc.draws))], np.int64)
    ids = np.zeros(len(sc.draws) + 1, np.uint32)  # by slot + 1; entry 0 = nothing
    for d, s in slot_of.items():
        ids[s + 1] = sc.draws[d].object_id
    best = np.where(rc["hit"][0], slots[np.maximum(rc["draw"][0], 0)] + 1, 0)
    sig = rc["signature"][0]
    for k in range(15):
        digit = (sig >> (4 * k)) & 15
        best = np.maximum(best, np.where(digit != 0, slots[np.maximum(digit - 1, 0)] + 1, 0))
    left_out = float((any_hit & ~compared).sum()) / max(int(any_hit.sum()), 1)
    return compared, ids[best], left_out, by_classify


def held(got_object_id, compared, want):
    """The number of compared texels whose ObjectId is not the expected one."""
    return int((compared & (np.asarray(got_object_id, np.uint32) != want)).sum())
