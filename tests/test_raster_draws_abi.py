"""One table of ur_raster_draws cases through every consumer, without a GPU: the four direct calls (ur_shadow_map, ur_depth_prepass,
ur_gbuffer_pass, ur_gbuffer_pass_materials) and the three frame setters (ur_frame_set_shadow_pass / _depth_pass / _gbuffer_pass) must
give the same verdict on the same draws, and a refusal must name the function that was called.

A direct call that accepts its draws would go on to launch on the stand-in context, so each one carries a stopper: an argument the
function checks only after the draws (a perspective light, an unknown flag bit, rows = 0). Reaching the stopper - its code and its
word in the error text - is that call's "accepted"; the setters return UR_OK. Every refusal of the draws is UR_EINVAL without the
stopper's word."""
import ctypes as C

import numpy as np
import pytest

from tests.test_shadow_abi import ORTHO, _stand_ins

PERSPECTIVE = ORTHO.copy()
PERSPECTIVE[11] = 1.0
IDENTITY = np.eye(4, dtype=np.float32).reshape(-1)


RANGES = ("idx", 2, "cmds", "cnt")  # a whole ur_draw_ranges: offsets, range_count, commands, counts

# name -> (accepted, the fields of ur_raster_draws that differ from every slot of `cmds`, its ranges, target offset or None for a null
# target, stats offset). A buffer is named, ("name", k) is that buffer k bytes on.
CASES = {
    "every slot": (True, {}, None, 0, 0),
    "a list": (True, {"visible_idx": "idx", "visible_count": "cnt"}, None, 0, 0),
    "a list with an index base": (True, {"visible_idx": "idx", "visible_count": "cnt", "index_base": 7}, None, 0, 0),
    "ranges": (True, {}, RANGES, 0, 0),
    "ranges, null commands outside": (True, {"commands": None}, RANGES, 0, 0),
    "ranges, misaligned commands outside": (True, {"commands": ("cmds", 8)}, RANGES, 0, 0),  # the slots live in the ranges' commands
    "no slot, null commands": (True, {"commands": None, "command_count": 0}, None, 0, 0),
    "no slot in ranges": (True, {"commands": None, "command_count": 0}, RANGES, 0, 0),
    "a list without its count": (False, {"visible_idx": "idx"}, None, 0, 0),
    "a count without its list": (False, {"visible_count": "cnt"}, None, 0, 0),
    "a list and ranges": (False, {"visible_idx": "idx", "visible_count": "cnt"}, RANGES, 0, 0),
    "a count and ranges": (False, {"visible_count": "cnt"}, RANGES, 0, 0),
    "ranges without offsets": (False, {}, (None, 2, "cmds", "cnt"), 0, 0),
    "ranges without commands": (False, {}, ("idx", 2, None, "cnt"), 0, 0),
    "ranges without counts": (False, {}, ("idx", 2, "cmds", None), 0, 0),
    "no range": (False, {}, ("idx", 0, "cmds", "cnt"), 0, 0),
    "slots without commands": (False, {"commands": None}, None, 0, 0),
    "commands off 16 bytes": (False, {"commands": ("cmds", 8)}, None, 0, 0),
    "visible_idx off 4 bytes": (False, {"visible_idx": ("idx", 2), "visible_count": "cnt"}, None, 0, 0),
    "visible_count off 4 bytes": (False, {"visible_idx": "idx", "visible_count": ("cnt", 2)}, None, 0, 0),
    "the ranges' commands off 16 bytes": (False, {}, ("idx", 2, ("cmds", 4), "cnt"), 0, 0),
    "the ranges' offsets off 4 bytes": (False, {}, (("idx", 2), 2, "cmds", "cnt"), 0, 0),
    "the ranges' counts off 4 bytes": (False, {}, ("idx", 2, "cmds", ("cnt", 1)), 0, 0),
    "the target off 4 bytes": (False, {}, None, 2, 0),
    "the counters off 4 bytes": (False, {}, None, 0, 1),
    "no target": (False, {}, None, None, 0),
}


@pytest.fixture(scope="module")
def world(urlib):
    """The stand-in buffers, a frame over the stand-in context and the seven consumers: name -> (call(draws, target, stats), the code and
    the word of its stopper; None for a setter)."""
    from unclerenderer_amd import lib
    buf, base, ctx = _stand_ins()
    E, U = lib.UR_EINVAL, lib.UR_EUNSUPPORTED
    at = dict(zip(("target", "cmds", "idx", "cnt", "st", "a", "b", "c", "hdr", "keys"), (base + 4096 * k for k in range(1, 11))))
    a, b, c, hdr, keys = (C.c_void_p(at[n]) for n in ("a", "b", "c", "hdr", "keys"))
    frame = C.c_void_p(urlib.ur_frame_create(ctx, None, 2, 0, 1))
    assert frame.value
    persp, ident = lib.fptr(PERSPECTIVE), lib.fptr(IDENTITY)
    tg = lambda k=keys: lib.GBufferTargets(a, b, c, hdr, None, k)  # noqa: E731
    # A stopper works only because each direct call checks its draws, target and counters before the stopper's argument: ur_shadow_map the
    # light's fourth column, ur_depth_prepass its flags, ur_gbuffer_pass* its rows. A call that wrongly accepted bad draws would reach its
    # stopper, count as accepted and fail the comparison below.
    consumers = {
        "ur_shadow_map": (lambda d, t, s: urlib.ur_shadow_map(ctx, persp, C.byref(d), t, 64, 64, s), (U, "orthographic")),
        "ur_depth_prepass": (lambda d, t, s: urlib.ur_depth_prepass(ctx, ident, ident, C.byref(d), t, 64, 64, 2, s), (E, "flag")),
        "ur_gbuffer_pass": (lambda d, t, s: urlib.ur_gbuffer_pass(ctx, ident, ident, C.byref(d), t, C.byref(tg()), 64, 64, 0, 0, 0, 0, s), (E, "rows")),
        "ur_gbuffer_pass_materials": (lambda d, t, s: urlib.ur_gbuffer_pass_materials(ctx, ident, ident, C.byref(d), t, C.byref(tg()), 64, 64, 0, 0, 0, 0, s, None, 0),
                                      (E, "rows")),
        "ur_frame_set_shadow_pass": (lambda d, t, s: urlib.ur_frame_set_shadow_pass(frame, C.byref(lib.FrameShadowPass(d, t, s))), None),
        "ur_frame_set_depth_pass": (lambda d, t, s: urlib.ur_frame_set_depth_pass(frame, C.byref(lib.FrameDepthPass(d, t, s, 0))), None),
        "ur_frame_set_gbuffer_pass": (lambda d, t, s: urlib.ur_frame_set_gbuffer_pass(frame, C.byref(lib.FrameGBufferPass(d, tg(t), s, 0, 0))), None),  # (its target: the keys)
    }
    yield at, consumers
    urlib.ur_frame_destroy(frame)
    del buf


@pytest.mark.parametrize("name", list(CASES))
def test_every_consumer_gives_the_same_verdict_on_the_same_draws(urlib, world, name):
    from unclerenderer_amd import lib
    at, consumers = world
    OK, E = lib.UR_OK, lib.UR_EINVAL
    accepted, fields, ranges, target_off, stats_off = CASES[name]

    def address(v):  # a buffer's name, (name, offset), or a plain value
        if isinstance(v, tuple):
            return C.c_void_p(at[v[0]] + v[1])
        return C.c_void_p(at[v]) if isinstance(v, str) else v

    d = lib.RasterDraws(C.c_void_p(at["cmds"]), 4, None, None, 0, None)
    for k, v in fields.items():
        setattr(d, k, address(v))
    if ranges is not None:
        rg = lib.DrawRanges(*(address(v) for v in ranges))
        d.ranges = C.pointer(rg)
    target = C.c_void_p(at["target"] + target_off) if target_off is not None else None
    verdicts = {}
    for who, (call, stopper) in consumers.items():
        rc = call(d, target, C.c_void_p(at["st"] + stats_off))
        text = urlib.ur_last_error().decode() if rc != OK else ""
        if stopper is not None and rc == stopper[0] and stopper[1] in text:
            verdicts[who] = OK  # the draws passed: the call came as far as its stopper
        else:
            verdicts[who] = rc
            if rc != OK:
                assert text.startswith(who + ":"), (who, text)
                assert stopper is None or stopper[1] not in text, (who, text)
    assert set(verdicts.values()) == {OK if accepted else E}, verdicts
