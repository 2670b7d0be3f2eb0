"""The TemporalAA jitter of the host math (ur_host_taa_jitter / ur_host_apply_taa_jitter) against an fp32 restatement of the
reference's Halton loop (DeferredRenderer.cpp:47-67) and its projection offset (:415-421). No GPU needed."""
import numpy as np

F = np.float32


def _halton(index: int, base: int) -> np.float32:
    """Every operation rounded to fp32, in the reference's order."""
    result, fraction, current = F(0.0), F(F(1.0) / F(base)), index
    while current > 0:
        result = F(result + F(F(current % base) * fraction))
        current //= base
        fraction = F(fraction / F(base))
    return result


def _jitter(sample: int) -> np.ndarray:
    return np.array([F(_halton(sample + 1, 2) - F(0.5)), F(_halton(sample + 1, 3) - F(0.5))], F)


def test_jitter_is_the_halton_loop_bit_for_bit(urlib):
    from unclerenderer_amd import hostmath
    for s in range(8):
        got, want = hostmath.taa_jitter(s), _jitter(s)
        assert got.dtype == F and got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (s, got, want)
    # the first three to fp32: (0, -1/6), (-0.25, 1/6), (0.25, -7/18)
    for s, (x, y) in enumerate(((0.0, -1 / 6), (-0.25, 1 / 6), (0.25, -7 / 18))):
        j = hostmath.taa_jitter(s)
        assert j[0] == F(x) and abs(float(j[1]) - y) <= 2.0 ** -24, (s, j)  # (a sum of fp32 terms: within half an ulp of 0.5 of the quotient)


def test_the_eight_samples_of_a_period_are_distinct_and_inside_the_pixel(urlib):
    """The renderer's sample index wraps at 8 (TaaSampleIndex = (TaaSampleIndex + 1) % 8): one period is eight different offsets,
    each inside (-0.5, 0.5), and the function itself is the pure Halton point of the index it is given (sample 8 is not sample 0)."""
    from unclerenderer_amd import hostmath
    pts = [tuple(hostmath.taa_jitter(s).tolist()) for s in range(8)]
    assert len(set(pts)) == 8
    assert all(-0.5 < v < 0.5 for p in pts for v in p)
    assert tuple(hostmath.taa_jitter(8).tolist()) not in pts
    for s in range(8):  # calling again gives the same bits: no state
        assert tuple(hostmath.taa_jitter(s).tolist()) == pts[s]


def test_apply_changes_elements_8_and_9_only(urlib):
    from unclerenderer_amd import hostmath
    proj = hostmath.reverse_z_projection(1.0471976, 16 / 9, 0.1)
    assert proj[8] == 0 and proj[9] == 0
    for s, (w, h) in enumerate(((1920, 1080), (3840, 2160), (515, 67), (130, 9))):
        j = hostmath.taa_jitter(s + 1)
        out = hostmath.apply_taa_jitter(proj, j, w, h)
        keep = [i for i in range(16) if i not in (8, 9)]
        assert out[keep].view(np.uint32).tolist() == proj[keep].view(np.uint32).tolist()
        assert out[8] == F(proj[8] + F(F(F(2.0) * j[0]) / F(w))) and out[9] == F(proj[9] + F(F(F(2.0) * j[1]) / F(h)))
        assert out[8] != 0 and out[9] != 0
        assert abs(float(out[8])) <= 1.0 / w and abs(float(out[9])) <= 1.0 / h  # at most half a pixel of ndc (2 * 0.5 / size)
        assert proj[8] == 0 and proj[9] == 0  # the input is not modified
    # an accumulating caller: applied to an already jittered matrix it adds
    j = hostmath.taa_jitter(1)
    twice = hostmath.apply_taa_jitter(hostmath.apply_taa_jitter(proj, j, 64, 64), j, 64, 64)
    assert twice[8] == F(F(F(2.0) * j[0]) / F(64)) * 2
    # a viewport without area changes nothing (the reference's guard)
    assert hostmath.apply_taa_jitter(proj, j, 0, 1080).tolist() == proj.tolist()
    assert hostmath.apply_taa_jitter(proj, j, 1920, 0).tolist() == proj.tolist()
    # zero jitter (a frame without history) leaves the matrix alone
    assert hostmath.apply_taa_jitter(proj, np.zeros(2, F), 1920, 1080).view(np.uint32).tolist() == proj.view(np.uint32).tolist()
