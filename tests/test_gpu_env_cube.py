"""ur_env_cube_build on the device (include/ur_env_cube.h): byte-equal to ur_host_env_cube_build - which
tests/test_env_cube_ref.py holds to the numpy restatement - over random payloads in the three formats, at edges where a level is smaller
than a block or ends inside one, full chains and single levels, into a destination that arrives as 0xFF and as zero; the info word; the
shipped cube against ur_stage_env_cube; two builds queued into one destination; and the lighting pass over a device-built cube."""
from pathlib import Path

import numpy as np
import pytest

from tests import env_cube_ref as R

pytestmark = pytest.mark.gpu

ASSETS = Path(__file__).parent / "golden" / "assets"
EDGES = (1, 2, 3, 4, 5, 6, 7, 8, 12, 33, 64)
FORMATS = (R.RGBA16F, R.UF16, R.SF16)


@pytest.fixture(scope="module")
def host_built(urlib):
    """{(format, base, mips): (payload, the host build's cube, its reserved count)}: computed once, shared and left unchanged."""
    from unclerenderer_amd import hostmath
    out = {}
    for k, fmt in enumerate(FORMATS):
        for base in EDGES:
            for mips in sorted({1, R.full_chain(base)}):
                payload = R.random_payload(5000 + 100 * k + base, fmt, base, mips)
                cube, bad = hostmath.env_cube_build(payload, fmt, base, mips)
                cube.setflags(write=False)
                out[(fmt, base, mips)] = (payload, cube, bad)
    return out


def device_bytes(t):
    return t.cpu().numpy().view(np.uint16).reshape(-1, 4)


@pytest.mark.parametrize("fill", [0xFF, 0x00])
@pytest.mark.parametrize("fmt", FORMATS)
def test_device_build_is_the_host_build(hotpath, host_built, fmt, fill):
    import torch
    from unclerenderer_amd.hotpath import to_device
    seen_reserved = 0
    for (f, base, mips), (payload, want, bad) in host_built.items():
        if f != fmt:
            continue
        src = to_device(payload)
        dst = torch.full((want.shape[0], 4), -1 if fill else 0, dtype=torch.int16, device=src.device)
        info = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device=src.device)  # a non-zero word planted: the build writes it
        got = hotpath.build_env_cube(src, f, base, mips, info, out=dst)
        assert got is dst
        torch.cuda.synchronize()
        got = device_bytes(dst)
        same = got.view(np.uint8) == want.view(np.uint8)
        assert same.all(), f"format {f}, base {base}, {mips} mips, fill {fill:#x}: {np.count_nonzero(~same)} bytes differ, first at {int(np.flatnonzero(~same.reshape(-1))[0])}"
        assert info.cpu().numpy().tolist() == [bad, 0x5A5A5A5A, 0x5A5A5A5A, 0x5A5A5A5A], (f, base, mips)
        seen_reserved += bad
        # info = NULL: the same bytes
        again = hotpath.build_env_cube(src, f, base, mips)
        torch.cuda.synchronize()
        assert np.array_equal(device_bytes(again), want), (f, base, mips)
    assert (seen_reserved > 0) == (fmt != R.RGBA16F)  # random blocks met reserved modes: the count was not trivially zero


def test_fixture_is_what_stage_env_cube_gives(hotpath):
    """tests/golden/assets/output_pmrem.dds: the device build of the file's payload against HotPath.stage_env_cube over the host decode."""
    import torch
    from unclerenderer_amd import assets
    payload, fmt, base, mips = assets.load_env_cube_dds_source(ASSETS / "output_pmrem.dds")
    texels, base2, mips2, bad = assets.load_env_cube_dds(ASSETS / "output_pmrem.dds")
    info = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    built = hotpath.build_env_cube(payload, fmt, base, mips, info)
    staged = hotpath.stage_env_cube(texels, base2, mips2)
    torch.cuda.synchronize()
    assert (base, mips) == (base2, mips2) == (256, 9) and built.shape == staged.shape and built.dtype == staged.dtype
    assert torch.equal(built, staged) and int(info.item()) == bad == 0


def test_two_builds_queued_into_one_destination(hotpath, host_built):
    """Two different cubes of one shape, built back to back into the same destination with nothing between them: the second one's bytes."""
    import torch
    from unclerenderer_amd import hostmath
    from unclerenderer_amd.hotpath import to_device
    fmt, base, mips = R.SF16, 33, 6
    payload_a, first_want, _ = host_built[(fmt, base, mips)]
    payload_b = R.random_payload(99, fmt, base, mips)
    want_b, bad_b = hostmath.env_cube_build(payload_b, fmt, base, mips)
    assert not np.array_equal(want_b, first_want)
    a, b = to_device(payload_a), to_device(payload_b)
    dst = torch.empty((first_want.shape[0], 4), dtype=torch.int16, device=a.device)
    info = torch.zeros(1, dtype=torch.int32, device=a.device)
    hotpath.build_env_cube(a, fmt, base, mips, info, out=dst)
    hotpath.build_env_cube(b, fmt, base, mips, info, out=dst)
    torch.cuda.synchronize()
    assert np.array_equal(device_bytes(dst), want_b) and int(info.item()) == bad_b


@pytest.mark.parametrize("w,h", [(64, 64), (50, 40)])
def test_lighting_over_a_device_built_cube(hotpath, w, h):
    """ur_deferred_lighting at 64 x 64 (the streaming kernel) and 50 x 40 (the per-tile kernel): over a device-built cube the result is
    byte-equal to the same call over the host-staged one."""
    import torch
    from tests.test_gpu_parity import _lighting_inputs
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import to_device
    fc, g, shadow, env, lut = _lighting_inputs("sponza", w, h, seed=21, mode="scene")
    env = np.ascontiguousarray(env, np.uint16)
    staged = hotpath.stage_env_cube(env, 32, 6)
    built = hotpath.build_env_cube(env.view(np.uint8).reshape(-1), lib.UR_ENV_SOURCE_RGBA16F, 32, 6)
    torch.cuda.synchronize()
    assert torch.equal(built, staged)
    d_shadow, d_lut = to_device(shadow), to_device(lut)
    dA, dB, dC = to_device(g.A), to_device(g.B), to_device(g.C)
    out = []
    for cube in (staged, built):
        hdr = to_device(g.hdr)
        hotpath.deferred_lighting(fc.scene, dA, dB, dC, hotpath.make_tables(d_shadow, cube, 32, 6, d_lut), hdr, w, h)
        torch.cuda.synchronize()
        out.append(hdr.cpu().numpy().view(np.uint16))
    assert np.array_equal(out[0], out[1])
    assert not np.array_equal(out[0], g.hdr.view(np.uint16))  # the pass wrote something
