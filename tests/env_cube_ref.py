"""A numpy restatement of the environment cube build (include/ur_env_cube.h): the walk over a DDS cube payload and the
staging of ur_stage_env_cube - border fold and row pairs - stated here on their own, not by calling the code under test. The BC6H texels of
a block come from ur_bc6h_decode_block, which tests/golden/bc6h_pillow.npz pins to Pillow; everything else is restated:

  payload   six faces, face-major with mips inner; a BC6H level of edge n is ceil(n / 4)^2 blocks, row-major, a block 4 x 4 texels
            row-major, texels past the level's edge dropped; an RGBA16F level is n * n texels of 8 bytes
  fold      a texel of a face's one-texel ring is the interior texel of the neighbouring face that the ring texel's centre lands on when
            the face plane is folded over the shared edge. Stated with points: the centre of texel (i, j) of a face of edge N is the cube
            point of (s, t) = ((2 i + 1) / N - 1, (2 j + 1) / N - 1); a ring texel has |s| or |t| = 1 + 1 / N, and folding moves the
            overshoot 1 / N from that coordinate (which becomes +-1) to the face's own axis (which becomes +-(1 - 1 / N)). A corner first
            clamps j into the face. All of it in integers, times N.
  pairs     behind all bordered levels, every level again: entry (f, j, i), j in [0, E - 2], is R G B of bordered texel (i, j), then R G B
            of (i, j + 1): 12 bytes.

`fault` plants one error (tests/test_env_cube_ref.py: each must change bytes)."""
import ctypes as C

import numpy as np

RGBA16F, UF16, SF16 = 10, 95, 96
FAULTS = ("wrong_face", "swap_ij", "corner_unclamped", "pair_rows_swapped", "pair_alpha", "mips_outer", "wrong_column")

# the cube point (x, y, z) of (s, t) on a face, D3D's order +X -X +Y -Y +Z -Z, and back
POINT = (lambda s, t, one: (one, -t, -s), lambda s, t, one: (-one, -t, s), lambda s, t, one: (s, one, t),
         lambda s, t, one: (s, -one, -t), lambda s, t, one: (s, -t, one), lambda s, t, one: (-s, -t, -one))
BACK = (lambda x, y, z: (-z, -y), lambda x, y, z: (z, -y), lambda x, y, z: (x, z), lambda x, y, z: (x, -z), lambda x, y, z: (x, -y), lambda x, y, z: (-x, -y))


def level_size(base, m):
    return max(1, base >> m)


def source_bytes(fmt, base, mips):
    if fmt not in (RGBA16F, UF16, SF16) or base == 0 or not 1 <= mips <= 16:
        return 0
    return 6 * sum(((level_size(base, m) + 3) // 4) ** 2 * 16 if fmt != RGBA16F else level_size(base, m) ** 2 * 8 for m in range(mips))


def texels_of(base, mips):
    e = [level_size(base, m) + 2 for m in range(mips)]
    return 6 * sum(x * x for x in e) + 9 * sum(x * (x - 1) for x in e)


def decode_block(urlib, block: bytes, signed: bool):
    """(16 texels [4, 4, 4] uint16, decoded?) of one block, by ur_bc6h_decode_block."""
    out = np.zeros((4, 4, 4), np.uint16)
    ok = urlib.ur_bc6h_decode_block(block, 1 if signed else 0, out.ctypes.data_as(C.c_void_p))
    return out, bool(ok)


def walk(urlib, payload, fmt, base, mips, fault=None):
    """The payload as levels[face][m] = [n, n, 4] uint16, and the number of reserved-mode blocks."""
    data = bytes(payload)
    assert len(data) == source_bytes(fmt, base, mips)
    levels = [[None] * mips for _ in range(6)]
    order = [(f, m) for m in range(mips) for f in range(6)] if fault == "mips_outer" else [(f, m) for f in range(6) for m in range(mips)]
    at, bad = 0, 0
    for f, m in order:
        n = level_size(base, m)
        if fmt == RGBA16F:
            levels[f][m] = np.frombuffer(data, np.uint16, n * n * 4, at).reshape(n, n, 4).copy()
            at += n * n * 8
            continue
        across = (n + 3) // 4
        full = np.zeros((4 * across, 4 * across, 4), np.uint16)
        for by in range(across):
            for bx in range(across):
                texels, ok = decode_block(urlib, data[at:at + 16], fmt == SF16)
                at += 16
                bad += 0 if ok else 1
                if fault == "wrong_column" and 4 * bx + 4 > n:  # a partial block: its rightmost columns instead of its leftmost
                    texels = np.roll(texels, -(4 * bx + 4 - n), axis=1)
                full[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = texels
        levels[f][m] = full[:n, :n].copy()
    assert at == len(data)
    return levels, bad


def fold(N, face, i, j, fault=None):
    """(face, i, j) of the interior texel a ring texel copies."""
    i_out, j_out = not 0 <= i < N, not 0 <= j < N
    assert i_out or j_out
    if i_out and j_out and fault != "corner_unclamped":
        j = min(max(j, 0), N - 1)
        j_out = False
    s, t = 2 * i + 1 - N, 2 * j + 1 - N  # times N
    p = list(POINT[face](s, t, N))
    own = face // 2
    for axis in range(3):  # the overshooting coordinate(s) fold over the edge
        if axis != own and abs(p[axis]) > N:
            p[own] -= (abs(p[axis]) - N) * (1 if p[own] > 0 else -1)
            p[axis] = N if p[axis] > 0 else -N
    axis = [a for a in range(3) if a != own and abs(p[a]) == N][0]  # (one alone, but for the planted unclamped corner)
    new = 2 * axis + (0 if p[axis] > 0 else 1)
    if fault == "wrong_face":
        new ^= 1
    s2, t2 = BACK[new](*p)
    i2, j2 = (s2 + N) // 2, (t2 + N) // 2  # s2 + N is odd: the floor of a half-integer
    i2, j2 = min(max(i2, 0), N - 1), min(max(j2, 0), N - 1)
    return (new, j2, i2) if fault == "swap_ij" else (new, i2, j2)


def stage(levels, base, mips, fault=None):
    """The staged cube as uint16 [texels, 4] from levels[face][m]."""
    out = np.zeros((texels_of(base, mips), 4), np.uint16)
    at = 0
    bordered = []
    for m in range(mips):
        N = level_size(base, m)
        E = N + 2
        faces = out[at:at + 6 * E * E].reshape(6, E, E, 4)
        at += 6 * E * E
        for f in range(6):
            faces[f, 1:N + 1, 1:N + 1] = levels[f][m]
        for f in range(6):
            for j in range(-1, N + 1):
                for i in range(-1, N + 1):
                    if 0 <= i < N and 0 <= j < N:
                        continue
                    sf, si, sj = fold(N, f, i, j, fault)
                    faces[f, j + 1, i + 1] = levels[sf][m][sj, si]
        bordered.append(faces)
    pairs = out[at:].reshape(-1).view(np.uint8)
    pos = 0
    for m in range(mips):
        faces = bordered[m]
        E = faces.shape[1]
        keep = 4 if fault == "pair_alpha" else 3
        top, bottom = faces[:, :E - 1, :, :keep], faces[:, 1:, :, :keep]
        if fault == "pair_rows_swapped":
            top, bottom = bottom, top
        entries = np.concatenate([top, bottom], axis=-1).reshape(-1, 2 * keep)
        if fault == "pair_alpha":
            entries = entries[:, :6]  # R G B A R G: the alpha carried into the pair
        raw = np.ascontiguousarray(entries).view(np.uint8).reshape(-1)
        pairs[pos:pos + raw.size] = raw
        pos += raw.size
    assert pos == pairs.size
    return out


def build(urlib, payload, fmt, base, mips, fault=None):
    """(the staged cube as uint16 [texels, 4], reserved-mode blocks): what ur_host_env_cube_build and ur_env_cube_build must give."""
    levels, bad = walk(urlib, payload, fmt, base, mips, fault)
    return stage(levels, base, mips, fault), bad


def random_payload(seed, fmt, base, mips):
    """Random bytes: random 16-byte blocks reach every mode, the reserved ones included; random halves reach NaN, Inf and denormals."""
    return np.random.default_rng(seed).integers(0, 256, source_bytes(fmt, base, mips), dtype=np.uint8)


def full_chain(base):
    return base.bit_length()
