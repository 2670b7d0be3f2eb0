"""Meshes for the mesh-build tests: name -> (buffer bytes, primitive dicts of tests/mesh_ref.py). Built once,
with fixed seeds; the restatement's answer for each is computed once (expected) and left unchanged."""
import json
from pathlib import Path

import numpy as np

from tests import mesh_ref as R

ASSETS = Path(__file__).resolve().parent / "golden" / "assets"
LANE_SEGMENT = 32  # the longest segment a lane sums on its own (csrc/mesh_rule.h, kLaneSegment)
Z = (0.0, 0.0, 1.0)


def _one(*args, **kwargs):
    data, prim = R.make_primitive(*args, **kwargs)
    return data, [prim]


def quad():
    """Two triangles over the unit square, uv = (x, y): tangent (1, 0, 0); the second quad has v flipped: the other handedness."""
    p = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (2, 0, 0), (3, 0, 0), (3, 1, 0), (2, 1, 0)]
    uv = [(0, 0), (1, 0), (1, 1), (0, 1), (0, 0), (1, 0), (1, -1), (0, -1)]
    return _one(p, [0, 1, 2, 0, 2, 3, 4, 5, 6, 4, 6, 7], normals=[Z] * 8, uvs=uv)


def flat_uv():
    """A triangle whose uv are one point (|det| < 1e-8: skipped), and two vertices no triangle names, |N.x| on either side of 0.99."""
    p = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (5, 5, 5), (6, 6, 6)]
    n = [Z, Z, Z, (0.98, 0.0, 0.19899749), (0.995, 0.0, 0.09987492)]
    return _one(p, [0, 1, 2], normals=n, uvs=[(0.5, 0.5)] * 5)


def grid(side, seed, *, zero_normals=0, tangents=False, ctype=5125, interleave=False, uv_scale=1.0):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:side, 0:side]
    p = np.stack([xs, ys, np.zeros_like(xs)], -1).reshape(-1, 3).astype(np.float32)
    p += rng.uniform(-0.3, 0.3, p.shape).astype(np.float32)
    uv = (p[:, :2] * np.float32(uv_scale / side)).astype(np.float32)
    n = rng.normal(size=p.shape).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True).astype(np.float32)
    for v in rng.choice(len(p), zero_normals, replace=False):
        n[v] = 0
    a = (ys[:-1, :-1] * side + xs[:-1, :-1]).reshape(-1)
    idx = np.stack([a, a + 1, a + side + 1, a, a + side + 1, a + side], 1).reshape(-1)
    t = None
    if tangents:
        t = np.concatenate([n[:, [1, 2, 0]], np.ones((len(p), 1), np.float32)], 1)
    return _one(p, idx, normals=n, uvs=uv, tangents=t, ctype=ctype, interleave=interleave)


def soup(seed=7, vertices=1000, triangles=5000):
    """Random triangles with repeated indices, zero-determinant triangles, a few zero normals and a few indices out of range."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-4, 4, (vertices, 3)).astype(np.float32)
    uv = rng.uniform(0, 1, (vertices, 2)).astype(np.float32)
    n = rng.normal(size=(vertices, 3)).astype(np.float32)
    n[rng.choice(vertices, 5, replace=False)] = 0
    idx = rng.integers(0, vertices, (triangles, 3))
    idx[10:20, 1] = idx[10:20, 0]          # a vertex named twice
    idx[30, :] = idx[30, 0]                # ... and three times
    uv[idx[40:50].reshape(-1)] = uv[idx[40, 0]]  # zero determinants
    idx[60, 2], idx[61, 0], idx[62, 1] = vertices, vertices + 7, 0xFFFFFFFF
    return _one(p, idx.reshape(-1), normals=n, uvs=uv)


def fans(big=5000, second=300):
    """A fan of `big` triangles around vertex 0 and a vertex of valence `second`: two entries in the long-segment queue, the first longer than
    a workgroup's LDS tile."""
    rng = np.random.default_rng(11)
    ring = big + 1
    angle = np.linspace(0, 2 * np.pi, ring, dtype=np.float32)
    p = np.concatenate([[(0, 0, 0.5)], np.stack([np.cos(angle), np.sin(angle), np.zeros(ring, np.float32)], 1) * rng.uniform(0.5, 2.0, (ring, 1))]).astype(np.float32)
    extra = rng.uniform(3, 5, (second + 2, 3)).astype(np.float32)
    p = np.concatenate([p, extra])
    base = ring + 1
    fan = np.stack([np.zeros(big, np.int64), np.arange(1, big + 1), np.arange(2, big + 2)], 1)
    rng.shuffle(fan)  # corner order in memory is triangle order, not ring order
    star = np.stack([np.full(second, base), base + 1 + np.arange(second), base + 1 + (np.arange(second) + 1) % second], 1)
    uv = rng.uniform(0, 1, (len(p), 2)).astype(np.float32)
    n = rng.normal(size=p.shape).astype(np.float32)
    n[3] = 0  # both passes run
    return _one(p, np.concatenate([fan, star]).reshape(-1), normals=n, uvs=uv)


def valence(k):
    """One vertex named by exactly k corners (k - 1 triangles name it once, one names it twice)."""
    rng = np.random.default_rng(100 + k)
    p = rng.uniform(-1, 1, (k + 2, 3)).astype(np.float32)
    tri = [(0, 1 + i, 2 + i) for i in range(k - 2)] + [(0, 0, 1)]
    return _one(p, np.array(tri).reshape(-1), uvs=rng.uniform(0, 1, (k + 2, 2)).astype(np.float32))


def count(vertices):
    """`vertices` vertices without normals or tangents; triangles over the first min(vertices, 40) of them and one on the last."""
    rng = np.random.default_rng(vertices)
    p = rng.uniform(-1, 1, (vertices, 3)).astype(np.float32)
    last = vertices - 1
    head = min(vertices, 40)
    idx = [i % head for i in range(max(head, 3))] + [last, last, 0]
    idx = idx[:len(idx) // 3 * 3]
    return _one(p, idx, uvs=rng.uniform(0, 1, (vertices, 2)).astype(np.float32))


def modes(ctype):
    """Three primitives, a list, a strip of 5 and a fan of 5, indices of one width."""
    rng = np.random.default_rng(ctype)
    parts = []
    for mode, idx in ((4, [0, 1, 2, 2, 1, 3, 4, 5, 6]), (5, [0, 1, 2, 3, 4]), (6, [0, 1, 2, 3, 4])):
        p = rng.uniform(-1, 1, (7, 3)).astype(np.float32)
        parts.append(R.make_primitive(p, idx, uvs=rng.uniform(0, 1, (7, 2)).astype(np.float32), ctype=ctype, mode=mode))
    return R.join(parts)


def hand():
    rng = np.random.default_rng(3)
    tri = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    uv3 = [(0, 0), (1, 0), (0, 1)]
    cases = {"quad": quad(), "flat_uv": flat_uv()}
    cases["zero_normal"] = _one(tri + [(1, 1, 0)], [0, 1, 2, 1, 3, 2], normals=[Z, Z, (0, 0, 0), Z], uvs=uv3 + [(1, 1)], tangents=[(1, 0, 0, 1)] * 4)
    cases["one_bad_tangent"] = _one(tri + [(1, 1, 0)], [0, 1, 2, 1, 3, 2], normals=[Z] * 4, uvs=uv3 + [(1, 1)], tangents=[(1, 0, 0, 1)] * 3 + [(0, 0, 0, 1)])
    cases["strip5"] = _one(rng.uniform(-1, 1, (5, 3)), [0, 1, 2, 3, 4], uvs=rng.uniform(0, 1, (5, 2)), mode=5)
    cases["fan5"] = _one(rng.uniform(-1, 1, (5, 3)), [0, 1, 2, 3, 4], uvs=rng.uniform(0, 1, (5, 2)), mode=6)
    cases["vec3_colour"] = _one(tri, [0, 1, 2], normals=[Z] * 3, uvs=uv3, colors=[(0.1, 0.2, 0.3)] * 3)
    cases["vec4_colour"] = _one(tri, [0, 1, 2], normals=[Z] * 3, uvs=uv3, colors=[(0.1, 0.2, 0.3, 0.4)] * 3)
    cases["bare"] = _one(tri, [0, 1, 2])
    cases["two_primitives"] = R.join([R.make_primitive(tri, [0, 1, 2], uvs=uv3), R.make_primitive(tri + [(1, 1, 1)], [0, 2, 3, 1, 2, 3], uvs=uv3 + [(1, 1)], ctype=5123)])
    cases["twice"] = _one(tri + [(1, 1, 0)], [0, 1, 2, 3, 3, 1], uvs=uv3 + [(1, 1)])
    cases["out_of_range"] = _one(tri + [(1, 1, 0)], [0, 1, 2, 1, 3, 4], uvs=uv3 + [(1, 1)])
    nan = np.float32(np.nan)
    cases["nan_bounds"] = _one([(nan, 1, 0), (2, nan, 0), (3, -1, -0.0), (-5, 4, 0.0)], [0, 1, 2, 1, 2, 3], normals=[Z] * 4, tangents=[(1, 0, 0, 1)] * 4)
    return cases


def fixture(name):
    """(buffer, [primitive dicts per mesh], the parsed gltf)."""
    folder, gltf_name = {"Box": ("BoxTextured", "BoxTextured.gltf"), "Duck": ("Duck", "Duck.gltf"), "CompareNormal": ("CompareNormal", "CompareNormal.gltf")}[name]
    gltf = json.loads((ASSETS / folder / gltf_name).read_text())
    data = (ASSETS / folder / gltf["buffers"][0]["uri"]).read_bytes()
    return data, [R.gltf_primitives(gltf, m)[0] for m in range(len(gltf["meshes"]))], gltf


def gpu_cases():
    cases = dict(hand())
    cases["grid33"] = grid(33, 5, uv_scale=1.0)
    cases["grid33_zero_normals"] = grid(33, 6, zero_normals=3)
    cases["soup"] = soup()
    cases["fans"] = fans()
    cases["valence_at_bound"] = valence(LANE_SEGMENT)
    cases["valence_above_bound"] = valence(LANE_SEGMENT + 1)
    for ctype in (5121, 5123, 5125):
        cases[f"modes_{ctype}"] = modes(ctype)
    cases["interleaved"] = grid(9, 8, interleave=True)
    cases["packed"] = grid(9, 8)
    cases["tangents_valid"] = grid(9, 9, tangents=True)
    for n in (1, 255, 256, 257, 65537):
        cases[f"count_{n}"] = count(n)
    for name in ("Box", "Duck", "CompareNormal"):
        data, meshes, _ = fixture(name)
        for m, prims in enumerate(meshes):
            cases[f"{name}_{m}"] = (data, prims)
    return cases


_CASES, _EXPECTED = {}, {}


def case(name):
    if not _CASES:
        _CASES.update(gpu_cases())
    return _CASES[name]


def names():
    if not _CASES:
        _CASES.update(gpu_cases())
    return sorted(_CASES)


def expected(name):
    """The restatement's (vertices, indices, sections, info) of a case: computed once, read-only."""
    if name not in _EXPECTED:
        data, prims = case(name)
        vertices, indices, sections, info = R.build(data, prims)
        vertices.setflags(write=False), indices.setflags(write=False)
        _EXPECTED[name] = (vertices, indices, sections, info)
    return _EXPECTED[name]


def host_primitives(prims):
    from unclerenderer_amd import hostmath
    out = []
    for prim in prims:
        prim = dict(prim)
        out.append(hostmath.mesh_primitive(prim.pop("vertex_count"), prim.pop("position"), prim.pop("indices"), **prim))
    return out
