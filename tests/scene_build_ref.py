"""A numpy restatement, in fp32, of what the reference does between its built meshes and its first frame, for ur_scene_build
(include/ur_scene_build.h). Written from the reference's lines, not from csrc/scene_rule.h:

  RendererUtils.cpp:402-410   World = NodeWorld * Scale * RotationRollPitchYaw * Translation (XMMatrixMultiply: row vectors, every element
                              the sum ((a0 b0 + a1 b1) + a2 b2) + a3 b3, as csrc/scene.cpp restates it)
  RendererUtils.cpp:418-440   the eight corners (x from bit 0, y from bit 1, z from bit 2) through XMVector3TransformCoord, which divides by
                              w; std::min / std::max from +-FLT_MAX
  RendererUtils.cpp:288-295   ComputeMaxScale over the node matrix
  RendererUtils.cpp:470-476   centre through World, radius = mesh radius * model scale * node scale
  RendererUtils.cpp:277-286   UpdateSceneBounds: centre +- radius; :533-540 scene centre and radius
  RendererUtils.cpp:1029-1088 UpdateSceneConstants: the record's fields by name
  RendererUtils.h:102-111     FIndirectDrawCommand; DeferredRenderer.cpp:3301-3366 how its words are filled

numpy's float32 arithmetic rounds every product and sum on its own, and its divide and square root are IEEE's. Everything is done over
all draws at once; `plant` puts one wrong reading in, for the tests that hold the checks themselves."""
import numpy as np

NODE = np.dtype([("node_world", "<f4", 16), ("scale", "<f4", 3), ("max_scale", "<f4"), ("rotation", "<f4", 9), ("translate", "<f4", 3), ("reserved", "<u4", 4)])
MESH = np.dtype([("vertices", "<u8"), ("indices", "<u8"), ("vertex_bytes", "<u4"), ("index_bytes", "<u4"), ("stride", "<u4"), ("index_format", "<u4")])
INFO = np.dtype([("min", "<f4", 3), ("max", "<f4", 3), ("center", "<f4", 3), ("radius", "<f4"), ("counters", "<u4", 4)])
FACTORS = np.dtype([("BaseColor", "<f4", 3), ("BaseColorAlpha", "<f4"), ("EmissiveFactor", "<f4", 3), ("MetallicFactor", "<f4"), ("RoughnessFactor", "<f4"),
                    ("AlphaCutoff", "<f4"), ("AlphaMode", "<u4"), ("Padding", "<u4"), ("transforms", "<f4", (8, 4))])
DRAW = np.dtype([(n, "<u4") for n in ("node", "mesh", "material", "constants_slot", "object_id", "index_start", "index_count", "reserved")])
SUMMARY = np.dtype([("scene_min", "<f4", 3), ("scene_max", "<f4", 3), ("scene_center", "<f4", 3), ("scene_radius", "<f4"), ("draw_count", "<u4"), ("skipped_draws", "<u4")])
# FSceneConstants (RendererUtils.h:41-79)
CONSTANTS = np.dtype([("World", "<f4", 16), ("View", "<f4", 16), ("ViewInverse", "<f4", 16), ("Projection", "<f4", 16), ("BaseColor", "<f4", 3), ("LightIntensity", "<f4"),
                      ("LightDirection", "<f4", 3), ("Padding1", "<f4"), ("CameraPosition", "<f4", 3), ("Padding2", "<f4"), ("LightColor", "<f4", 3), ("Padding3", "<f4"),
                      ("EmissiveFactor", "<f4", 3), ("Padding4", "<f4"), ("LightViewProjection", "<f4", 16), ("ShadowStrength", "<f4"), ("ShadowBias", "<f4"),
                      ("ShadowMapSize", "<f4", 2), ("MetallicFactor", "<f4"), ("RoughnessFactor", "<f4"), ("BaseColorAlpha", "<f4"), ("AlphaCutoff", "<f4"),
                      ("AlphaMode", "<u4"), ("PaddingMaterial", "<u4", 3), ("transforms", "<f4", (8, 4)), ("EnvMapMipCount", "<f4"), ("PaddingEnvMap", "<f4", 3),
                      ("ObjectId", "<u4"), ("PaddingObjectId", "<f4", 3)])
assert (NODE.itemsize, MESH.itemsize, INFO.itemsize, FACTORS.itemsize, DRAW.itemsize, SUMMARY.itemsize, CONSTANTS.itemsize) == (144, 32, 56, 176, 32, 48, 608)
FLT_MAX = np.float32(3.402823466e38)
PLANTS = ("product_order", "no_divide", "corner_order", "slot_is_command_index", "template_over_factors", "radius_without_node_scale")


def rm_mul(A, B):
    """XMMatrixMultiply over [D, 4, 4] float32 arrays."""
    R = np.empty_like(A)
    for i in range(4):
        for j in range(4):
            R[:, i, j] = ((A[:, i, 0] * B[:, 0, j] + A[:, i, 1] * B[:, 1, j]) + A[:, i, 2] * B[:, 2, j]) + A[:, i, 3] * B[:, 3, j]
    return R


def transform_coord(M, p, divide=True):
    """XMVector3TransformCoord of [D, 3] points by [D, 4, 4] matrices."""
    r = [((p[:, 0] * M[:, 0, j] + p[:, 1] * M[:, 1, j]) + p[:, 2] * M[:, 2, j]) + M[:, 3, j] for j in range(4)]
    return np.stack([r[j] / r[3] if divide else r[j] for j in range(3)], axis=1)


def std_min(a, b):
    return np.where(b < a, b, a)


def std_max(a, b):
    return np.where(a < b, b, a)


def place(nodes, infos, plant=None):
    """World [D, 4, 4], bounds min / max [D, 3], centre [D, 3], radius [D] of draws given their node and info records ([D] each)."""
    D = len(nodes)
    f = np.float32
    NW = nodes["node_world"].reshape(D, 4, 4).astype(f)
    S, R, T = np.zeros((D, 4, 4), f), np.zeros((D, 4, 4), f), np.zeros((D, 4, 4), f)
    for k in range(3):
        S[:, k, k] = nodes["scale"][:, k]
    S[:, 3, 3] = 1
    R[:, :3, :3] = nodes["rotation"].reshape(D, 3, 3)
    R[:, 3, 3] = 1
    for k in range(4):
        T[:, k, k] = 1
    T[:, 3, :3] = nodes["translate"]
    World = rm_mul(rm_mul(rm_mul(NW, S), R), T) if plant != "product_order" else rm_mul(NW, rm_mul(S, rm_mul(R, T)))
    lo, hi = np.full((D, 3), FLT_MAX, f), np.full((D, 3), -FLT_MAX, f)
    corners = range(8) if plant != "corner_order" else reversed(range(8))
    for corner in corners:
        p = np.stack([infos["max"][:, a] if corner & (1 << a) else infos["min"][:, a] for a in range(3)], axis=1)
        w = transform_coord(World, p, plant != "no_divide")
        lo, hi = std_min(lo, w), std_max(hi, w)
    node_scale = np.zeros(D, f)
    for c in range(3):
        node_scale = std_max(node_scale, np.sqrt((NW[:, 0, c] * NW[:, 0, c] + NW[:, 1, c] * NW[:, 1, c]) + NW[:, 2, c] * NW[:, 2, c]))
    center = transform_coord(World, infos["center"], plant != "no_divide")
    radius = (infos["radius"] * nodes["max_scale"]) * node_scale if plant != "radius_without_node_scale" else infos["radius"] * nodes["max_scale"]
    return World, lo, hi, center, radius


def total_order_min(values):
    """The minimum of a float32 vector and FLT_MAX where a NaN is ignored and -0 lies below +0."""
    v = np.concatenate([values[~np.isnan(values)], [FLT_MAX]]).astype(np.float32)
    m = v.min()
    return np.float32(-0.0) if m == 0 and np.signbit(v[v == 0]).any() else m


def total_order_max(values):
    v = np.concatenate([values[~np.isnan(values)], [-FLT_MAX]]).astype(np.float32)
    m = v.max()
    return np.float32(0.0) if m == 0 and (~np.signbit(v[v == 0])).any() else m


def scene_summary(center, radius, live, draw_count):
    s = np.zeros((), SUMMARY)
    with np.errstate(all="ignore"):
        for a in range(3):
            s["scene_min"][a] = total_order_min((center[live, a] - radius[live]).astype(np.float32))
            s["scene_max"][a] = total_order_max((center[live, a] + radius[live]).astype(np.float32))
        e2 = np.float32(0)
        for a in range(3):
            s["scene_center"][a] = np.float32(0.5) * (s["scene_min"][a] + s["scene_max"][a])
            e2 = e2 + (s["scene_max"][a] - s["scene_min"][a]) * (s["scene_max"][a] - s["scene_min"][a])
        half = np.sqrt(e2) * np.float32(0.5)
        s["scene_radius"] = np.float32(1.0) if half < np.float32(1.0) else half  # std::max(half, 1.0f)
    s["draw_count"], s["skipped_draws"] = draw_count, draw_count - int(live.sum())
    return s


def build(nodes, meshes, infos, materials, draws, frame, slot_count, stride=608, constants_address=0, *, transforms_only=False, out=None, plant=None):
    """The five outputs as a dict of numpy arrays (bounds float32 [D, 2, 4], commands uint32 [D, 16], constants uint8 [slot_count, stride],
    centers float32 [D, 4], summary uint8 [48]). frame: 608 bytes (anything np.frombuffer takes). out: the arrays' content before the call
    (copied), else zeros: what the call leaves alone keeps it."""
    nodes, meshes, infos = np.asarray(nodes).view(NODE).reshape(-1), np.asarray(meshes).view(MESH).reshape(-1), np.asarray(infos).view(INFO).reshape(-1)
    materials, draws = np.asarray(materials).view(FACTORS).reshape(-1), np.asarray(draws).view(DRAW).reshape(-1)
    D = len(draws)
    if out is None:
        out = {"bounds": np.zeros((D, 2, 4), np.float32), "commands": np.zeros((D, 16), np.uint32), "constants": np.zeros((slot_count, stride), np.uint8),
               "centers": np.zeros((D, 4), np.float32), "summary": np.zeros(48, np.uint8)}
    out = {k: (v.copy() if v is not None else None) for k, v in out.items()}
    live = (draws["node"] < len(nodes)) & (draws["mesh"] < len(meshes)) & (draws["material"] < len(materials)) & (draws["constants_slot"] < slot_count)
    at = np.flatnonzero(live)
    d = draws[at]
    with np.errstate(all="ignore"):
        World, lo, hi, center, radius = place(nodes[d["node"]], infos[d["mesh"]], plant)
    bounds = np.zeros((D, 2, 4), np.float32)
    bounds[at, 0, :3], bounds[at, 1, :3] = lo, hi
    out["bounds"][...] = bounds
    centers = np.zeros((D, 4), np.float32)
    centers[at, :3], centers[at, 3] = center, radius
    if out.get("centers") is not None:
        out["centers"][...] = centers
    out["summary"][...] = np.frombuffer(scene_summary(centers[:, :3], centers[:, 3], live, D).tobytes(), np.uint8)

    slot = d["constants_slot"].astype(np.int64) if plant != "slot_is_command_index" else at.astype(np.int64)
    records = out["constants"][:, :608].copy().view(CONSTANTS).reshape(-1)  # [slot_count]
    if transforms_only:
        records["World"][slot] = World.reshape(-1, 16)
    else:
        new = np.repeat(np.frombuffer(bytes(frame), CONSTANTS, 1), len(at))
        m = materials[d["material"]]
        new["World"] = World.reshape(-1, 16)
        if plant != "template_over_factors":
            for name in ("BaseColor", "EmissiveFactor", "MetallicFactor", "RoughnessFactor", "BaseColorAlpha", "AlphaCutoff", "AlphaMode", "transforms"):
                new[name] = m[name]
        new["ObjectId"] = d["object_id"]
        records[slot] = new
        mesh = meshes[d["mesh"]]
        address = (np.uint64(constants_address) + slot.astype(np.uint64) * np.uint64(stride)).astype(np.uint64)
        commands = np.zeros((D, 16), np.uint32)
        c = np.zeros((len(at), 16), np.uint32)
        c[:, 0], c[:, 1], c[:, 2], c[:, 3] = mesh["vertices"] & np.uint64(0xFFFFFFFF), mesh["vertices"] >> np.uint64(32), mesh["vertex_bytes"], mesh["stride"]  # VertexBufferView
        c[:, 4], c[:, 5], c[:, 6], c[:, 7] = mesh["indices"] & np.uint64(0xFFFFFFFF), mesh["indices"] >> np.uint64(32), mesh["index_bytes"], mesh["index_format"]  # IndexBufferView
        c[:, 8], c[:, 9] = address & np.uint64(0xFFFFFFFF), address >> np.uint64(32)  # ConstantBufferAddress
        c[:, 10], c[:, 11], c[:, 12], c[:, 13], c[:, 14] = d["index_count"], 1, d["index_start"], 0, slot  # DrawIndexedArguments
        commands[at] = c
        out["commands"][...] = commands
    out["constants"][:, :608] = records.view(np.uint8).reshape(-1, 608)
    return out


def frame_template(seed=7):
    """608 bytes of a constants template in which every word is different, material fields included: a build that kept one of them shows."""
    words = (np.arange(152, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(seed)) & np.uint32(0x3FFFFFFF) | np.uint32(0x3C000000)
    return words.tobytes()


def rotation_roll_pitch_yaw(pitch, yaw, roll):
    """The upper 3 x 3 of XMMatrixRotationRollPitchYaw, row-major, in fp32."""
    f = np.float32
    cp, sp, cy, sy, cr, sr = (f(g(f(a))) for a in (pitch, yaw, roll) for g in (np.cos, np.sin))
    return np.array([cr * cy + sr * sp * sy, sr * cp, sr * sp * cy - cr * sy, cr * sp * sy - sr * cy, cr * cp, sr * sy + cr * sp * cy, cp * sy, -sp, cp * cy], f)


def seeded_tables(seed, D, slot_count=None):
    """Tables of D draws for the byte-equality tests: shared nodes (about D / 3 of them), five meshes, seven materials, slots a
    permutation of more slots than draws, node matrices with w columns that are not (0, 0, 0, 1), negative and zero scales, signed zeros,
    a NaN mesh box, an infinite one, a node whose w is 0, and - from D = 8 on - one draw with each kind of out-of-range index."""
    rng = np.random.default_rng(seed)
    f = np.float32
    n_nodes, n_meshes, n_materials = max(1, D // 3), 5, 7
    slot_count = D + 3 if slot_count is None else slot_count
    nodes = np.zeros(n_nodes, NODE)
    base = np.tile(np.eye(4, dtype=f).reshape(-1), (n_nodes, 1))
    spread = np.tile(np.array([1, 1, 1, 0.05] * 4, f), (n_nodes, 1))  # the w column stays near (0, 0, 0, 1): w != 1, seldom near 0
    nodes["node_world"] = base + rng.choice(np.array([0, 0, 0, 0.25, -0.5, 1.5], f), (n_nodes, 16)) * rng.standard_normal((n_nodes, 16)).astype(f) * spread
    zeros = rng.random((n_nodes, 16)) < 0.1
    zeros[:, 15] = False
    nodes["node_world"][zeros] = f(-0.0)
    nodes["node_world"][::5, 3::4] = (0, 0, 0, 1)  # every fifth an affine matrix
    if n_nodes >= 3:
        nodes["node_world"][n_nodes - 1, 3::4] = 0  # w == 0 for every point
    nodes["scale"] = rng.choice(np.array([1, 1, 2, -1, 0.5, -3, 0, -0.0], f), (n_nodes, 3))
    nodes["max_scale"] = np.abs(nodes["scale"]).max(axis=1)
    if n_nodes >= 3:
        nodes["node_world"][1] = np.eye(4, dtype=f).reshape(-1)
        nodes["node_world"][1, 3], nodes["node_world"][1, 15] = 1, 0  # w = x
        nodes["scale"][1] = (1, 0, 1)
    nodes["max_scale"] = np.abs(nodes["scale"]).max(axis=1)
    eulers = rng.choice(np.array([0, 0, 90, -45, 30, 180], f), (n_nodes, 3)) * f(3.14159265358979 / 180.0)
    nodes["rotation"] = np.stack([rotation_roll_pitch_yaw(*e) for e in eulers])
    nodes["translate"] = rng.choice(np.array([0, -0.0, 1, -2.5, 100, 1e-3], f), (n_nodes, 3))
    if n_nodes >= 3:
        nodes["rotation"][1], nodes["translate"][1] = np.eye(3, dtype=f).reshape(-1), 0
    infos = np.zeros(n_meshes, INFO)
    lo = rng.uniform(-2, 0, (n_meshes, 3)).astype(f)
    hi = (lo + rng.uniform(0, 3, (n_meshes, 3))).astype(f)
    lo[1], hi[1] = (-1, -1, -1), (1, 1, 1)
    lo[2, 0] = hi[2, 1] = np.nan   # a NaN mesh box
    hi[3, 2] = np.inf
    lo[4], hi[4] = (-0.0, 0, -1), (0.0, 0, 1)
    infos["min"], infos["max"] = lo, hi
    with np.errstate(all="ignore"):
        infos["center"] = f(0.5) * (lo + hi)
        e = hi - lo
        r = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) * f(0.5)
    infos["radius"] = np.where(r < 1, f(1), r)
    infos["counters"] = rng.integers(0, 9, (n_meshes, 4))
    meshes = np.zeros(n_meshes, MESH)
    meshes["vertices"] = 0x7F0000000000 + rng.integers(0, 1 << 30, n_meshes).astype(np.uint64) * 64
    meshes["indices"] = 0x7E0000000000 + rng.integers(0, 1 << 30, n_meshes).astype(np.uint64) * 4
    meshes["vertex_bytes"], meshes["index_bytes"] = rng.integers(64, 1 << 20, n_meshes) * 64, rng.integers(3, 1 << 20, n_meshes) * 4
    meshes["stride"], meshes["index_format"] = 64, 42
    materials = np.frombuffer(rng.integers(0, 1 << 32, n_materials * 44, dtype=np.uint64).astype(np.uint32).tobytes(), FACTORS).copy()
    draws = np.zeros(D, DRAW)
    draws["node"], draws["mesh"], draws["material"] = rng.integers(0, n_nodes, D), rng.choice([0, 1, 4], D), rng.integers(0, n_materials, D)
    draws["mesh"][7::16] = rng.choice([2, 3], len(draws["mesh"][7::16]))  # the NaN and the infinite box are rare: the scene box stays finite on most axes
    if n_nodes >= 3:
        draws["node"][3::64], draws["mesh"][3::64] = n_nodes - 1, 1  # w == 0: infinite bounds, a NaN centre
        draws["node"][5::64], draws["mesh"][5::64] = 1, 1  # y = +0 / w with w = -1 and +1 over the unit box: -0 and +0 meet in the corner walk
    draws["constants_slot"] = rng.permutation(slot_count)[:D]
    draws["object_id"] = np.arange(1, D + 1)
    draws["index_start"], draws["index_count"] = rng.integers(0, 1 << 20, D) * 3, rng.integers(1, 1 << 16, D) * 3
    if D >= 8:
        draws["node"][1], draws["mesh"][2], draws["material"][4], draws["constants_slot"][D - 1] = n_nodes, 0xFFFFFFFF, n_materials, slot_count
    return nodes, meshes, infos, materials, draws, slot_count
