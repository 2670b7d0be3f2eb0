"""Device side of the textured GBuffer tests: upload tests/gbuffer_tex_ref.py materials (hotpath.pack_texture / pack_materials)."""
from __future__ import annotations

from tests import gbuffer_tex_ref as X


def device_materials(materials):
    """The ur_material table of a list of gbuffer_tex_ref materials; a Tex with valid=False keeps its texels and gets a
    descriptor broken the way its `how` says."""
    from unclerenderer_amd import hotpath, lib
    packed = []
    for m in materials:
        rec = {"key": m.get("key", 0)}
        for name, _, _ in X.MAPS:
            t = m.get(name)
            if t is None:
                continue
            tex = hotpath.pack_texture(t.levels, t.srgb)
            if not t.valid:
                d = tex.desc
                f = {"texels": d.texels, "width": d.width, "height": d.height, "mips": d.mips, "format": d.format}
                f.update({"format": {"format": 0}, "null": {"texels": 0}, "misaligned": {"texels": d.texels + 2}, "width": {"width": 0}, "height": {"height": 0},
                          "mips": {"mips": 0}}[t.how])
                tex = hotpath.Texture(tex.buffer, lib.Texture2D(f["texels"], f["width"], f["height"], f["mips"], f["format"], 0))
            rec[name] = tex
        packed.append(rec)
    return hotpath.pack_materials(packed)
