"""Python face of the C-ABI for device tensors (torch is used for device memory and streams only).

Method names follow the reference's passes: CullIndirectArgs (Renderer.cpp:394 DispatchGpuCulling), BuildHZB
(DeferredRenderer.cpp:998), DeferredLighting (:1219), SkyAtmosphere (:1263).

One module an area: tensors (torch plumbing and the payload path), context, post, raster, builds, frame. A new wrapper is
a method of its area's class, or a function of its area's module that is re-exported here.
"""
from __future__ import annotations

import torch  # noqa: F401  (the tests reach hotpath.torch)

from . import builds, context, frame, post, raster, tensors
from .builds import BuiltScene, Mesh, SceneTables, mesh_draws, mesh_infos  # noqa: F401
from .context import HzbLayout, check_draw_offsets, cull_view, cull_views_array, draw_ranges  # noqa: F401
from .frame import Frame  # noqa: F401
from .post import debug_print_buffer, debug_print_buffer_bytes, post_record_bytes, taa_record_bytes  # noqa: F401
from .raster import (Materials, Texture, forward_targets, gbuffer_targets, pack_draw_commands, pack_materials, pack_texture,  # noqa: F401
                     pack_texture_bc, raster_draws)
from .tensors import to_device, to_host  # noqa: F401


class HotPath(context.Context, post.PostPasses, post.DebugPrint, raster.RasterPasses, builds.AssetBuilds):
    """One ur_ctx bound to a device and a stream."""
