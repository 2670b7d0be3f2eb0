"""The two resolves over the visibility keys without a GPU: every instantiation of gbuffer_resolve_kernel and forward_resolve_kernel in the
built library keeps the registers its occupancy rests on (DESIGN.md sections 3.13 and 3.14). The textured forward kernel sits at its
three-wave bound, where moving text between functions has cost it scratch before; this is the check that says so without a GPU run.
Read from the code objects' metadata notes alone."""
import re

import pytest

from tests.code_objects import library_kernels

# vgpr_count bounds by occupancy step: 512 registers per SIMD in steps of 8: three waves <= 168, six waves <= 80
THREE_WAVES, SIX_WAVES = 168, 80


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return library_kernels(tmp_path_factory.mktemp("code_objects"))


def _instantiations(kernels, name, flags):
    """{(template flags as bools): metadata} of the kernel `name` with `flags` bool template arguments."""
    out = {}
    for mangled, m in kernels.items():
        found = re.search(r"\d+%sI%sEEv" % (name, "Lb([01])E" * flags), mangled)
        if found:
            out[tuple(g == "1" for g in found.groups())] = m
    return out


def test_gbuffer_resolve_instantiations(urlib, kernels):
    """<OBJECT_ID, MAPS, MASKED>: the six forms launch_gbuffer_resolve picks from (no ObjectId beside a mask)."""
    forms = _instantiations(kernels, "gbuffer_resolve_kernel", 3)
    assert sorted(forms) == sorted([(o, m, k) for o in (False, True) for m in (False, True) for k in (False, True) if not (o and k)]), sorted(forms)
    for (object_id, maps, masked), m in forms.items():
        print("gbuffer_resolve_kernel", object_id, maps, masked, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, ((object_id, maps, masked), m)
        assert m["vgpr_count"] <= (THREE_WAVES if maps else SIX_WAVES), ((object_id, maps, masked), m)


def test_forward_resolve_instantiations(urlib, kernels):
    """<MAPS, MASKED>: four forms, all held to three waves per SIMD."""
    forms = _instantiations(kernels, "forward_resolve_kernel", 2)
    assert sorted(forms) == sorted([(m, k) for m in (False, True) for k in (False, True)]), sorted(forms)
    for (maps, masked), m in forms.items():
        print("forward_resolve_kernel", maps, masked, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, ((maps, masked), m)
        assert m["vgpr_count"] <= THREE_WAVES, ((maps, masked), m)
