"""The CullIndirectArgs kernels without a GPU: every instantiation of cull_kernel, compact_kernel and zero_views_kernel in the built library
keeps no scratch and no spills, and no more registers than it had in commit 5393b7c, the last before csrc/cull_kernels.h was split into
cull_params.h, cull_tests.h, cull_compact.h and cull_launch.h: moving text between headers must not change what
the compiler makes of a kernel. Read from the code objects' metadata notes alone."""
import re

import pytest

from tests.code_objects import code_objects, kernel_metadata

# (vgpr_count, sgpr_count) of commit 5393b7c's library; no kernel of it had scratch or a spill
CULL = {  # <SINGLE_BLOCK, RANGES, VIEWS>
    (False, False, False): (43, 47), (False, True, False): (43, 47), (True, False, False): (38, 47), (True, True, False): (39, 52),
    (False, False, True): (45, 50), (False, True, True): (45, 50), (True, False, True): (54, 54), (True, True, True): (54, 54),
}
COMPACT = {  # <RANGES, VIEWS>
    (False, False): (35, 25), (True, False): (52, 46), (False, True): (44, 52), (True, True): (44, 52),
}
ZERO = (5, 12)  # one copy in each of the two modules


@pytest.fixture(scope="module")
def kernels(tmp_path_factory, urlib):
    """[(mangled name, metadata)] of every cull kernel, code object by code object (the zeroing kernel has the same name in both modules)."""
    from unclerenderer_amd import lib
    out = []
    for co in code_objects(lib.library_path(), tmp_path_factory.mktemp("code_objects")):
        out += [(k, m) for k, m in kernel_metadata(co).items() if re.search(r"\d+(cull_kernel|compact_kernel|zero_views_kernel)", k)]
    return out


def _check(name, flags, m, bound):
    print(name, flags, m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, flags, m)
    assert m["vgpr_count"] <= bound[0] and m["sgpr_count"] <= bound[1], (name, flags, m, bound)


@pytest.mark.parametrize("name, bounds", [("cull_kernel", CULL), ("compact_kernel", COMPACT)])
def test_cull_instantiations(kernels, name, bounds):
    flags = len(next(iter(bounds)))
    forms = {}
    for mangled, m in kernels:
        found = re.search(r"\d+%sI%sEEv" % (name, "Lb([01])E" * flags), mangled)
        if found:
            key = tuple(g == "1" for g in found.groups())
            assert key not in forms, f"{name}{key} is instantiated in two modules"
            forms[key] = m
    assert sorted(forms) == sorted(bounds), sorted(forms)
    for key, m in forms.items():
        _check(name, key, m, bounds[key])


def test_zeroing_kernels(kernels):
    zero = [m for mangled, m in kernels if "zero_views_kernel" in mangled]
    assert len(zero) == 2, zero
    for m in zero:
        _check("zero_views_kernel", (), m, ZERO)
