"""The public surface of unclerenderer_amd.hotpath (tools/binding_surface.py) against tests/golden/binding_surface.txt, which is the tool's
output on the commit before hotpath became a package: every public name, signature and docstring is where it was. And the checkable form
of "no function is assigned onto a class afterwards": each method of HotPath and Frame was defined in a class body of the package."""
import importlib.util
import inspect
import pathlib

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _tool():
    spec = importlib.util.spec_from_file_location("binding_surface", ROOT / "tools" / "binding_surface.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_surface_has_not_moved():
    from unclerenderer_amd import hotpath
    want = (ROOT / "tests" / "golden" / "binding_surface.txt").read_text()
    got = _tool().surface(hotpath)
    assert len(want.splitlines()) == 116
    missing, extra = sorted(set(want.splitlines()) - set(got.splitlines())), sorted(set(got.splitlines()) - set(want.splitlines()))
    assert got == want, f"missing: {missing}\nnew: {extra}"


def test_every_method_is_defined_in_a_class_body_of_the_package():
    from unclerenderer_amd import hotpath
    modules = [m for m in vars(hotpath).values() if inspect.ismodule(m) and m.__name__.startswith(hotpath.__name__ + ".")]
    classes = {c.__name__ for m in [hotpath, *modules] for c in vars(m).values() if inspect.isclass(c) and c.__module__.startswith(hotpath.__name__)}
    assert {"HotPath", "Frame", "HzbLayout"} <= classes
    for cls in (hotpath.HotPath, hotpath.Frame):
        seen = 0
        for name in dir(cls):
            if name.startswith("_"):
                continue
            raw = inspect.getattr_static(cls, name)
            if isinstance(raw, property):
                f = raw.fget
            elif isinstance(raw, staticmethod):
                f = raw.__func__
                if getattr(hotpath, name, None) is f:  # post_record_bytes, taa_record_bytes, debug_print_buffer_bytes: module functions
                    assert name in ("post_record_bytes", "taa_record_bytes", "debug_print_buffer_bytes")
                    continue
            else:
                f = raw
            assert inspect.isfunction(f), (cls.__name__, name)
            assert f.__qualname__.split(".")[0] in classes and f.__qualname__.split(".")[-1] == name, (cls.__name__, name, f.__qualname__)
            assert f.__module__.startswith(hotpath.__name__ + "."), (cls.__name__, name, f.__module__)
            seen += 1
        assert seen >= 25, (cls.__name__, seen)
