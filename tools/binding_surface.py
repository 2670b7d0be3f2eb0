#!/usr/bin/env python
"""The public surface of unclerenderer_amd.hotpath as text: one sorted line per public item, `name kind signature docstring-hash`.

An item is a module attribute not starting with "_" that is a function or a class (imported modules are skipped), or an attribute of
such a class that does not start with "__". A callable's line carries str(inspect.signature(...)) and the first 12 hex digits of the
SHA-1 of inspect.getdoc(...), "-" without a docstring. tests/golden/binding_surface.txt is this tool's output on the commit before
hotpath became a package; tests/test_binding_surface.py holds the package to it.

    python tools/binding_surface.py > tests/golden/binding_surface.txt     (only when the surface is meant to change)
"""
from __future__ import annotations

import hashlib
import inspect
import pathlib
import sys


def _callable_part(obj) -> str:
    try:
        sig = str(inspect.signature(obj))
    except (TypeError, ValueError):
        sig = "(?)"
    doc = inspect.getdoc(obj)
    return f"{sig} {hashlib.sha1(doc.encode()).hexdigest()[:12] if doc else '-'}"


def _member_line(cls, name: str) -> str:
    raw = inspect.getattr_static(cls, name)
    if isinstance(raw, staticmethod):
        return f"{cls.__name__}.{name} staticmethod {_callable_part(raw.__func__)}"
    if isinstance(raw, classmethod):
        return f"{cls.__name__}.{name} classmethod {_callable_part(raw.__func__)}"
    if isinstance(raw, property):
        return f"{cls.__name__}.{name} property"
    if inspect.isfunction(raw):
        return f"{cls.__name__}.{name} method {_callable_part(raw)}"
    return f"{cls.__name__}.{name} attribute"


def surface(module) -> str:
    lines = []
    for name, obj in vars(module).items():
        if name.startswith("_") or not (inspect.isfunction(obj) or inspect.isclass(obj)):
            continue
        if inspect.isclass(obj):
            lines.append(f"{name} class {_callable_part(obj)}")
            lines += [_member_line(obj, m) for m in dir(obj) if not m.startswith("__")]
        else:
            lines.append(f"{name} function {_callable_part(obj)}")
    return "\n".join(sorted(lines)) + "\n"


if __name__ == "__main__":
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
    from unclerenderer_amd import hotpath
    sys.stdout.write(surface(hotpath))
