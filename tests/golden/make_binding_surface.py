#!/usr/bin/env python3
"""The Python binding's surface as data: tests/golden/binding_surface.json, which tests/test_binding_surface.py holds the package to.

Recorded from the imported package (the library is not loaded): the sorted attribute names (dir, without __dunder__ names), `__all__`, and for every public
callable that the package defines (module-level, and the public methods and `__init__` of DeviceScene, Accumulator, LoadedScene and
Sensor) its str(inspect.signature(...)) and whether it has a docstring. Callables without a Python signature (the ctypes records) are
not recorded. Regenerate only when the surface is meant to change:   python tests/golden/make_binding_surface.py
"""
import importlib
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = "raytracing-course-hw-public_amd"
CLASSES = ("DeviceScene", "Accumulator", "LoadedScene", "Sensor")


def describe(obj):
    """{"signature", "doc"} of a callable the package defines, None for anything else."""
    if not callable(obj) or not (getattr(obj, "__module__", None) or "").startswith(PKG):
        return None
    try:
        return {"signature": str(inspect.signature(obj)), "doc": bool((obj.__doc__ or "").strip())}
    except (TypeError, ValueError):
        return None


def surface():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    callables = {}
    for name in dir(pkg):
        if not name.startswith("_"):
            d = describe(getattr(pkg, name))
            if d is not None:
                callables[name] = d
    for cls in CLASSES:
        for name in dir(getattr(pkg, cls)):
            if name == "__init__" or not name.startswith("_"):
                d = describe(getattr(getattr(pkg, cls), name))
                if d is not None:
                    callables[f"{cls}.{name}"] = d
    names = sorted(n for n in dir(pkg) if not (n.startswith("__") and n.endswith("__")))  # not the import system's own attributes
    return {"attributes": names, "all": list(pkg.__all__), "callables": callables}


def main():
    out = os.path.join(HERE, "binding_surface.json")
    with open(out, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    s = surface()
    print(len(s["attributes"]), "attributes,", len(s["callables"]), "callables ->", os.path.relpath(out, ROOT))


if __name__ == "__main__":
    main()
