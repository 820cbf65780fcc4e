"""The Python binding keeps its surface: every name, signature and docstring recorded in tests/golden/binding_surface.json (written by
tests/golden/make_binding_surface.py) is still there, whichever module of the package now defines it. New names are allowed."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_binding_surface  # noqa: E402

RECORDED = json.load(open(os.path.join(ROOT, "tests", "golden", "binding_surface.json")))


def test_every_recorded_name_is_present(rt):
    assert len(RECORDED["attributes"]) > 100 and len(RECORDED["callables"]) > 90
    missing = [n for n in RECORDED["attributes"] if not hasattr(rt, n)]
    assert not missing, missing
    assert [n for n in RECORDED["all"] if n not in rt.__all__] == []
    assert [n for n in rt.__all__ if not hasattr(rt, n)] == []
    for private in ("_check", "_as_desc", "_camera_from_c", "_ctypes_abi"):
        assert hasattr(rt, private)


def test_every_recorded_signature_and_docstring_is_kept(rt):
    now = make_binding_surface.surface()["callables"]
    for name, was in RECORDED["callables"].items():
        assert name in now, f"{name} is no longer a callable of the package"
        assert now[name]["signature"] == was["signature"], f"{name}{now[name]['signature']} was {name}{was['signature']}"
        assert now[name]["doc"] or not was["doc"], f"{name} has lost its docstring"


def test_importing_the_package_does_not_import_torch():
    """In a child process: conftest.py may have imported torch into this one. The child loads no library and opens no GPU."""
    code = f"import importlib, sys; sys.path.insert(0, {ROOT!r}); importlib.import_module({make_binding_surface.PKG!r}); assert 'torch' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", code])
