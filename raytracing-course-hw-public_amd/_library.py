"""Loading csrc/librt_amd.so and turning its status codes into exceptions. There is NO CPU fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._ctypes_abi import ABI_PROTOTYPES, ERROR_NAMES, HOST_PROTOTYPES, RT_OK, bind

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT_AMD_LIB") or os.path.join(_HERE, "csrc", "librt_amd.so")  # RT_AMD_LIB: tuning variants only
_lib: Optional[C.CDLL] = None


class RtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERROR_NAMES.get(code, code)}: {msg}")
        self.code = code


def lib() -> C.CDLL:
    """Load csrc/librt_amd.so. Raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: the HIP library is not built; there is no CPU fallback. Run __graft_entry__.build().")
        _lib = C.CDLL(LIB_PATH)
        bind(_lib, ABI_PROTOTYPES)
        bind(_lib, HOST_PROTOTYPES)
    return _lib


def _check(code: int) -> None:
    if code != RT_OK:
        raise RtError(code, lib().rt_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    return int(lib().rt_device_count())
