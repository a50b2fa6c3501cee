"""CPU-side checks of the first-hit queries' C-ABI (no GPU needed): the five entry points are
exported with the signatures include/cpt.h documents, the ctypes prototypes restate them, and a
NULL context is CPT_ERR_INVALID_ARG.
"""
import ctypes
import os
import re

from cpppathtracer_amd import Renderer, _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cpt.h")
INVALID = 1

# name -> the parameter types of the declaration, as the header spells them
DOCUMENTED = {
    "cpt_gbuffer": ["cpt_ctx*", "const cpt_camera*", "uint32_t"],
    "cpt_read_gbuffer": ["cpt_ctx*", "int32_t*", "float*", "float*", "float*", "size_t"],
    "cpt_trace_rays": ["cpt_ctx*", "size_t", "const float*", "const float*", "const float*", "uint32_t", "int32_t*", "float*",
                       "float*"],
    "cpt_pick": ["cpt_ctx*", "const cpt_camera*", "int", "int", "uint32_t", "int32_t*", "float*"],
    "cpt_last_query_ms": ["cpt_ctx*", "float*"],
}
CTYPE_OF = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t}


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", text, re.M)
    assert m, name + " is not declared"
    params = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        params.append(re.sub(r"\s*\w+$", "", p) if not p.endswith("*") else p)   # drop the parameter's name
    return params


def test_declared_as_documented():
    for name, want in DOCUMENTED.items():
        assert _declared(name) == want, name


def test_exported_with_matching_prototypes():
    L = _lib.load()
    for name, params in DOCUMENTED.items():
        assert hasattr(L, name), name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int, name
        assert args == [CTYPE_OF.get(p, ctypes.c_void_p) for p in params], name
    assert L.cpt_abi_version() == 1


def test_null_context_is_invalid_arg():
    L = _lib.load()
    one = (ctypes.c_float * 3)(0, 0, 1)
    i = ctypes.c_int32(0)
    f = ctypes.c_float(0)
    cam = (ctypes.c_uint8 * 136)()
    assert L.cpt_gbuffer(None, cam, 0) == INVALID
    assert L.cpt_read_gbuffer(None, None, None, None, None, 0) == INVALID
    assert L.cpt_trace_rays(None, 1, one, one, None, 0, ctypes.byref(i), ctypes.byref(f), one) == INVALID
    assert L.cpt_pick(None, cam, 0, 0, 0, ctypes.byref(i), ctypes.byref(f)) == INVALID
    assert L.cpt_last_query_ms(None, ctypes.byref(f)) == INVALID
    assert i.value == 0 and f.value == 0.0


def test_renderer_has_the_query_methods():
    for name in ("gbuffer", "read_gbuffer", "trace_rays", "pick", "last_query_ms"):
        assert callable(getattr(Renderer, name)), name
