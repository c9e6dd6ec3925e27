"""CPU-side checks of vt_gemm_form (include/vittrack.h): which GEMM kinds of a ViT-Base / ViT-Large forward run on the narrow 128 x 64
tile.  No compute call is made here: the symbol is declared, bound and exported by both libraries, and a null model is refused."""
import ctypes
import os
import re

from conftest import REPO


def _libs():
    from vittracker_amd import native
    if not (os.path.exists(native.LIB_PATH) and os.path.exists(native.LIB_PATH_F16)):
        import __graft_entry__ as ge
        ge.build()
    return native.LIB_PATH, native.LIB_PATH_F16


def test_gemm_form_is_declared_bound_and_exported_by_both_libraries():
    from vittracker_amd import native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vittrack.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+vt_gemm_form\s*\(\s*const\s+vt_model\s*\*\s*m\s*,\s*int32_t\s+B\s*\)\s*;", src)
    assert "vt_gemm_form" in native.SYMBOLS
    restype, argtypes = native.ABI["vt_gemm_form"]
    assert restype is ctypes.c_int and list(argtypes) == [ctypes.c_void_p, ctypes.c_int32]
    assert callable(native.Model.gemm_form)
    for path in _libs():
        assert hasattr(ctypes.CDLL(path), "vt_gemm_form"), path


def test_the_bits_of_the_header_and_the_binding_agree():
    from vittracker_amd import native
    src = open(os.path.join(REPO, "include", "vittrack.h")).read()
    bits = {k: int(v) for k, v in re.findall(r"#define\s+VT_GEMM_([A-Z0-9]+)\s+(\d+)", src)}
    assert bits == {"PATCH": native.GEMM_PATCH, "QK": native.GEMM_QK, "PROJ": native.GEMM_PROJ, "FC1": native.GEMM_FC1, "FC2": native.GEMM_FC2,
                    "HEAD": native.GEMM_HEAD}
    assert sorted(bits.values()) == [1, 2, 4, 8, 16, 32]


def test_null_model_is_refused():
    for path in _libs():
        L = ctypes.CDLL(path)
        L.vt_gemm_form.restype = ctypes.c_int
        L.vt_gemm_form.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        L.vt_last_error.restype = ctypes.c_char_p
        assert L.vt_gemm_form(None, 1) == -1
        assert b"null model" in L.vt_last_error()
