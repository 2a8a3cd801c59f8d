"""The resident generic assembler is there on every layer (no compute, CPU box): the five symbols in the built library, their signatures in femus_amd/_lib.py,
the class in femus_amd/capi.py, the declarations in include/femus_hip.h."""
import ctypes
import os

import femus_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["fh_generic_assembler_create", "fh_generic_assembler_set_coords", "fh_generic_assembler_assemble", "fh_generic_assembler_info",
           "fh_generic_assembler_destroy"]


def test_the_generic_assembler_is_exported_declared_and_wrapped():
    L = femus_amd.load_library()      # orders the HIP runtimes (torch first) before the raw handle below
    raw = ctypes.CDLL(femus_amd.library_path())
    header = open(os.path.join(ROOT, "include", "femus_hip.h")).read()
    nargs = {"fh_generic_assembler_create": 12, "fh_generic_assembler_set_coords": 3, "fh_generic_assembler_assemble": 6, "fh_generic_assembler_info": 5,
             "fh_generic_assembler_destroy": 1}
    for name in SYMBOLS:
        assert hasattr(raw, name), "%s is not exported by the built library" % name
        assert ("int %s(" % name) in header
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes is not None and len(f.argtypes) == nargs[name], name
    assert L.fh_generic_assembler_assemble.argtypes[3] is ctypes.c_double          # the scale goes by value as a double
    from femus_amd import capi
    for method in ("set_coords", "assemble", "info", "destroy"):
        assert callable(getattr(capi.GenericAssembler, method))


def test_a_null_object_is_refused_with_a_message():
    L = femus_amd.load_library()
    assert L.fh_generic_assembler_info(None, None, None, None, None) != 0
    assert b"fh_generic_assembler_info" in L.fh_last_error()
    assert L.fh_generic_assembler_destroy(None) == 0
