"""ctypes binding of tests/libjy_primcheck.so (tests/prims_check.hip): the
test-only entry points over the engine's scan, select and sort primitives.
Shared by test_prims_build.py (no GPU) and test_prims_gpu.py."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "libjy_primcheck.so")

P, U64, U32, I32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32

# name -> (restype, argtypes); the first argument of every GPU call is the jy_engine*
SIGNATURES = {
    "jyt_scan_u64": (I32, [P, I32, I32, U64, P, P]),
    "jyt_scan_u32": (I32, [P, I32, I32, U64, P, P]),
    "jyt_scan_colmajor": (I32, [P, U64, U64, P]),
    "jyt_select_flags": (I32, [P, U64, P, P, P]),
    "jyt_sort_bits": (I32, [P, U64, P, P, P, U32, U32, C.POINTER(I32)]),
    "jyt_sort_hist_words": (U64, [U64]),
    "jyt_sort_bits_for": (U32, [U64]),
    "jyt_last_le": (I32, [P, U64, P, U64, P, P]),
    "jyt_block_excl": (I32, [P, U32, U32, P, P, P]),
    "jyt_lookback_scan": (I32, [P, U64, P, P]),
    "jyt_drounds": (I32, [P, U64, P, P, P, U32, U32, U32, P, P, P, P, P]),
    "jyt_dscan_epoch_set": (None, [P, U32]),
    "jyt_dscan_epoch_get": (U32, [P]),
}


def build():
    """the library file, built if it is not there yet"""
    if not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "jylis_amd"), "primcheck"], check=True)
    return LIB_PATH


def load():
    """the engine library first, by the package's own loader (one HIP runtime
    shared with torch; this library's imports resolve to that copy), then this one, typed"""
    from jylis_amd import _lib
    _lib.load()
    lib = C.CDLL(build())
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib
