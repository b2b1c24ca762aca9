"""ctypes bindings of the grouping sort's C++ entry points in libgpuwin.so
(flink_amd/csrc/gw_sort.h; namespace gw, so the names are the Itanium-mangled ones).  They are
not part of the C ABI of include/gpuwin.h: the tests call them to judge the sort by itself."""
import ctypes
from types import SimpleNamespace

from flink_amd import _native as N

_p, _i, _l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
_alt = ctypes.POINTER(ctypes.c_int)

SORT_PAIRS_U32 = "_ZN2gw14sort_pairs_u32EPjS0_S0_S0_liiPvP12ihipStream_tPib"
SORT_PAIRS_U64 = "_ZN2gw14sort_pairs_u64EPmPjS0_S1_liiPvP12ihipStream_tPib"
# hipError_t f(k0, v0, k1, v1, n, lo, hi, scratch, stream, int* result_in_alt, bool iota)
_SORT_PAIRS = (_i, [_p, _p, _p, _p, _l, _i, _i, _p, _p, _alt, ctypes.c_bool])
_SYMBOLS = {
    "sort_pairs_u32": (SORT_PAIRS_U32, *_SORT_PAIRS),
    "sort_pairs_u64": (SORT_PAIRS_U64, *_SORT_PAIRS),
    # hipError_t f(k0, v0, k1, v1, n, bits, scratch, stream, int* result_in_alt)
    "radix_sort_pairs": ("_ZN2gw16radix_sort_pairsEPmPjS0_S1_liPvP12ihipStream_tPi",
                         _i, [_p, _p, _p, _p, _l, _i, _p, _p, _alt]),
    "sort_scratch_bytes": ("_ZN2gw18sort_scratch_bytesEl", _l, [_l]),
    "radix_sort_scratch_bytes": ("_ZN2gw24radix_sort_scratch_bytesEl", _l, [_l]),
    # hipError_t f(uint32_t* v, n, stream)
    "launch_iota": ("_ZN2gw11launch_iotaEPjlP12ihipStream_t", _i, [_p, _l, _p]),
}


def sort_entry_points():
    """Namespace of the six functions, restype / argtypes set."""
    L = N.lib()
    ns = SimpleNamespace()
    for name, (sym, restype, argtypes) in _SYMBOLS.items():
        f = getattr(L, sym)
        f.restype, f.argtypes = restype, argtypes
        setattr(ns, name, f)
    return ns
