"""ctypes bindings of the network-buffer decoder's C++ entry points in libgpuwin.so
(flink_amd/csrc/gw_netbuf.h; namespace gw, so the names are the Itanium-mangled ones; the
const NbLayout& parameter is a pointer at the ABI level).  They are not part of the C ABI of
include/gpuwin.h: the tests call them to judge the decoder by itself, on buffers the test owns
(gw_decode_serialized allocates its own scratch and shows neither the scratch nor the counters)."""
import ctypes
from types import SimpleNamespace

import numpy as np

from flink_amd import _native as N

_p, _i, _l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64

LAUNCH_NB_DECODE = "_ZN2gw16launch_nb_decodeEPKhlRKNS_8NbLayoutEPlS5_S5_lS5_S5_lPvPNS_8NbStatusEP12ihipStream_t"
NB_SCRATCH_BYTES = "_ZN2gw16nb_scratch_bytesEl"

WIDTH = {"J": 8, "D": 8, "I": 4, "F": 4, "S": 2, "B": 1, "Z": 1}


class NbLayout(ctypes.Structure):
    _fields_ = [("vbytes", ctypes.c_int32), ("key_off", ctypes.c_int32), ("val_off", ctypes.c_int32),
                ("val_type", ctypes.c_int32)]


class NbStatus(ctypes.Structure):
    _fields_ = [("corrupt", ctypes.c_uint64), ("unsupported", ctypes.c_uint64), ("full", ctypes.c_uint64),
                ("skipped", ctypes.c_uint64), ("consumed", ctypes.c_int64), ("records", ctypes.c_int64),
                ("watermarks", ctypes.c_int64), ("walkback", ctypes.c_uint64), ("fallback", ctypes.c_uint64)]


STATUS_FIELDS = [f[0] for f in NbStatus._fields_]


def nb_entry_points():
    """Namespace of the two functions, restype / argtypes set."""
    L = N.lib()
    ns = SimpleNamespace()
    # hipError_t f(buf, nbytes, const NbLayout*, key, ts, val, rec_cap, wm_pos, wm_val, wm_cap, scratch, NbStatus*, stream)
    f = getattr(L, LAUNCH_NB_DECODE)
    f.restype, f.argtypes = _i, [_p, _l, ctypes.POINTER(NbLayout), _p, _p, _p, _l, _p, _p, _l, _p, _p, _p]
    ns.launch_nb_decode = f
    g = getattr(L, NB_SCRATCH_BYTES)
    g.restype, g.argtypes = _l, [_l]
    ns.nb_scratch_bytes = g
    return ns


def nb_layout(types, kf, vf):
    offs = np.cumsum([0] + [WIDTH[t] for t in types]).tolist()
    return NbLayout(offs[-1], offs[kf], offs[vf] if vf >= 0 else 0, ord(types[vf]) if vf >= 0 else 0)


def status_code(st):
    """gw_runtime.cpp nb_status_code: the C ABI's return code of a decode with this status.  Of
    corrupt and unsupported the larger rank is the earlier error (gw_netbuf.h nb_corrupt_first)."""
    if st.corrupt and st.corrupt >= st.unsupported:
        return -1  # GW_E_INVALID
    if st.unsupported:
        return -2  # GW_E_UNSUPPORTED
    return -5 if st.full else 0  # GW_E_OUTPUT_FULL


GUARD_ROWS = 64
PATTERN = 0x5AA55AA55AA55AA5  # what every output row holds before a launch
SCRATCH_POISON = 0xFF         # hipMalloc memory is not zeroed: the scratch starts as all ones
SCRATCH_GUARD = 0xA5
SCRATCH_GUARD_BYTES = 4096


class NbDecoder:
    """Device buffers of one size, reused over many launches: the bytes (0xFF past the uploaded
    stream), the three columns and the two watermark arrays in one int64 tensor, each with
    GUARD_ROWS rows past its capacity, the NbStatus behind them, and the scratch.  Before every
    launch all rows are set to PATTERN, the nb_scratch_bytes(n) bytes of scratch to 0xFF and the
    bytes behind them to a guard value."""

    def __init__(self, max_bytes, rec_rows, wm_rows):
        import torch
        self.torch = torch
        self.E = nb_entry_points()
        self.max_bytes, self.rec_rows, self.wm_rows = max_bytes, rec_rows, wm_rows
        self.bytes = torch.full((max_bytes + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
        self.R, self.W = rec_rows + GUARD_ROWS, wm_rows + GUARD_ROWS
        self.out = torch.empty(3 * self.R + 2 * self.W + len(STATUS_FIELDS), dtype=torch.int64, device="cuda")
        self.scratch = torch.empty(self.E.nb_scratch_bytes(max_bytes) + SCRATCH_GUARD_BYTES, dtype=torch.uint8,
                                   device="cuda")
        assert self.bytes.data_ptr() % 4 == 0 and self.out.data_ptr() % 8 == 0 and self.scratch.data_ptr() % 8 == 0

    def upload(self, data):
        torch = self.torch
        assert len(data) <= self.max_bytes
        self.bytes.fill_(0xFF)
        if data:
            self.bytes[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        self.nbytes = len(data)

    def poison_from(self, n):
        """Every byte from n on reads 0xFF from now on."""
        self.bytes[n:].fill_(0xFF)

    def decode(self, n, types, kf, vf, rec_cap=None, wm_cap=None):
        """One launch over the first n uploaded bytes -> namespace(status, code, key, ts, val,
        wm_pos, wm_val (whole regions, guard rows included), rec_cap, wm_cap, scratch_ok)."""
        rec_cap = self.rec_rows if rec_cap is None else rec_cap
        wm_cap = self.wm_rows if wm_cap is None else wm_cap
        assert 0 <= n <= self.max_bytes and rec_cap <= self.rec_rows and wm_cap <= self.wm_rows
        R, W = self.R, self.W
        at = [0, R, 2 * R, 3 * R, 3 * R + W, 3 * R + 2 * W]
        ptr = [ctypes.c_void_p(self.out.data_ptr() + 8 * a) for a in at]
        used = self.E.nb_scratch_bytes(n)
        self.out.fill_(PATTERN)
        self.scratch.fill_(SCRATCH_GUARD)
        self.scratch[:used].fill_(SCRATCH_POISON)
        lay = nb_layout(types, kf, vf)
        err = self.E.launch_nb_decode(ctypes.c_void_p(self.bytes.data_ptr()), n, ctypes.byref(lay), ptr[0], ptr[1],
                                      ptr[2], rec_cap, ptr[3], ptr[4], wm_cap,
                                      ctypes.c_void_p(self.scratch.data_ptr()), ptr[5], None)
        assert err == 0, f"launch_nb_decode: hipError {err}"
        h = self.out.cpu().numpy()
        scratch_ok = bool((self.scratch[used:] == SCRATCH_GUARD).all().item())
        st = NbStatus.from_buffer_copy(h[at[5]:].tobytes())
        return SimpleNamespace(status=st, code=status_code(st), key=h[at[0]:at[1]], ts=h[at[1]:at[2]],
                               val=h[at[2]:at[3]], wm_pos=h[at[3]:at[4]], wm_val=h[at[4]:at[5]], rec_cap=rec_cap,
                               wm_cap=wm_cap, scratch_ok=scratch_ok, raw=h)
