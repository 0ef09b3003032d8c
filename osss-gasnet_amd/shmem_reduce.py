"""ctypes binding of libshmem_reduce.so for tests and bench.py.

The product is the C library (include/shmem.h, shmemx.h, mi355_reduce.h);
this module only loads it and marshals numpy arrays and pointers, the way an
OpenSHMEM test program in C would call it. It never computes a reduction
itself: if the library is missing, loading fails loudly.
"""
import ctypes
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SHMEM_REDUCE_LIBDIR: a variant build of the same library (e.g. lib/probe,
# csrc/Makefile `probe`) for measurement tools; default: the in-tree lib/
LIB_DIR = os.environ.get("SHMEM_REDUCE_LIBDIR") or os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libshmem_reduce.so")

OPS = ["sum", "prod", "and", "or", "xor", "min", "max"]           # enum mi355_op
DTYPES = ["short", "int", "long", "longlong", "float", "double",   # enum mi355_dtype
          "longdouble", "complexf", "complexd", "half", "bfloat16"]
NP = {
    "short": np.int16, "int": np.int32, "long": np.int64, "longlong": np.int64,
    "float": np.float32, "double": np.float64, "longdouble": np.longdouble,
    "complexf": np.complex64, "complexd": np.complex128,
    "half": np.float16, "bfloat16": np.uint16,   # numpy has no bfloat16: its bit patterns
}
# the 16-bit float types are not in the reference: their entry points are shmemx_<T>_<op>_to_all
SHMEMX_DTYPES = ("half", "bfloat16")
# torch dtype name -> the shmem type whose C type has its layout (LP64: long = long long = int64)
TORCH_DTYPES = {"int16": "short", "int32": "int", "int64": "long", "float32": "float", "float64": "double",
                "complex64": "complexf", "complex128": "complexd", "float16": "half", "bfloat16": "bfloat16"}
ALGORITHMS = {"auto": 0, "p2p": 1, "exact": 2, "rccl": 3}          # enum shmemx_reduce_algorithm
ORDERS = {"reference": 0, "pe_start": 1}                            # enum shmemx_reduce_order
SHMEM_REDUCE_SYNC_SIZE = 128
SHMEM_REDUCE_MIN_WRKDATA_SIZE = 64
SHMEM_SYNC_VALUE = -1

_vp = ctypes.c_void_p
_sz = ctypes.c_size_t
_i = ctypes.c_int
_pd = ctypes.c_ssize_t  # ptrdiff_t


def bf16_from_f32(array):
    """float32 values -> bfloat16 bit patterns (uint16): round to nearest,
    ties to even, subnormals kept, overflow to +-inf; a NaN becomes the
    canonical quiet NaN 0x7FC0 (the library's sum/prod step, shmemx.h)."""
    a = np.ascontiguousarray(array, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    bits = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(a), np.uint16(0x7FC0), bits)


def bf16_to_f32(bits):
    """bfloat16 bit patterns (uint16) -> the float32 values they denote (exact)"""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    return (b.astype(np.uint32) << 16).view(np.float32)


class CallInfo(ctypes.Structure):
    """shmemx_call_info (include/shmemx.h): what the last *_to_all call ran"""
    _fields_ = [("schedule", ctypes.c_char * 64), ("kernel", ctypes.c_char * 256), ("ordered", _i),
                ("sources", _i), ("outputs", _i), ("peer_sources", _i), ("launches", _i),
                ("bytes_per_buffer", ctypes.c_ulonglong), ("alg_bytes", ctypes.c_ulonglong),
                ("peer_bytes", ctypes.c_ulonglong)]


def load(path=LIB_PATH):
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    sig = {
        "shmem_init": ([], None), "shmem_finalize": ([], None),
        "shmem_my_pe": ([], _i), "shmem_n_pes": ([], _i),
        "shmem_malloc": ([_sz], _vp), "shmem_free": ([_vp], None),
        "shmem_barrier_all": ([], None),
        "shmem_barrier": ([_i, _i, _i, _vp], None),
        "shmem_global_exit": ([_i], None),
        "shmemx_barrier_on_stream": ([_i, _i, _i, _vp], None),
        "shmemx_malloc_device": ([_sz], _vp), "shmemx_free_device": ([_vp], None),
        "shmemx_is_device_symmetric": ([_vp], _i), "shmemx_peer_device_ptr": ([_vp, _i], _vp),
        "shmemx_set_reduce_algorithm": ([_i], _i), "shmemx_get_reduce_algorithm": ([], _i),
        "shmemx_set_reduce_order": ([_i], _i), "shmemx_get_reduce_order": ([], _i),
        "shmemx_set_persistent": ([_i], _i),
        "shmemx_persistent_stats": ([ctypes.POINTER(ctypes.c_long)] * 2, None),
        "shmemx_external_map_stats": ([ctypes.POINTER(ctypes.c_long)] * 3, None),
        "shmemx_external_map_flush": ([], None),
        "shmemx_device_id": ([], _i), "shmemx_device_synchronize": ([], None),
        "shmemx_threshold_calibration": ([ctypes.POINTER(ctypes.c_double), _i], _i),
        "shmemx_peer_link": ([_i, ctypes.POINTER(_i), ctypes.POINTER(_i)], _i),
        "shmemx_memcpy": ([_vp, _vp, _sz], None), "shmemx_wtime": ([], ctypes.c_double),
        "shmemx_kernel_timing": ([_i], None),
        "shmemx_rccl_init": ([ctypes.c_double], _i),
        "shmemx_last_call_info": ([ctypes.POINTER(CallInfo)], _i),
        "shmemx_coherence_selftest": ([ctypes.POINTER(_i)] * 3, None),
        "shmemx_coherence_sysload": ([ctypes.POINTER(_i)] * 2, None),
        "shmemx_kernel_timing_stats": ([ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_double)], None),
        "shmemx_kernel_timing_phase_stats": ([_i, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(ctypes.c_double)], None),
        "mi355_dtype_size": ([_i], _sz), "mi355_op_supported": ([_i, _i], _i),
        "mi355_combine": ([_i, _i, _vp, ctypes.POINTER(_vp), _i, _sz, _vp], _i),
        "mi355_combine_orders": ([_i, _i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i, _sz, _vp], _i),
        "mi355_combine_prefix": ([_i, _i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i, _sz, _vp], _i),
        "mi355_copy_segments": ([ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_sz), _i, _vp], _i),
        "mi355_copy_direction_next_launch": ([_i], None),
        "mi355_device_cus": ([], _i),
        "mi355_last_launch_grid": ([ctypes.POINTER(ctypes.c_uint)] * 2, None),
        "mi355_nan_patch_copy": ([_i, _vp, _vp, _vp, _sz, _vp, _vp], _i),
        "mi355_shard_bounds": ([_sz, _sz, _i, _i, ctypes.POINTER(_sz), ctypes.POINTER(_sz)], None),
    }
    for name, (args, res) in sig.items():
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = res
    return lib


class Shmem:
    """One PE's view of the library (call init() once per process)."""

    def __init__(self, path=LIB_PATH):
        self.lib = load(path)
        self._psync = np.full(SHMEM_REDUCE_SYNC_SIZE, SHMEM_SYNC_VALUE, dtype=np.int64)
        self._psync_ptr = self._psync.ctypes.data
        self._fns = {}

    def _reduction(self, op, dtype):
        f = self._fns.get((op, dtype))
        if f is None:
            prefix = "shmemx" if dtype in SHMEMX_DTYPES else "shmem"
            f = getattr(self.lib, f"{prefix}_{dtype}_{op}_to_all")
            f.restype = None
            f.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp, _vp]
            self._fns[(op, dtype)] = f
        return f

    # ---- runtime
    def init(self):
        self.lib.shmem_init()

    def finalize(self):
        self.lib.shmem_finalize()

    def my_pe(self):
        return self.lib.shmem_my_pe()

    def n_pes(self):
        return self.lib.shmem_n_pes()

    def barrier_all(self):
        self.lib.shmem_barrier_all()

    def malloc_device(self, nbytes):
        return self.lib.shmemx_malloc_device(nbytes)

    def free_device(self, ptr):
        self.lib.shmemx_free_device(ptr)

    def threshold_calibration(self):
        """None, or the init-time threshold calibration (shmemx_threshold_calibration):
        {"fused": [(bytes, fused_us, multi_launch_us)...], "oneshot": [(bytes, oneshot_us, twoshot_us)...]}"""
        us = (ctypes.c_double * 22)()
        if not self.lib.shmemx_threshold_calibration(us, 22):
            return None
        fs = [64 << 10, 256 << 10, 512 << 10, 1 << 20, 2 << 20, 4 << 20]
        os_ = [16 << 10, 32 << 10, 64 << 10, 128 << 10, 256 << 10]
        return {"fused": [(b, us[i], us[6 + i]) for i, b in enumerate(fs)],
                "oneshot": [(b, us[12 + i], us[17 + i]) for i, b in enumerate(os_)]}

    def peer_device_ptr(self, ptr, pe):
        """PE pe's copy of a device-heap object, addressable by kernels on
        this PE's GPU (shmemx_peer_device_ptr); None if not mapped."""
        return self.lib.shmemx_peer_device_ptr(ptr, pe)

    def malloc(self, nbytes):
        return self.lib.shmem_malloc(nbytes)

    def free(self, ptr):
        self.lib.shmem_free(ptr)

    def set_algorithm(self, name):
        return self.lib.shmemx_set_reduce_algorithm(ALGORITHMS[name])

    def set_order(self, name):
        """"reference": every PE gets the reference's result for itself; "pe_start": PE_start's everywhere"""
        return self.lib.shmemx_set_reduce_order(ORDERS[name])

    def set_fused_max(self, nbytes):
        """fused-kernel threshold in bytes per PE (collective setting, shmemx.h); returns the previous"""
        f = self.lib.shmemx_set_fused_max_bytes
        f.argtypes, f.restype = [ctypes.c_size_t], ctypes.c_size_t
        return int(f(nbytes))

    def thresholds(self):
        """(fused_max, oneshot_max) in bytes per PE (shmemx.h)"""
        for name in ("shmemx_get_fused_max_bytes", "shmemx_get_oneshot_max_bytes"):
            getattr(self.lib, name).restype = ctypes.c_size_t
        return int(self.lib.shmemx_get_fused_max_bytes()), int(self.lib.shmemx_get_oneshot_max_bytes())

    def set_oneshot_max(self, nbytes):
        """one-shot threshold in bytes per PE (collective setting, shmemx.h); returns the previous"""
        f = self.lib.shmemx_set_oneshot_max_bytes
        f.argtypes, f.restype = [ctypes.c_size_t], ctypes.c_size_t
        return int(f(nbytes))

    def set_persistent(self, enable):
        """opt-in persistent fused server (shmemx.h); returns the previous setting"""
        return bool(self.lib.shmemx_set_persistent(1 if enable else 0))

    def persistent_stats(self):
        """(calls served by a resident server, servers launched) since init"""
        a, b = ctypes.c_long(), ctypes.c_long()
        self.lib.shmemx_persistent_stats(ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def external_map_fallbacks(self):
        """calls staged because a member could not open a peer's buffer (shmemx.h)"""
        self.lib.shmemx_external_map_fallbacks.restype = ctypes.c_long
        return int(self.lib.shmemx_external_map_fallbacks())

    def external_map_stats(self):
        """(peers' allocations mapped now, opened, closed since init): device
        buffers outside the heap that calls mapped (shmemx.h)"""
        a, b, c = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
        self.lib.shmemx_external_map_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return a.value, b.value, c.value

    def sync(self):
        self.lib.shmemx_device_synchronize()

    # ---- data movement (hipMemcpy, blocking)
    def put(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self.lib.shmemx_memcpy(dptr, arr.ctypes.data, arr.nbytes)

    def get(self, dptr, n, dtype):
        out = np.empty(n, dtype=NP[dtype] if isinstance(dtype, str) else dtype)
        self.lib.shmemx_memcpy(out.ctypes.data, dptr, out.nbytes)
        return out

    # ---- the reduction entry points (include/shmem.h)
    def to_all(self, op, dtype, target, source, nreduce, PE_start=0, logPE_stride=0, PE_size=None,
               pWrk=None, pSync=None):
        if PE_size is None:
            PE_size = self.n_pes()
        if pSync is None:
            pSync = self._psync_ptr
        self._reduction(op, dtype)(target, source, nreduce, PE_start, logPE_stride, PE_size, pWrk, pSync)

    def to_all_tensors(self, op, target, source, PE_start=0, logPE_stride=0, PE_size=None):
        """shmem_<T>_<op>_to_all on two contiguous device tensors of one dtype
        (T from the tensor's dtype; long double has no torch dtype;
        torch.float16 and torch.bfloat16 take shmemx_half_* / shmemx_bfloat16_*:
        sum, prod, min, max, every step rounded to the type). They need
        not come from the symmetric heap: at PE_size > 1 the members map each
        other's allocations for the call (shmemx.h, extmap.c). Blocking, like
        the C call: on return `target` holds this PE's result."""
        if target.dtype != source.dtype or target.numel() != source.numel():
            raise ValueError("target and source must have the same dtype and number of elements")
        if not (target.is_contiguous() and source.is_contiguous()) or target.device.type != "cuda" \
                or source.device.type != "cuda":
            raise ValueError("target and source must be contiguous GPU tensors")
        dtype = TORCH_DTYPES.get(str(source.dtype).replace("torch.", ""))
        if dtype is None:
            raise TypeError(f"no shmem_*_to_all for {source.dtype}")
        self.to_all(op, dtype, target.data_ptr(), source.data_ptr(), source.numel(), PE_start, logPE_stride, PE_size)

    # ---- scan: inclusive / exclusive prefix reductions (include/shmemx.h)
    def _scan_fn(self, op, dtype, exclusive):
        key = ("scan", op, dtype, bool(exclusive))
        f = self._fns.get(key)
        if f is None:
            f = getattr(self.lib, f"shmemx_{dtype}_{op}_{'exscan' if exclusive else 'inscan'}")
            f.restype = None
            f.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp, _vp]
            self._fns[key] = f
        return f

    def scan(self, op, dtype, target, source, nreduce, PE_start=0, logPE_stride=0, PE_size=None, exclusive=False,
             pWrk=None, pSync=None):
        """shmemx_<T>_<op>_inscan (exclusive: _exscan): member j of the active
        set receives src_0 op ... op src_j (exclusive: ... op src_(j-1), and
        member 0's target is left untouched). Blocking."""
        if PE_size is None:
            PE_size = self.n_pes()
        if pSync is None:
            pSync = self._psync_ptr
        self._scan_fn(op, dtype, exclusive)(target, source, nreduce, PE_start, logPE_stride, PE_size, pWrk, pSync)

    def scan_tensors(self, op, out, x, PE_start=0, logPE_stride=0, PE_size=None, exclusive=False):
        """scan() on two contiguous tensors of one dtype from heap_tensor (the
        scan collectives take device buffers of the symmetric heap only); every
        torch dtype to_all_tensors maps, float16 and bfloat16 included."""
        if out.dtype != x.dtype or out.numel() != x.numel():
            raise ValueError("out and x must have the same dtype and number of elements")
        if not (out.is_contiguous() and x.is_contiguous()) or out.device.type != "cuda" or x.device.type != "cuda":
            raise ValueError("out and x must be contiguous GPU tensors")
        dtype = TORCH_DTYPES.get(str(x.dtype).replace("torch.", ""))
        if dtype is None:
            raise TypeError(f"no scan for {x.dtype}")
        for t in (out, x):
            if t.numel() and not self.lib.shmemx_is_device_symmetric(t.data_ptr()):
                raise ValueError("scan_tensors takes tensors from heap_tensor (the device symmetric heap)")
        self.scan(op, dtype, out.data_ptr(), x.data_ptr(), x.numel(), PE_start, logPE_stride, PE_size, exclusive)

    # ---- value and location: maxloc / minloc (include/shmemx.h)
    LOC_OPS = ("max", "min")
    LOC_DTYPES = ("short", "int", "long", "longlong", "float", "double", "half", "bfloat16")

    def loc_to_all(self, op, dtype, target, target_loc, source, source_loc, nreduce, PE_start=0, logPE_stride=0,
                   PE_size=None):
        """shmemx_<dtype>_<op>loc_to_all (op "max" or "min"): every member
        receives, per element, the winning value in `target` (its bits
        unchanged) and its location in `target_loc` (int64). source_loc=None
        passes NULL: the location is the member's index in the active set.
        All arrays in the device symmetric heap. Blocking."""
        if op not in self.LOC_OPS or dtype not in self.LOC_DTYPES:
            raise ValueError(f"no {op}loc_to_all for {dtype}")
        if PE_size is None:
            PE_size = self.n_pes()
        f = self._typed_fn(f"shmemx_{dtype}_{op}loc_to_all", None, [_vp, _vp, _vp, _vp, _i, _i, _i, _i])
        f(target, target_loc, source, source_loc, nreduce, PE_start, logPE_stride, PE_size)

    def loc_to_all_tensors(self, op, out, out_idx, x, idx=None, PE_start=0, logPE_stride=0, PE_size=None):
        """loc_to_all() on contiguous tensors from heap_tensor: `out` and `x`
        of one dtype (int16/32/64, float32/64, float16, bfloat16), `out_idx`
        and `idx` int64, all of one size; idx=None: the member index.
        out is x together with out_idx is idx: in place."""
        import torch
        dtype = TORCH_DTYPES.get(str(x.dtype).replace("torch.", ""))
        if dtype not in self.LOC_DTYPES:
            raise TypeError(f"no {op}loc_to_all for {x.dtype}")
        tensors = [out, out_idx, x] + ([idx] if idx is not None else [])
        if out.dtype != x.dtype or any(t.dtype != torch.int64 for t in tensors[1::2]):
            raise TypeError("out and x must have one dtype, out_idx and idx must be int64")
        if any(t.numel() != x.numel() or not t.is_contiguous() or t.device.type != "cuda" for t in tensors):
            raise ValueError("the tensors must be contiguous GPU tensors of one size")
        for t in tensors:
            if t.numel() and not self.lib.shmemx_is_device_symmetric(t.data_ptr()):
                raise ValueError("loc_to_all_tensors takes tensors from heap_tensor (the device symmetric heap)")
        self.loc_to_all(op, dtype, out.data_ptr(), out_idx.data_ptr(), x.data_ptr(),
                        idx.data_ptr() if idx is not None else None, x.numel(), PE_start, logPE_stride, PE_size)

    def combine_loc(self, op, dtype, dst_val, dst_loc, src_vals, src_locs, loc_base, n, stream=None):
        """mi355_combine_loc: the value-and-location fold of len(src_vals)
        sources. src_locs: None (all implicit), or a list whose entries may be
        None (source j's location is then loc_base + j). Returns its status."""
        f = self._typed_fn("mi355_combine_loc", _i, [_i, _i, _vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                                     ctypes.c_long, _i, _sz, _vp])
        sv = (_vp * max(1, len(src_vals)))(*src_vals)
        sl = None if src_locs is None else (_vp * max(1, len(src_locs)))(*[x if x else None for x in src_locs])
        return f(OPS.index(op), DTYPES.index(dtype), dst_val, dst_loc, sv, sl, loc_base, len(src_vals), n, stream)

    # ---- wide sum: half / bfloat16 sums accumulated in binary32 (include/shmemx.h)
    WSUM_DTYPES = ("half", "bfloat16")

    def wsum(self, dtype, out_float, target_ptr, source_ptr, n, PE_start=0, logPE_stride=0, PE_size=None):
        """shmemx_<dtype>_wsum_to_all (out_float: _wsum_to_all_float): the sum
        of the members' 16-bit sources accumulated in binary32 in ascending
        member order and rounded once (or kept as float32); the same bits on
        every member. Both arrays in the device symmetric heap. Blocking."""
        if dtype not in self.WSUM_DTYPES:
            raise ValueError(f"no wsum_to_all for {dtype}")
        if PE_size is None:
            PE_size = self.n_pes()
        f = self._typed_fn(f"shmemx_{dtype}_wsum_to_all{'_float' if out_float else ''}", None,
                           [_vp, _vp, _i, _i, _i, _i])
        f(target_ptr, source_ptr, n, PE_start, logPE_stride, PE_size)

    def wsum_tensors(self, out, x, PE_start=0, logPE_stride=0, PE_size=None):
        """wsum() on contiguous tensors from heap_tensor: `x` float16 or
        bfloat16, `out` of the same dtype (out is x: in place) or float32."""
        import torch
        dtype = TORCH_DTYPES.get(str(x.dtype).replace("torch.", ""))
        if dtype not in self.WSUM_DTYPES:
            raise TypeError(f"no wsum_to_all for {x.dtype}")
        if out.dtype != x.dtype and out.dtype != torch.float32:
            raise TypeError(f"out must be {x.dtype} or torch.float32, not {out.dtype}")
        if any(t.numel() != x.numel() or not t.is_contiguous() or t.device.type != "cuda" for t in (out, x)):
            raise ValueError("out and x must be contiguous GPU tensors of one size")
        for t in (out, x):
            if t.numel() and not self.lib.shmemx_is_device_symmetric(t.data_ptr()):
                raise ValueError("wsum_tensors takes tensors from heap_tensor (the device symmetric heap)")
        o, s, nb = out.data_ptr(), x.data_ptr(), x.numel() * 2
        if o < s + nb and s < o + out.numel() * out.element_size() and (out.dtype != x.dtype or o != s):
            raise ValueError("out overlaps x (only a 16-bit out that is x itself may: in place)")
        self.wsum(dtype, out.dtype != x.dtype, o, s, x.numel(), PE_start, logPE_stride, PE_size)

    def combine_wide(self, dtype, out_dtype, dst, srcs, n, stream=None):
        """mi355_combine_wide: the binary32-accumulated sum of len(srcs) half
        or bfloat16 arrays into dst (out_dtype: the same type, or "float").
        Returns its status."""
        f = self._typed_fn("mi355_combine_wide", _i, [_i, _i, _vp, ctypes.POINTER(_vp), _i, _sz, _vp])
        sv = (_vp * max(1, len(srcs)))(*srcs)
        return f(DTYPES.index(dtype), DTYPES.index(out_dtype), dst, sv, len(srcs), n, stream)

    def combine_wide_plan(self, n, out_dtype, cus):
        """(grid, elements per grid pass) of mi355_combine_wide's 16-byte-aligned launch"""
        f = self._typed_fn("mi355_combine_wide_plan", None,
                           [_sz, _i, _i, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_ulonglong)])
        g, p = ctypes.c_uint(), ctypes.c_ulonglong()
        f(n, DTYPES.index(out_dtype), cus, ctypes.byref(g), ctypes.byref(p))
        return g.value, p.value

    # ---- all-to-all (include/shmem.h)
    def _alltoall_fn(self, bits, strided):
        if bits not in (32, 64):
            raise ValueError("bits must be 32 or 64")
        name = f"shmem_alltoall{'s' if strided else ''}{bits}"
        f = self._fns.get(name)
        if f is None:
            f = getattr(self.lib, name)
            f.restype = None
            f.argtypes = ([_vp, _vp, _pd, _pd, _sz, _i, _i, _i, _vp] if strided
                          else [_vp, _vp, _sz, _i, _i, _i, _vp])
            self._fns[name] = f
        return f

    def alltoall(self, bits, target, source, nelems, PE_start=0, logPE_stride=0, PE_size=None):
        """shmem_alltoall32/64: block m of member i's source becomes block i of
        member m's target (nelems elements of bits/8 bytes per block)"""
        if PE_size is None:
            PE_size = self.n_pes()
        self._alltoall_fn(bits, False)(target, source, nelems, PE_start, logPE_stride, PE_size, self._psync_ptr)

    def alltoalls(self, bits, target, source, dst, sst, nelems, PE_start=0, logPE_stride=0, PE_size=None):
        """shmem_alltoalls32/64: the same with the elements dst apart in the
        target and sst apart in the source (in elements, both >= 1)"""
        if PE_size is None:
            PE_size = self.n_pes()
        self._alltoall_fn(bits, True)(target, source, dst, sst, nelems, PE_start, logPE_stride, PE_size,
                                      self._psync_ptr)

    def alltoall_tensors(self, out, x, PE_start=0, logPE_stride=0, PE_size=None):
        """All-to-all of two contiguous tensors: x (a heap_tensor) is cut into
        PE_size equal blocks, block m goes to member m; out (any device tensor
        of the same total bytes) receives member i's block as its block i.
        Moved as 64-bit elements when a block is a multiple of 8 bytes, as
        32-bit ones when a multiple of 4; any other block size: ValueError.
        Blocking, like the C call."""
        if PE_size is None:
            PE_size = self.n_pes()
        total = x.numel() * x.element_size()
        if out.numel() * out.element_size() != total:
            raise ValueError("out and x must hold the same number of bytes")
        if PE_size < 1 or total % PE_size != 0:
            raise ValueError(f"{total} bytes do not divide into {PE_size} blocks")
        block = total // PE_size
        if block % 8 == 0:
            bits = 64
        elif block % 4 == 0:
            bits = 32
        else:
            raise ValueError(f"the per-peer block of {block} bytes is not a multiple of 4 bytes")
        if not (out.is_contiguous() and x.is_contiguous()) or out.device.type != "cuda" or x.device.type != "cuda":
            raise ValueError("out and x must be contiguous GPU tensors")
        self.alltoall(bits, out.data_ptr(), x.data_ptr(), block // (bits // 8), PE_start, logPE_stride, PE_size)

    def strided_pull(self, elem_size, dsts, srcs, dst_stride, src_stride, nelems, stream=None):
        """mi355_strided_pull: dsts[i][k * dst_stride] = srcs[i][k * src_stride], k < nelems"""
        f = self._fns.get("mi355_strided_pull")
        if f is None:
            f = self.lib.mi355_strided_pull
            f.restype = _i
            f.argtypes = [_i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _pd, _pd, _sz, _i, _vp]
            self._fns["mi355_strided_pull"] = f
        d = (_vp * len(dsts))(*dsts)
        s = (_vp * len(srcs))(*srcs)
        return f(elem_size, d, s, dst_stride, src_stride, nelems, len(dsts), stream)

    def strided_copy(self, elem_size, dsts, srcs, dst_stride, src_stride, nelems, stream=None):
        """mi355_strided_copy: the same for elements of 1, 2, 4, 8 or 16 bytes"""
        f = self._fns.get("mi355_strided_copy")
        if f is None:
            f = self.lib.mi355_strided_copy
            f.restype = _i
            f.argtypes = [_i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _pd, _pd, _sz, _i, _vp]
            self._fns["mi355_strided_copy"] = f
        d = (_vp * len(dsts))(*dsts)
        s = (_vp * len(srcs))(*srcs)
        return f(elem_size, d, s, dst_stride, src_stride, nelems, len(dsts), stream)

    # ---- strided put/get (include/shmem.h)
    _STRIDED_NAMES = {1: "shmem_char_i{}", 2: "shmem_short_i{}", 4: "shmem_i{}32", 8: "shmem_i{}64",
                      16: "shmem_i{}128"}

    def _strided_fn(self, op, elem_size):
        if elem_size not in self._STRIDED_NAMES:
            raise ValueError("elem_size must be 1, 2, 4, 8 or 16")
        name = self._STRIDED_NAMES[elem_size].format(op)
        f = self._fns.get(name)
        if f is None:
            f = getattr(self.lib, name)
            f.restype = None
            f.argtypes = [_vp, _vp, _pd, _pd, _sz, _i]
            self._fns[name] = f
        return f

    def iput(self, elem_size, target, source, tst, sst, nelems, pe):
        """shmem_iput: target_on_pe[k * tst] = source[k * sst] for k < nelems
        (shmem_char_iput, shmem_short_iput, shmem_iput32/64/128 by elem_size);
        target symmetric, strides in elements. Blocking."""
        self._strided_fn("put", elem_size)(target, source, tst, sst, nelems, pe)

    def iget(self, elem_size, target, source, tst, sst, nelems, pe):
        """shmem_iget: target[k * tst] = source_on_pe[k * sst] for k < nelems;
        source symmetric. Blocking."""
        self._strided_fn("get", elem_size)(target, source, tst, sst, nelems, pe)

    # ---- atomics, waits, locks (include/shmem.h; csrc/atomic.c)
    _AMO_C = {"short": ctypes.c_short, "int": ctypes.c_int, "long": ctypes.c_long, "longlong": ctypes.c_longlong,
              "float": ctypes.c_float, "double": ctypes.c_double}
    _AMO_ARGS = {"swap": "v", "cswap": "cv", "fadd": "v", "finc": "", "add": "v", "inc": "", "fetch": "", "set": "v"}
    AMO_OPS = ["swap", "cswap", "fadd", "fetch", "set"]                 # enum mi355_amo_op
    CMP = {"eq": 0, "ne": 1, "gt": 2, "le": 3, "lt": 4, "ge": 5}       # enum shmem_cmp_constants

    def _typed_fn(self, name, restype, argtypes):
        f = self._fns.get(name)
        if f is None:
            f = getattr(self.lib, name)
            f.restype = restype
            f.argtypes = argtypes
            self._fns[name] = f
        return f

    def atomic(self, op, dtype, ptr, pe, value=None, cond=None):
        """shmem_<dtype>_<op> on the symmetric object at ptr on PE pe: op one
        of swap, cswap, fadd, finc, add, inc, fetch, set; dtype int, long,
        longlong (every op) or float, double (swap, fetch, set). Returns the
        old value for the fetching ops, None for add, inc and set."""
        ct = self._AMO_C[dtype]
        fetching = op not in ("add", "inc", "set")
        extra = [ct] * len(self._AMO_ARGS[op])
        f = self._typed_fn(f"shmem_{dtype}_{op}", ct if fetching else None, [_vp] + extra + [_i])
        args = {"": [], "v": [value], "cv": [cond, value]}[self._AMO_ARGS[op]]
        if any(a is None for a in args):
            raise ValueError(f"{op} needs " + ("cond and value" if op == "cswap" else "value"))
        return f(ptr, *args, pe)

    def wait_until(self, dtype, ptr, cmp, value):
        """shmem_<dtype>_wait_until: dtype short, int, long or longlong; cmp one of eq ne gt le lt ge"""
        ct = self._AMO_C[dtype]
        self._typed_fn(f"shmem_{dtype}_wait_until", None, [_vp, _i, ct])(ptr, self.CMP[cmp], value)

    def set_lock(self, lock):
        self._typed_fn("shmem_set_lock", None, [_vp])(lock)

    def clear_lock(self, lock):
        self._typed_fn("shmem_clear_lock", None, [_vp])(lock)

    def test_lock(self, lock):
        """0 when this PE took the lock, non-zero when it is busy; never blocks"""
        return self._typed_fn("shmem_test_lock", _i, [_vp])(lock)

    def quiet(self):
        self._typed_fn("shmem_quiet", None, [])()

    def fence(self):
        self._typed_fn("shmem_fence", None, [])()

    def atomic_add_v(self, dtype, target, source, nelems, pe):
        """shmemx_<dtype>_atomic_add_v: target_on_pe[i] += source[i] atomically
        for i < nelems; dtype int, long, longlong, float or double; target
        symmetric, source any device or host memory. Blocking."""
        self._typed_fn(f"shmemx_{dtype}_atomic_add_v", None, [_vp, _vp, _sz, _i])(target, source, nelems, pe)

    def atomic_add_v_tensors(self, target, source, pe):
        """The same on tensors: `target` a heap_tensor, `source` any contiguous
        torch tensor (GPU or CPU) of the same dtype and size."""
        name = TORCH_DTYPES.get(str(target.dtype).replace("torch.", ""))
        if name not in ("int", "long", "float", "double"):
            raise TypeError(f"no atomic_add_v for {target.dtype}")
        if target.dtype != source.dtype or target.numel() != source.numel() or \
                not (target.is_contiguous() and source.is_contiguous()):
            raise ValueError("target and source must be contiguous tensors of one dtype and size")
        self.atomic_add_v(name, target.data_ptr(), source.data_ptr(), target.numel(), pe)

    def amo_raw(self, op, width, target, value=0, cond=0, slot=None, stream=None):
        """mi355_amo: one atomic of `width` bytes on device-visible memory;
        op one of AMO_OPS; the old value goes to the 8 bytes at `slot`"""
        f = self._typed_fn("mi355_amo", _i, [_i, _i, _vp, ctypes.c_ulonglong, ctypes.c_ulonglong, _vp, _vp])
        return f(self.AMO_OPS.index(op), width, target, value, cond, slot, stream)

    def atomic_add_v_raw(self, dtype, target, source, n, stream=None):
        """mi355_atomic_add_v: target[i] += source[i] atomically, i < n"""
        f = self._typed_fn("mi355_atomic_add_v", _i, [_i, _vp, _vp, _sz, _vp])
        return f(DTYPES.index(dtype), target, source, n, stream)

    def atomic_add_v_plan(self, n, cus):
        """(grid, elements per grid pass) of mi355_atomic_add_v for n elements on `cus` compute units"""
        f = self._typed_fn("mi355_atomic_add_v_plan", None,
                           [_sz, _i, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_ulonglong)])
        g, p = ctypes.c_uint(), ctypes.c_ulonglong()
        f(n, cus, ctypes.byref(g), ctypes.byref(p))
        return g.value, p.value

    def heap_tensor(self, n, dtype):
        """A 1-D torch tensor of n elements of torch dtype `dtype` in the
        device symmetric heap (collective, like shmemx_malloc_device): the
        buffer the stream-ordered, graph-capturable reductions take. The tensor
        does not own the memory: free it with free_device(t.data_ptr()) once
        no tensor or queued work uses it."""
        import torch
        name = TORCH_DTYPES.get(str(dtype).replace("torch.", ""))
        if name is None:
            raise TypeError(f"no shmem_*_to_all for {dtype}")
        # bfloat16 has no array-interface type string: wrapped as 16-bit integers, viewed below
        np_dt = np.dtype(np.int16 if name == "bfloat16" else NP[name])
        ptr = self.malloc_device(max(1, n) * np_dt.itemsize)
        if not ptr:
            raise MemoryError("device symmetric heap exhausted")

        class _HeapBuffer:
            __cuda_array_interface__ = {"shape": (n,), "typestr": np_dt.str, "data": (ptr, False), "version": 3,
                                        "strides": None}

        t = torch.as_tensor(_HeapBuffer(), device=f"cuda:{self.lib.shmemx_device_id()}")
        if t.data_ptr() != ptr:
            raise RuntimeError("torch copied the heap buffer instead of wrapping it")
        return t if t.dtype == dtype else t.view(dtype)   # bfloat16: wrapped as its 16-bit patterns

    def _stream_reduction(self, op, dtype):
        key = ("stream", op, dtype)
        f = self._fns.get(key)
        if f is None:
            f = getattr(self.lib, f"shmemx_{dtype}_{op}_to_all_on_stream")   # the 16-bit floats' too
            f.restype = None
            f.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]
            self._fns[key] = f
        return f

    # ---- stream-ordered variants (include/shmemx.h)
    def to_all_on_stream(self, op, dtype, target, source, nreduce, PE_start, logPE_stride, PE_size, stream):
        self._stream_reduction(op, dtype)(target, source, nreduce, PE_start, logPE_stride, PE_size, None,
                                          self._psync_ptr, stream)

    def barrier_on_stream(self, PE_start, logPE_stride, PE_size, stream):
        self.lib.shmemx_barrier_on_stream(PE_start, logPE_stride, PE_size, stream)

    # ---- HIP streams and graphs, for callers of the stream-ordered API
    #      (resolved through the library's own libamdhip64 dependency)
    def _hip(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        if rc != 0:
            raise RuntimeError(f"{name} failed: {rc}")

    def stream_create(self):
        s = _vp()
        self._hip("hipStreamCreate", ctypes.byref(s))
        return s.value

    def stream_sync(self, stream):
        self._hip("hipStreamSynchronize", _vp(stream))

    def stream_destroy(self, stream):
        self._hip("hipStreamDestroy", _vp(stream))

    def capture_begin(self, stream, mode=2):  # hipStreamCaptureModeRelaxed
        self._hip("hipStreamBeginCapture", _vp(stream), _i(mode))

    def capture_end(self, stream):
        g, e = _vp(), _vp()
        self._hip("hipStreamEndCapture", _vp(stream), ctypes.byref(g))
        self._hip("hipGraphInstantiate", ctypes.byref(e), g, None, None, _sz(0))
        return g.value, e.value

    def graph_launch(self, exe, stream):
        self._hip("hipGraphLaunch", _vp(exe), _vp(stream))

    def graph_destroy(self, graph, exe):
        self._hip("hipGraphExecDestroy", _vp(exe))
        self._hip("hipGraphDestroy", _vp(graph))

    # ---- the combine layer (include/mi355_reduce.h)
    def combine(self, op, dtype, dst, srcs, n, stream=None):
        arr = (_vp * len(srcs))(*srcs)
        return self.lib.mi355_combine(OPS.index(op), DTYPES.index(dtype), dst, arr, len(srcs), n, stream)

    def combine_orders(self, op, dtype, dsts, srcs, n, stream=None):
        """dsts[q] (or None) <- the fold in member q's reference order (mi355_combine_orders)"""
        d = (_vp * len(dsts))(*[x if x else None for x in dsts])
        s = (_vp * len(srcs))(*srcs)
        return self.lib.mi355_combine_orders(OPS.index(op), DTYPES.index(dtype), d, s, len(srcs), n, stream)

    def combine_prefix(self, op, dtype, dsts, srcs, n, stream=None):
        """dsts[j] (or None) <- srcs[0] op ... op srcs[j], every prefix from one pass (mi355_combine_prefix)"""
        d = (_vp * len(dsts))(*[x if x else None for x in dsts])
        s = (_vp * len(srcs))(*srcs)
        return self.lib.mi355_combine_prefix(OPS.index(op), DTYPES.index(dtype), d, s, len(srcs), n, stream)

    def device_cus(self):
        """mi355_device_cus: the CU count the launchers cap their grids with"""
        return int(self.lib.mi355_device_cus())

    def last_launch_grid(self):
        """(gx, gy) of the kernel the combine layer launched last from this
        thread (mi355_last_launch_grid); (0, 0) before the first launch"""
        gx, gy = ctypes.c_uint(), ctypes.c_uint()
        self.lib.mi355_last_launch_grid(ctypes.byref(gx), ctypes.byref(gy))
        return gx.value, gy.value

    def last_kernel_name(self):
        """demangled name of that same kernel (mi355_last_kernel, mi355_kernel_name); "" before the first launch"""
        self.lib.mi355_last_kernel.restype = ctypes.c_void_p
        self.lib.mi355_kernel_name.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        buf = ctypes.create_string_buffer(512)
        return buf.value.decode() if self.lib.mi355_kernel_name(self.lib.mi355_last_kernel(), buf, 512) == 0 else ""

    def last_call_info(self):
        """dict of shmemx_last_call_info, or None before the first call"""
        ci = CallInfo()
        if self.lib.shmemx_last_call_info(ctypes.byref(ci)) != 0:
            return None
        d = {f: getattr(ci, f) for f, _ in CallInfo._fields_}
        d["schedule"] = ci.schedule.decode()
        d["kernel"] = ci.kernel.decode()
        return d

    def coherence_selftest(self):
        """(ran, passed, stale_without_acquire) of the init-time peer-read coherence test"""
        a, b, c = _i(), _i(), _i()
        self.lib.shmemx_coherence_selftest(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return bool(a.value), bool(b.value), bool(c.value)

    def coherence_sysload(self):
        """(sysload_fresh, acquires_skipped): the coherence test's check of the
        fused kernel's system-coherent loads, and whether its acquires are off"""
        a, b = _i(), _i()
        self.lib.shmemx_coherence_sysload(ctypes.byref(a), ctypes.byref(b))
        return bool(a.value), bool(b.value)

    PRODUCER_FIELDS = ("fused_plain_no_acquire", "fused_sysload", "fused_after_acquire",
                       "host_plain_no_acquire", "host_sysload", "host_after_acquire")

    def coherence_producer(self):
        """(ran, {field: fresh}) of the init test of a caller's producer path
        (plain stores in a null-stream kernel, then the fused kernel's or the
        multi-launch schedules' ordering; shmemx.h shmemx_coherence_producer)"""
        ran, fresh = _i(), (ctypes.c_int * 6)()
        self.lib.shmemx_coherence_producer(ctypes.byref(ran), fresh)
        return bool(ran.value), {k: bool(fresh[i]) for i, k in enumerate(self.PRODUCER_FIELDS)}

    def device_wait_report(self):
        """(slow, us): the init timing of device barriers over the job (shmemx.h
        shmemx_device_wait_report); slow = host barriers and no fused kernel"""
        slow, us = _i(), ctypes.c_double()
        self.lib.shmemx_device_wait_report(ctypes.byref(slow), ctypes.byref(us))
        return bool(slow.value), us.value

    def kernel_timing(self, enable):
        self.lib.shmemx_kernel_timing(1 if enable else 0)

    def kernel_timing_stats(self):
        n, tot, avg = ctypes.c_long(), ctypes.c_double(), ctypes.c_double()
        self.lib.shmemx_kernel_timing_stats(ctypes.byref(n), ctypes.byref(tot), ctypes.byref(avg))
        return n.value, tot.value, avg.value

    def kernel_timing_phase_stats(self, phase):
        """phase 0: each call's dominant kernel; 1: the P2P all-gather copy"""
        n, tot, avg = ctypes.c_long(), ctypes.c_double(), ctypes.c_double()
        self.lib.shmemx_kernel_timing_phase_stats(phase, ctypes.byref(n), ctypes.byref(tot), ctypes.byref(avg))
        return n.value, tot.value, avg.value


BENCH_LIB_PATH = os.path.join(LIB_DIR, "libshmem_bench.so")


def bench_loop(path=BENCH_LIB_PATH, name="double_sum"):
    """bench.py's timed loop in C (csrc/bench_loop.c): K back-to-back
    shmem_<name>_to_all calls (double_sum, float_max, longlong_and). Load
    after the main library."""
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    f = getattr(ctypes.CDLL(path), f"shmemb_{name}_loop")
    f.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i]
    f.restype = None
    return f


def bench_rotating(path=BENCH_LIB_PATH):
    """csrc/bench_loop.c shmemb_double_sum_rotating: K calls over npairs
    disjoint (target, source) pairs taken in turn; returns
    f(targets, sources, nreduce, pe_start, log_stride, pe_size, psync, k)."""
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    f = ctypes.CDLL(path).shmemb_double_sum_rotating
    f.argtypes = [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i]
    f.restype = None

    def run(targets, sources, nreduce, pe_start, log_stride, pe_size, psync, k):
        t = (_vp * len(targets))(*targets)
        s = (_vp * len(sources))(*sources)
        f(t, s, len(targets), nreduce, pe_start, log_stride, pe_size, None, psync, k)
    return run


def bench_call_times(path=BENCH_LIB_PATH):
    """csrc/bench_loop.c shmemb_double_sum_times: K shmem_double_sum_to_all
    calls, each timed alone; returns f(target, source, nreduce, PE_start,
    logPE_stride, PE_size, k) -> numpy array of k durations in us"""
    import numpy as np
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    f = ctypes.CDLL(path).shmemb_double_sum_times
    f.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp]
    f.restype = None

    def run(target, source, nreduce, pe_start, log_stride, pe_size, psync, k):
        out = np.zeros(k)
        f(target, source, nreduce, pe_start, log_stride, pe_size, None, psync, k, out.ctypes.data)
        return out
    return run


def kernel_code_hash(path=LIB_PATH):
    """sha256 (16 hex digits) of the gfx950 code objects the library carries
    (its .hip_fatbin ELF section): the machine code PMC counter profiles
    describe. Host-only changes leave it unchanged; any change to a kernel,
    a kernel header or the device compile flags changes it (the build is
    deterministic: rebuilding the same sources gives the same bytes).
    profiles/pmc_traffic.json records it per entry and bench.py reports an
    entry's HBM traffic only for a library with the same hash."""
    import struct
    with open(path, "rb") as f:
        b = f.read()
    shoff = struct.unpack_from("<Q", b, 0x28)[0]
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    secs = [struct.unpack_from("<IIQQQQ", b, shoff + i * shentsize) for i in range(shnum)]
    stroff = secs[shstrndx][4]
    for name, _typ, _flags, _addr, off, size in secs:
        if b[stroff + name:b.index(b"\0", stroff + name)] == b".hip_fatbin":
            return hashlib.sha256(b[off:off + size]).hexdigest()[:16]
    raise RuntimeError(f"{path} has no .hip_fatbin section")


def shard_bounds(lib, n, elem_size, nshards, i):
    lo, hi = _sz(), _sz()
    lib.mi355_shard_bounds(n, elem_size, nshards, i, ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value
