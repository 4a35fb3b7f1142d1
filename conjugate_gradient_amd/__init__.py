"""conjugate_gradient_amd -- MI355X-native conjugate-gradient hot path.

Python mirror of the reference's solver interface over the C ABI of
``lib/libcgx.so`` (declared in ``include/cgx.h``).  The reference
(mawunyega/conjugate_gradient) is a set of C programs; the functions a user
of that code calls are reproduced here with the same names and argument
meaning so the parity tests read like the reference's own call sites:

=====================  ==============================================  =========================
reference               where                                           here
=====================  ==============================================  =========================
``conjugrad(A,b,x)``    serialConjugate.c:180-259                       :func:`conjugrad`
``conjugrad(..., P)``   parallel_cg.c:248-345 (row blocks, P ranks)     :func:`conjugrad` (shards)
``matVec``              serialConjugate.c:109-120                       :func:`matVec`
``vecVec``              serialConjugate.c:145-155                       :func:`vecVec`
``residual``            serialConjugate.c:124-131                       :func:`residual`
``scalarVec+vecAdd``    serialConjugate.c:221-243                       :func:`update_xr`,
                                                                        :func:`update_p`
``initialize``          serialConjugate.c:85-105                        :func:`read_text`
=====================  ==============================================  =========================

Everything runs on the GPU through libcgx.so; there is no CPU fallback.  If
the library is missing or no GPU is visible the calls raise.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

__all__ = [
    "CGX_F64", "CGX_F32_REF", "CGX_A_F32", "CGX_TIMING", "CGX_HOST_STREAM", "CGX_NO_OVERLAP", "CGX_COMM_P2P", "CGX_SYMMETRIC",
    "CGX_PHASES", "CGX_PEER_ACTIVE", "CGX_SMALL_ACTIVE", "CGX_FOLD_ACTIVE", "CGX_XDEFER_ACTIVE", "CGX_XDEFER3_ACTIVE",
    "CGX_PULL_ACTIVE", "CGX_FOLDED_ACTIVE", "CGX_HALO_PULL_ACTIVE", "CGX_THREADS_ACTIVE", "CGX_HALO_OVERLAP_ACTIVE",
    "PHASE_NAMES", "overlap_rule", "CgxError", "Stats",
    "Solver", "lib", "build",
    "device_pci_bus_id", "device_link",
    "CGX_MAX_NRHS", "matVec_nrhs",
    "CGX_CSR_ACTIVE", "spmv_csr", "spmm_csr",
    "CGX_BSR_ACTIVE", "CGX_MAX_BSR_BLOCK", "bsr_check", "spmv_bsr",
    "CGX_DIA_ACTIVE", "dia_check", "spmv_dia",
    "CGX_DIA_SYM_ACTIVE", "dia_sym_check", "spmv_dia_sym",
    "CGX_CSR_HALO_ACTIVE", "csr_halo_counts", "csr_halo_list", "gather_indexed",
    "CGX_PRECOND_ACTIVE", "PRECOND_KINDS", "PC_BLOCK", "CGX_MAX_PC_BLOCK", "csr_diag_blocks", "precond_block_invert",
    "conjugrad", "matVec", "vecVec", "residual", "update_xr", "update_p", "read_text",
    "count_text", "read_dims", "device_count", "get_unique_id", "DeviceArray",
]

CGX_F64 = 0x0
CGX_F32_REF = 0x1
CGX_A_F32 = 0x2
CGX_TIMING = 0x100
CGX_HOST_STREAM = 0x200
CGX_NO_OVERLAP = 0x400
CGX_OVERLAP_ACTIVE = 0x800
CGX_FUSED_ACTIVE = 0x2000
CGX_DETERMINISTIC = 0x4000
CGX_COMM_P2P = 0x1000
CGX_SYMMETRIC = 0x8000
CGX_PHASES = 0x10000
CGX_PEER_ACTIVE = 0x20000
CGX_SMALL_ACTIVE = 0x40000
CGX_FOLD_ACTIVE = 0x80000
CGX_XDEFER_ACTIVE = 0x100000
CGX_XDEFER3_ACTIVE = 0x200000
CGX_PULL_ACTIVE = 0x400000
CGX_FOLDED_ACTIVE = 0x800000
CGX_HALO_PULL_ACTIVE = 0x1000000
CGX_THREADS_ACTIVE = 0x2000000
CGX_HALO_OVERLAP_ACTIVE = 0x4000000
CGX_CSR_ACTIVE = 0x8000000  # reported in info.flags: a cgx_create_csr context (Solver(n, csr_nnz=...))
CGX_PRECOND_ACTIVE = 0x10000000  # reported in info.flags: a CSR context iterating with a diagonal preconditioner
# reported in info.flags: a CSR solver over several row blocks (devices=) exchanging p by index lists
CGX_CSR_HALO_ACTIVE = 0x20000000
CGX_BSR_ACTIVE = 0x40000000  # reported in info.flags beside CGX_CSR_ACTIVE: a CSR solver that is block-valued (set_bsr)
CGX_MAX_BSR_BLOCK = 8  # the largest block size of set_bsr
CGX_DIA_ACTIVE = 0x4  # reported in info.flags beside CGX_CSR_ACTIVE: a CSR solver that is diagonal-valued (set_dia)
CGX_DIA_SYM_ACTIVE = 0x8  # ... beside CGX_DIA_ACTIVE: the upper diagonals of a symmetric A alone (set_dia_sym)
# cgx_set_precond's kinds, CGX_PC_NONE / CGX_PC_JACOBI / CGX_PC_DIAG (include/cgx.h), by the names Solver.precond
# reports.  Kept out of the CGX_* names: those are the flag words, and a kind is not a bit of one.
PRECOND_KINDS = {"none": 0, "jacobi": 1, "diag": 2}
# CGX_PC_BLOCK, the block-Jacobi kind: it has its own entry points (Solver.set_precond_block), so it stays out of the
# dict of kinds cgx_set_precond knows, and, a kind and not a flag bit, out of the CGX_* names; Solver.precond reports
# it as "block".
PC_BLOCK = 3
CGX_MAX_PC_BLOCK = 8  # the largest block size
CGX_MAX_NRHS = 8  # cgx_create_nrhs: systems solved together on one matrix

# cgx_phase_times indices (include/cgx.h), in the order the phases tile an iteration
PHASE_NAMES = ("matvec_own", "gather_exposed", "matvec", "combine_pap", "update_r", "combine_rr", "update_xp",
               "gap", "iteration", "matvec_busy")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcgx.so")
CLI_PATH = os.path.join(_HERE, "bin", "cg_hip")
_LIB = None


class CgxError(RuntimeError):
    def __init__(self, code: int, what: str):
        L = lib()
        msg = L.cgx_strerror(code).decode()
        detail = L.cgx_last_error().decode()
        super().__init__(f"{what}: {msg} ({detail})" if detail else f"{what}: {msg}")
        self.code = code


class Stats(ctypes.Structure):
    _fields_ = [
        ("iterations", ctypes.c_int64),
        ("converged", ctypes.c_int),
        ("rr", ctypes.c_double),
        ("solve_ms", ctypes.c_double),
        ("matvec_ms", ctypes.c_double),
        ("matvec_count", ctypes.c_int64),
        ("total_iterations", ctypes.c_int64),
    ]


class Info(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_int64), ("lda", ctypes.c_int64), ("nranks", ctypes.c_int),
        ("nshards", ctypes.c_int), ("rank0", ctypes.c_int), ("row0", ctypes.c_int64),
        ("nrows", ctypes.c_int64), ("flags", ctypes.c_int), ("elem_bytes", ctypes.c_int),
    ]


class PhaseTimes(ctypes.Structure):
    _fields_ = [("samples", ctypes.c_int64 * 10), ("median_us", ctypes.c_double * 10),
                ("mean_us", ctypes.c_double * 10)]


class CommInfo(ctypes.Structure):
    _fields_ = [("rccl_nranks", ctypes.c_int), ("rccl_device", ctypes.c_int), ("rccl_rank", ctypes.c_int),
                ("device", ctypes.c_int), ("pci_bus_id", ctypes.c_char * 32)]


class OverlapInfo(ctypes.Structure):
    _fields_ = [("active", ctypes.c_int), ("decided_by", ctypes.c_int), ("allgather_us", ctypes.c_double),
                ("split_us", ctypes.c_double), ("one_launch_us", ctypes.c_double), ("split_cost_us", ctypes.c_double),
                ("overlap_form_us", ctypes.c_double), ("plain_form_us", ctypes.c_double), ("margin", ctypes.c_double),
                ("forms_ms", ctypes.c_double)]


# cgx_overlap_info.decided_by
OVERLAP_DECIDED_BY = {0: "measured", 1: "forced_on", 2: "off", 3: "n/a"}


def overlap_rule(info: dict) -> bool:
    """The library's decision rule on an overlap_info() dict (measured case):
    the overlapped form when it beat the plain form by more than the margin."""
    return info["overlap_form_us"] < (1.0 - info["margin"]) * info["plain_form_us"]


class UniqueId(ctypes.Structure):
    _fields_ = [("bytes", ctypes.c_char * 128)]


def build() -> None:
    """Compile libcgx.so and cg_hip for gfx950 (hipcc; works without a GPU)."""
    subprocess.run(["make", "-s", "-C", os.path.join(_HERE, "csrc")], check=True)


def lib() -> ctypes.CDLL:
    """Load libcgx.so; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} missing: run `make -C conjugate_gradient_amd/csrc` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    i64, i32, f64, vp, sz = ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    pctx = ctypes.POINTER(ctypes.c_void_p)
    sigs = {
        "cgx_strerror": ([i32], ctypes.c_char_p),
        "cgx_last_error": ([], ctypes.c_char_p),
        "cgx_version": ([], i32),
        "cgx_device_count": ([ctypes.POINTER(i32)], i32),
        "cgx_hip_last_error": ([], i32),
        "cgx_device_pci_bus_id": ([i32, ctypes.c_char_p, i32], i32),
        "cgx_device_link": ([i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)], i32),
        "cgx_get_comm_info": ([vp, ctypes.POINTER(CommInfo)], i32),
        "cgx_get_overlap_info": ([vp, ctypes.POINTER(OverlapInfo)], i32),
        "cgx_get_phase_times": ([vp, ctypes.POINTER(PhaseTimes)], i32),
        "cgx_create": ([pctx, i64, i32, i32], i32),
        "cgx_create_multi": ([pctx, i64, i32, ctypes.POINTER(i32), i32], i32),
        "cgx_create_nrhs": ([pctx, i64, i32, i32, i32], i32),
        "cgx_get_nrhs": ([vp, ctypes.POINTER(i32)], i32),
        "cgx_get_stats_rhs": ([vp, i32, ctypes.POINTER(Stats)], i32),
        "cgx_residual_norms": ([vp, ctypes.POINTER(f64), ctypes.POINTER(f64)], i32),
        "cgx_matvec_nrhs": ([vp, i64, i64, i64, i32, vp, i64, vp, i64, vp], i32),
        "cgx_csr_check": ([i64, i64, vp, vp], i32),
        "cgx_create_csr": ([pctx, i64, i64, i32, i32], i32),
        "cgx_set_csr": ([vp, vp, vp, vp], i32),
        "cgx_set_csr_f32": ([vp, vp, vp, vp], i32),
        "cgx_spmv_csr": ([i64, i64, vp, vp, vp, vp, vp, vp], i32),
        "cgx_bsr_check": ([i64, i64, vp, vp], i32),
        "cgx_set_bsr": ([vp, i32, vp, vp, vp], i32),
        "cgx_bsr_tile_values": ([i64, i32, vp, vp, vp], i32),
        "cgx_spmv_bsr": ([i64, i64, i32, vp, vp, vp, vp, vp, vp], i32),
        "cgx_dia_check": ([i64, i64, vp], i32),
        "cgx_set_dia": ([vp, i64, vp, vp, i64], i32),
        "cgx_spmv_dia": ([i64, i64, vp, vp, i64, vp, vp, vp], i32),
        "cgx_dia_sym_check": ([i64, i64, vp], i32),
        "cgx_set_dia_sym": ([vp, i64, vp, vp, i64], i32),
        "cgx_spmv_dia_sym": ([i64, i64, vp, vp, i64, vp, vp, vp], i32),
        "cgx_spmv_csr_f32": ([i64, i64, vp, vp, vp, vp, vp, vp], i32),
        "cgx_create_csr_nrhs": ([pctx, i64, i64, i32, i32, i32], i32),
        "cgx_create_csr_multi": ([pctx, i64, i64, i32, ctypes.POINTER(i32), i32], i32),
        "cgx_csr_halo_counts": ([i64, i32, vp, vp, vp], i32),
        "cgx_csr_halo_list": ([i64, i32, vp, vp, i32, i32, vp], i32),
        "cgx_get_csr_halo": ([vp, vp], i32),
        "cgx_gather_indexed": ([vp, vp, i64, vp, vp], i32),
        "cgx_spmm_csr": ([i64, i64, vp, vp, vp, i32, vp, i64, vp, i64, vp], i32),
        "cgx_spmm_csr_f32": ([i64, i64, vp, vp, vp, i32, vp, i64, vp, i64, vp], i32),
        "cgx_precond_diag_check": ([i64, vp], i32),
        "cgx_set_precond": ([vp, i32], i32),
        "cgx_set_precond_diag": ([vp, vp], i32),
        "cgx_get_precond": ([vp, ctypes.POINTER(i32)], i32),
        "cgx_get_precond_diag": ([vp, vp], i32),
        "cgx_set_precond_block": ([vp, i32], i32),
        "cgx_set_precond_block_values": ([vp, i32, vp], i32),
        "cgx_get_precond_block": ([vp, ctypes.POINTER(i32), vp], i32),
        "cgx_precond_block_invert": ([i64, i32, vp, vp], i32),
        "cgx_precond_block_check": ([i64, i32, vp], i32),
        "cgx_csr_diag_blocks": ([i64, i32, vp, vp, vp, vp, vp], i32),
        "cgx_get_unique_id": ([ctypes.POINTER(UniqueId)], i32),
        "cgx_rccl_available": ([], i32),
        "cgx_create_rank": ([pctx, i64, i32, i32, ctypes.POINTER(UniqueId), i32, i32], i32),
        "cgx_create_poisson": ([pctx, i64, i32, i32], i32),
        "cgx_create_poisson_multi": ([pctx, i64, i32, ctypes.POINTER(i32), i32], i32),
        "cgx_create_poisson_rank": ([pctx, i64, i32, i32, ctypes.POINTER(UniqueId), i32, i32], i32),
        "cgx_fill": ([vp, f64, f64], i32),
        "cgx_destroy": ([vp], i32),
        "cgx_get_info": ([vp, ctypes.POINTER(Info)], i32),
        "cgx_set_rows": ([vp, i64, i64, vp, i64, vp, vp], i32),
        "cgx_set_system": ([vp, vp, vp, vp], i32),
        "cgx_generate_spd": ([vp, ctypes.c_uint64], i32),
        "cgx_get_x": ([vp, vp], i32),
        "cgx_set_x": ([vp, vp], i32),
        "cgx_solve": ([vp, vp, f64, i64, ctypes.POINTER(Stats)], i32),
        "cgx_solve_begin": ([vp], i32),
        "cgx_conjugrad": ([vp, vp, vp, i64, i32, f64, i64, ctypes.POINTER(Stats)], i32),
        "cgx_iterate": ([vp, i64, f64, ctypes.POINTER(i64), ctypes.POINTER(i32)], i32),
        "cgx_get_stats": ([vp, ctypes.POINTER(Stats)], i32),
        "cgx_reset_timing": ([vp], i32),
        "cgx_synchronize": ([vp], i32),
        "cgx_stream": ([vp], vp),
        "cgx_residual_norm": ([vp, ctypes.POINTER(f64), ctypes.POINTER(f64)], i32),
        "cgx_set_matvec_plan": ([vp, i32, i32, i32, i32], i32),
        "cgx_get_matvec_plan": ([vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32),
                                 ctypes.POINTER(i32)], i32),
        "cgx_dev_malloc": ([ctypes.POINTER(vp), sz], i32),
        "cgx_dev_free": ([vp], i32),
        "cgx_memcpy_h2d": ([vp, vp, sz], i32),
        "cgx_memcpy_d2h": ([vp, vp, sz], i32),
        "cgx_dev_synchronize": ([], i32),
        "cgx_matvec": ([i32, vp, i64, i64, i64, vp, vp, vp], i32),
        "cgx_dot": ([i32, i64, vp, vp, vp, vp], i32),
        "cgx_residual": ([i32, i64, vp, vp, vp, vp, vp, vp], i32),
        "cgx_update_xr": ([i32, i64, vp, vp, vp, vp, vp, vp, vp, vp], i32),
        "cgx_update_p": ([i32, i64, vp, vp, vp, vp, vp], i32),
        "cgx_text_count": ([ctypes.c_char_p], i64),
        "cgx_text_read": ([ctypes.c_char_p, i64, i32, vp, i32], i32),
        "cgx_text_dims": ([ctypes.c_char_p, ctypes.POINTER(i64)], i32),
    }
    for name, (args, res) in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _LIB = L
    return L


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise CgxError(rc, what)


def _ptr(a: np.ndarray) -> int:
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("array must be C-contiguous")
    return a.ctypes.data


def _dtype(flags: int) -> np.dtype:
    return np.dtype(np.float32) if flags & CGX_F32_REF else np.dtype(np.float64)


def _a_dtype(flags: int) -> np.dtype:
    """A's element type: float32 under CGX_A_F32 (beside float64 vectors), else the vectors'."""
    return np.dtype(np.float32) if flags & CGX_A_F32 else _dtype(flags)


def device_count() -> int:
    n = ctypes.c_int(0)
    _check(lib().cgx_device_count(ctypes.byref(n)), "cgx_device_count")
    return n.value


def device_pci_bus_id(device: int) -> str:
    buf = ctypes.create_string_buffer(32)
    _check(lib().cgx_device_pci_bus_id(device, buf, 32), "cgx_device_pci_bus_id")
    return buf.value.decode()


def device_link(a: int, b: int) -> dict:
    """The link between two visible devices: HSA link type (4 = xGMI, 2 = PCIe,
    -1 unknown), hop count, and whether a can access b's memory directly."""
    lt, hops, peer = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _check(lib().cgx_device_link(a, b, ctypes.byref(lt), ctypes.byref(hops), ctypes.byref(peer)), "cgx_device_link")
    names = {0: "hypertransport", 1: "qpi", 2: "pcie", 3: "infiniband", 4: "xgmi"}
    return {"link": names.get(lt.value, "unknown" if lt.value < 0 else str(lt.value)), "hops": hops.value,
            "peer_access": bool(peer.value)}


def get_unique_id() -> bytes:
    """RCCL bootstrap id for cgx_create_rank (call on rank 0, broadcast)."""
    u = UniqueId()
    _check(lib().cgx_get_unique_id(ctypes.byref(u)), "cgx_get_unique_id")
    return ctypes.string_at(ctypes.addressof(u), 128)  # may contain NULs


# ----------------------------------------------------------------------------
# text I/O (initialize(), serialConjugate.c:85-105)
# ----------------------------------------------------------------------------
def count_text(path: str) -> int:
    c = lib().cgx_text_count(path.encode())
    if c < 0:
        raise FileNotFoundError(path)
    return int(c)


def read_text(path: str, count: int, dtype=np.float64, threads: int = 4) -> np.ndarray:
    dt = np.dtype(dtype)
    out = np.empty(count, dtype=dt)
    rc = lib().cgx_text_read(path.encode(), count, 1 if dt == np.float32 else 0, _ptr(out), threads)
    if rc == -1:
        raise FileNotFoundError(path)
    if rc == -2:
        raise ValueError(f"{path}: fewer than {count} numbers")
    if rc != 0:
        raise ValueError(f"{path}: malformed number")
    return out


def read_dims(path: str) -> tuple[int, int, int, int]:
    d = (ctypes.c_int64 * 4)()
    rc = lib().cgx_text_dims(path.encode(), d)
    if rc != 0:
        raise ValueError(f"{path}: cannot read dimensions (rc={rc})")
    return tuple(int(v) for v in d)


# ----------------------------------------------------------------------------
# device arrays (for the kernel-level entry points)
# ----------------------------------------------------------------------------
class DeviceArray:
    """A device buffer owned by libcgx (hipMalloc), with host copy helpers."""

    def __init__(self, count: int, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.count = int(count)
        p = ctypes.c_void_p()
        _check(lib().cgx_dev_malloc(ctypes.byref(p), max(1, self.count) * self.dtype.itemsize), "cgx_dev_malloc")
        self.ptr = p.value

    @classmethod
    def from_host(cls, a: np.ndarray, dtype=None) -> "DeviceArray":
        a = np.ascontiguousarray(a, dtype=dtype or a.dtype)
        d = cls(a.size, a.dtype)
        if a.size:
            _check(lib().cgx_memcpy_h2d(d.ptr, _ptr(a), a.nbytes), "cgx_memcpy_h2d")
        return d

    def to_host(self) -> np.ndarray:
        out = np.empty(self.count, self.dtype)
        if self.count:
            _check(lib().cgx_dev_synchronize(), "cgx_dev_synchronize")
            _check(lib().cgx_memcpy_d2h(_ptr(out), self.ptr, out.nbytes), "cgx_memcpy_d2h")
        return out

    def free(self) -> None:
        if self.ptr:
            lib().cgx_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _dt_flag(dtype) -> int:
    return CGX_F32_REF if np.dtype(dtype) == np.float32 else CGX_F64


def _need(cond: bool, msg: str) -> None:
    """Explicit size check before a C call (not `assert`: python -O strips it;
    a short buffer passed on would be read or written past its end)."""
    if not cond:
        raise ValueError(msg)


def _fits(arrs, n: int, what: str) -> None:
    for a in arrs:
        if a is not None:
            _need(a.count >= n, f"{what}: device array of {a.count} elements, {n} needed")


def matVec(A: DeviceArray, v: DeviceArray, out: DeviceArray, rows: int, cols: int, lda: int | None = None) -> None:
    """serialConjugate.c:109-120 / parallel_cg.c:172-184 (rows = local_row).
    A float32 ``A`` with float64 ``v`` and ``out`` runs the CGX_A_F32 kernel
    (A widened exactly, fp64 arithmetic)."""
    lda = lda or cols
    _need(rows >= 0 and cols >= 0 and lda >= cols, "matVec: need rows, cols >= 0 and lda >= cols")
    if rows and cols:
        _fits([A], (rows - 1) * lda + cols, "matVec A")
        _fits([v], cols, "matVec v")
        _fits([out], rows, "matVec out")
    dt = _dt_flag(A.dtype)
    if A.dtype == np.float32 and v.dtype == np.float64 and out.dtype == np.float64:
        dt = CGX_A_F32
    else:
        _need(v.dtype == A.dtype and out.dtype == A.dtype,
              "matVec: A, v and out of one dtype, or a float32 A with float64 v and out")
    _check(lib().cgx_matvec(dt, A.ptr, lda or cols, rows, cols, v.ptr, out.ptr, None), "cgx_matvec")


def matVec_nrhs(A: DeviceArray, V: DeviceArray, Out: DeviceArray, rows: int, cols: int, nrhs: int,
                lda: int | None = None, ldv: int | None = None, ldo: int | None = None, v_offset: int = 0) -> None:
    """``nrhs`` matVecs in one pass over A (fp64): Out[j*ldo + i] = sum_c A[i*lda + c] * V[j*ldv + c].
    Column j is :func:`matVec`'s result on column j of V bit for bit.  ``v_offset``: V starts that many
    elements into its device array (an odd offset takes every column off the 16-byte grid)."""
    lda, ldv, ldo = lda or cols, ldv or cols, ldo or rows
    _need(1 <= nrhs <= CGX_MAX_NRHS, f"matVec_nrhs: nrhs must be in [1, {CGX_MAX_NRHS}] (got {nrhs})")
    _need(rows >= 0 and cols >= 0 and lda >= cols and ldv >= cols and ldo >= rows and v_offset >= 0,
          "matVec_nrhs: need rows, cols >= 0, lda >= cols, ldv >= cols and ldo >= rows")
    _need(A.dtype == np.float64 and V.dtype == np.float64 and Out.dtype == np.float64, "matVec_nrhs: float64 only")
    if rows and cols:
        _fits([A], (rows - 1) * lda + cols, "matVec_nrhs A")
        _fits([V], v_offset + (nrhs - 1) * ldv + cols, "matVec_nrhs V")
        _fits([Out], (nrhs - 1) * ldo + rows, "matVec_nrhs Out")
    _check(lib().cgx_matvec_nrhs(A.ptr, lda, rows, cols, nrhs, V.ptr + 8 * v_offset, ldv, Out.ptr, ldo, None),
           "cgx_matvec_nrhs")


def _a_f32_flag(what: str, a_f32) -> bool:
    _need(isinstance(a_f32, (bool, np.bool_)), f"{what}: a_f32 must be True or False (got {a_f32!r})")
    return bool(a_f32)


def _csr_arrays(indptr, indices=None, data=None, a_f32: bool = False):
    """(indptr int64, indices int32, data float64), contiguous; ``indptr`` may be
    an object with ``.indptr / .indices / .data`` (no scipy needed).  ``a_f32``:
    data as float32 (a float64 array is rounded to nearest, as the dense
    CGX_A_F32 path rounds A)."""
    if indices is None and data is None and hasattr(indptr, "indptr"):
        indptr, indices, data = indptr.indptr, indptr.indices, indptr.data
    _need(indices is not None and data is not None, "CSR: indptr, indices and data are needed")
    rp = np.ascontiguousarray(indptr, np.int64)
    ci = np.ascontiguousarray(indices, np.int32)
    va = np.ascontiguousarray(data, np.float32 if a_f32 else np.float64)
    _need(rp.ndim == 1 and ci.ndim == 1 and va.ndim == 1, "CSR: indptr, indices and data are one-dimensional")
    _need(ci.size == va.size, f"CSR: {ci.size} indices but {va.size} values")
    return rp, ci, va


def _csr_checked(what: str, rp, ci, rows: int, cols: int) -> None:
    """The structure check of the kernel-level CSR calls: raises unless every index is inside [0, cols)."""
    _csr_checked_with(lib().cgx_csr_check, "cgx_csr_check", what, rp, ci, rows, cols)


def _csr_checked_with(check, check_name: str, what: str, rp, ci, rows: int, cols: int) -> None:
    """_csr_checked through `check` (cgx_csr_check, or cgx_bsr_check on block rows and block columns)."""
    # cgx_csr_check takes a square structure: fewer rows than columns are
    # padded with empty rows (the same last row pointer), so the columns are
    # checked against cols; with more rows than columns they are checked here
    nsq = max(rows, cols)
    rp_sq = rp if nsq == rows else np.concatenate([rp, np.full(nsq - rows, rp[-1], np.int64)])
    _check(check(nsq, ci.size, _ptr(rp_sq), _ptr(ci)), check_name)
    bad = np.flatnonzero(ci >= cols)
    _need(bad.size == 0, f"{what}: indices[{bad[0] if bad.size else 0}] outside [0, {cols})")


def spmv_csr(indptr, indices, data, v: DeviceArray, out: DeviceArray, rows: int, cols: int, *,
             a_f32: bool = False) -> None:
    """out[i] = sum_e data[e] * v[indices[e]] over row i's entries, in stored
    order (k_csr_mult_f64; the plan from CGX_SPMV_PLAN).  The structure comes
    as host arrays: it is checked (cgx_csr_check) and only then uploaded, so the
    kernel never sees an index outside v.  ``a_f32=True`` (cgx_spmv_csr_f32): data
    is cast to float32 and stays float32 on the device; the kernel widens it
    exactly, so the result is this call's on ``data.astype(float32)`` bit for bit."""
    a_f32 = _a_f32_flag("spmv_csr", a_f32)
    rp, ci, va = _csr_arrays(indptr, indices, data, a_f32)
    _need(rows >= 1 and cols >= 1, "spmv_csr: need rows, cols >= 1")
    _need(rp.size == rows + 1, f"spmv_csr: indptr has {rp.size} entries, rows + 1 = {rows + 1} needed")
    _need(v.dtype == np.float64 and out.dtype == np.float64, "spmv_csr: float64 only")
    _fits([v], cols, "spmv_csr v")
    _fits([out], rows, "spmv_csr out")
    L = lib()
    _csr_checked("spmv_csr", rp, ci, rows, cols)
    d_rp, d_ci, d_va = DeviceArray.from_host(rp), DeviceArray.from_host(ci), DeviceArray.from_host(va)
    try:
        fn, name = (L.cgx_spmv_csr_f32, "cgx_spmv_csr_f32") if a_f32 else (L.cgx_spmv_csr, "cgx_spmv_csr")
        _check(fn(rows, cols, d_rp.ptr, d_ci.ptr, d_va.ptr, v.ptr, out.ptr, None), name)
        _check(L.cgx_dev_synchronize(), "cgx_dev_synchronize")
    finally:
        for d in (d_rp, d_ci, d_va):
            d.free()


def spmm_csr(indptr, indices, data, V: DeviceArray, Out: DeviceArray, rows: int, cols: int, nrhs: int,
             ldv: int | None = None, ldo: int | None = None, *, a_f32: bool = False) -> None:
    """``nrhs`` sparse matVecs in one pass over the CSR arrays (k_csr_mult_f64; the plan from
    CGX_SPMM_PLAN): Out[j*ldo + i] = sum_e data[e] * V[j*ldv + indices[e]].  Column j is
    :func:`spmv_csr`'s result on column j of V bit for bit at the same T.  The structure is
    checked on the host before anything is uploaded, as :func:`spmv_csr` does.
    ``a_f32=True`` (cgx_spmm_csr_f32): float32 data, as :func:`spmv_csr`'s."""
    a_f32 = _a_f32_flag("spmm_csr", a_f32)
    rp, ci, va = _csr_arrays(indptr, indices, data, a_f32)
    ldv, ldo = ldv or cols, ldo or rows
    _need(isinstance(nrhs, (int, np.integer)) and 1 <= nrhs <= CGX_MAX_NRHS,
          f"spmm_csr: nrhs must be in [1, {CGX_MAX_NRHS}] (got {nrhs})")
    _need(rows >= 1 and cols >= 1 and ldv >= cols and ldo >= rows,
          "spmm_csr: need rows, cols >= 1, ldv >= cols and ldo >= rows")
    _need(rp.size == rows + 1, f"spmm_csr: indptr has {rp.size} entries, rows + 1 = {rows + 1} needed")
    _need(V.dtype == np.float64 and Out.dtype == np.float64, "spmm_csr: float64 only")
    _fits([V], (nrhs - 1) * ldv + cols, "spmm_csr V")
    _fits([Out], (nrhs - 1) * ldo + rows, "spmm_csr Out")
    L = lib()
    _csr_checked("spmm_csr", rp, ci, rows, cols)
    d_rp, d_ci, d_va = DeviceArray.from_host(rp), DeviceArray.from_host(ci), DeviceArray.from_host(va)
    try:
        fn, name = (L.cgx_spmm_csr_f32, "cgx_spmm_csr_f32") if a_f32 else (L.cgx_spmm_csr, "cgx_spmm_csr")
        _check(fn(rows, cols, d_rp.ptr, d_ci.ptr, d_va.ptr, int(nrhs), V.ptr, ldv, Out.ptr, ldo, None), name)
        _check(L.cgx_dev_synchronize(), "cgx_dev_synchronize")
    finally:
        for d in (d_rp, d_ci, d_va):
            d.free()


def _bsr_arrays(what: str, indptr, indices=None, data=None):
    """(indptr int64, indices int32, data float64 of shape (nnzb, bs, bs), bs), contiguous; ``indptr`` may be an
    object with ``.indptr / .indices / .data`` such as scipy's bsr_matrix (no scipy needed).  Raises unless the
    blocks are square with 2 <= bs <= CGX_MAX_BSR_BLOCK."""
    if indices is None and data is None and hasattr(indptr, "indptr"):
        indptr, indices, data = indptr.indptr, indptr.indices, indptr.data
    _need(indices is not None and data is not None, f"{what}: indptr, indices and data are needed")
    d = np.asarray(data)
    _need(d.dtype.kind in "fiu", f"{what}: data must be real numbers (got {d.dtype})")
    rp = np.ascontiguousarray(indptr, np.int64)
    ci = np.ascontiguousarray(indices, np.int32)
    va = np.ascontiguousarray(d, np.float64)
    _need(rp.ndim == 1 and ci.ndim == 1, f"{what}: indptr and indices are one-dimensional")
    _need(va.ndim == 3 and va.shape[1] == va.shape[2],
          f"{what}: data must have shape (nnzb, bs, bs) (got {va.shape})")
    bs = int(va.shape[1])
    _need(bs != 1, f"{what}: bs = 1 is scalar CSR (set_csr / spmv_csr)")
    _need(2 <= bs <= CGX_MAX_BSR_BLOCK, f"{what}: bs must be in [2, {CGX_MAX_BSR_BLOCK}] (got {bs})")
    _need(ci.size == va.shape[0], f"{what}: {ci.size} indices but {va.shape[0]} blocks")
    return rp, ci, va, bs


def _dia_arrays(what: str, offsets, data=None):
    """(offsets int32[ndiag], data float64 of shape (ndiag, ld)), contiguous, scipy's dia_matrix layout
    (``data[k, j] = A[j - offsets[k], j]``); ``offsets`` may be an object with ``.offsets / .data`` such as scipy's
    dia_matrix (no scipy needed)."""
    if data is None and hasattr(offsets, "offsets"):
        offsets, data = offsets.offsets, offsets.data
    _need(data is not None, f"{what}: offsets and data are needed")
    d = np.asarray(data)
    o = np.asarray(offsets)
    _need(d.dtype.kind in "fiu", f"{what}: data must be real numbers (got {d.dtype})")
    _need(o.dtype.kind in "iu" or o.size == 0, f"{what}: offsets must be integers (got {o.dtype})")
    _need(o.ndim == 1, f"{what}: offsets are one-dimensional")
    _need(d.ndim == 2, f"{what}: data must have shape (ndiag, ld) (got {d.shape})")
    _need(o.size == d.shape[0], f"{what}: {o.size} offsets but {d.shape[0]} diagonals")
    _need(o.size == 0 or (int(o.min()) >= -2**31 and int(o.max()) < 2**31), f"{what}: an offset does not fit int32")
    return np.ascontiguousarray(o, np.int32), np.ascontiguousarray(d, np.float64)


def _dia_check(what: str, offsets, n) -> None:
    """dia_check / dia_sym_check under the caller's name ``what`` (cgx_<what> is the C call)."""
    o = np.asarray(offsets)
    _need(o.ndim == 1 and (o.dtype.kind in "iu" or o.size == 0), f"{what}: offsets are one-dimensional integers")
    _need(isinstance(n, (int, np.integer)), f"{what}: n is an integer")
    _need(o.size == 0 or (int(o.min()) >= -2**31 and int(o.max()) < 2**31), f"{what}: an offset does not fit int32")
    o = np.ascontiguousarray(o, np.int32)
    _check(getattr(lib(), f"cgx_{what}")(int(n), o.size, _ptr(o) if o.size else None), f"cgx_{what}")


def _spmv_dia(what: str, sym: bool, offsets, data, v: DeviceArray, out: DeviceArray, n) -> None:
    """spmv_dia / spmv_dia_sym under the caller's name ``what`` (cgx_<what> is the C call)."""
    o, d = _dia_arrays(what, offsets, data)
    _need(isinstance(n, (int, np.integer)) and n >= 1, f"{what}: need an integer n >= 1")
    ld = int(d.shape[1])
    _need(ld >= n, f"{what}: data has {ld} columns, n = {n} needed")
    _need(v.dtype == np.float64 and out.dtype == np.float64, f"{what}: float64 only")
    _fits([v], n, f"{what} v")
    _fits([out], n, f"{what} out")
    L = lib()
    check = "cgx_dia_sym_check" if sym else "cgx_dia_check"
    _check(getattr(L, check)(int(n), o.size, _ptr(o) if o.size else None), check)
    ndiag = int(o.size)
    d_o = DeviceArray.from_host(o if ndiag else np.zeros(1, np.int32))
    d_d = DeviceArray.from_host(d.reshape(-1) if ndiag else np.zeros(1))
    try:
        _check(getattr(L, f"cgx_{what}")(int(n), ndiag, d_o.ptr, d_d.ptr, ld, v.ptr, out.ptr, None), f"cgx_{what}")
        _check(L.cgx_dev_synchronize(), "cgx_dev_synchronize")
    finally:
        for a in (d_o, d_d):
            a.free()


def dia_check(offsets, n: int) -> None:
    """cgx_dia_check (host only, no GPU): raises CgxError(-4) naming the first offset outside (-n, n)."""
    _dia_check("dia_check", offsets, n)


def spmv_dia(offsets, data, v: DeviceArray, out: DeviceArray, n: int) -> None:
    """out[i] = sum over the diagonals k, in stored order, with 0 <= i + offsets[k] < n of
    data[k, i + offsets[k]] * v[i + offsets[k]], i < n (k_dia_mult_f64; the plan from CGX_DIA_PLAN).  ``data`` has
    shape (ndiag, ld), ld >= n, scipy's dia_matrix layout.  The offsets come as a host array: they are checked
    (cgx_dia_check) and only then uploaded; slots of ``data`` that hold no entry of A are never read by the kernel."""
    _spmv_dia("spmv_dia", False, offsets, data, v, out, n)


def dia_sym_check(offsets, n: int) -> None:
    """cgx_dia_sym_check (host only, no GPU): raises CgxError(-4) naming the first offset outside [0, n) -- one-sided
    storage holds offsets >= 0, the diagonal -o is the stored diagonal o."""
    _dia_check("dia_sym_check", offsets, n)


def spmv_dia_sym(offsets, data, v: DeviceArray, out: DeviceArray, n: int) -> None:
    """out = A v for the symmetric A whose upper diagonals ``offsets`` (>= 0) / ``data`` hold, scipy's dia_matrix
    layout of triu(A): per stored diagonal k, in stored order, ``data[k, i + o] * v[i + o]`` where o > 0 and
    i + o < n, then ``data[k, i] * v[i - o]`` where i - o >= 0 (k_dia_sym_mult_f64; the plan from CGX_DIA_SYM_PLAN)
    -- the bits of :func:`spmv_dia` on the expansion (o, then -o).  ``data`` has shape (ndiag, ld), ld >= n.  The
    offsets come as a host array: they are checked (cgx_dia_sym_check) and only then uploaded; slots outside
    [o, n) are never read by the kernel."""
    _spmv_dia("spmv_dia_sym", True, offsets, data, v, out, n)


def _from_dia(cls, what: str, setter: str, offsets, data, n, precond, device, flags) -> "Solver":
    """Solver.from_dia / from_dia_sym under the caller's name ``what``; ``setter`` is the kind's set_dia / set_dia_sym."""
    if n is None and data is None and hasattr(offsets, "shape") and hasattr(offsets, "offsets"):
        n = int(offsets.shape[0])
    o, d = _dia_arrays(what, offsets, data)
    n = int(d.shape[1]) if n is None else n
    _need(isinstance(n, (int, np.integer)) and n >= 1, f"{what}: n must be an integer >= 1 (got {n})")
    _need(d.shape[1] >= n, f"{what}: data has {d.shape[1]} columns, n = {n} needed")
    s = cls.csr(int(n), int(o.size) * int(n), device=device, flags=flags)
    try:
        getattr(s, setter)(o, d)
        if precond is not None:
            s.set_precond(precond)
    except Exception:
        s.close()
        raise
    return s


def _set_dia(self, what: str, noun: str, offsets, data) -> None:
    """Solver.set_dia / set_dia_sym under the caller's name ``what`` (cgx_<what> is the C call); ``noun`` is what the
    room is counted in."""
    _need(getattr(self, "csr_nnz", None) is not None, f"{what}: the solver was not created with csr_nnz=")
    _need(getattr(self, "devices", None) is None and getattr(self, "nrhs", None) is None,
          f"{what}: diagonal storage runs on one GPU with one right-hand side (not with devices= or nrhs=)")
    o, d = _dia_arrays(what, offsets, data)
    _need(d.shape[1] >= self.n, f"{what}: data has {d.shape[1]} columns, n = {self.n} needed")
    _need(o.size * self.n <= self.csr_nnz,
          f"{what}: {o.size} {noun} of {self.n} rows are {o.size * self.n} entries, the solver has room for "
          f"{self.csr_nnz}")
    _check(getattr(lib(), f"cgx_{what}")(self._h, int(o.size), _ptr(o) if o.size else None,
                                         _ptr(d) if o.size else None, int(d.shape[1])), f"cgx_{what}")


def bsr_check(indptr, indices, nb: int | None = None) -> None:
    """cgx_bsr_check (host only, no GPU): raises CgxError(-4) naming the first offence of a block structure of
    ``nb`` block rows and ``nb`` block columns (default: ``len(indptr) - 1``)."""
    rp = np.ascontiguousarray(indptr, np.int64)
    ci = np.ascontiguousarray(indices, np.int32)
    _need(rp.ndim == 1 and ci.ndim == 1, "bsr_check: indptr and indices are one-dimensional")
    nb = rp.size - 1 if nb is None else nb
    _need(isinstance(nb, (int, np.integer)) and rp.size == nb + 1,
          f"bsr_check: indptr has {rp.size} entries, nb + 1 = {nb + 1 if isinstance(nb, (int, np.integer)) else nb} needed")
    _check(lib().cgx_bsr_check(int(nb), ci.size, _ptr(rp), _ptr(ci)), "cgx_bsr_check")


def spmv_bsr(indptr, indices, data, v: DeviceArray, out: DeviceArray, nb: int, ncolb: int) -> None:
    """out[I bs + i] = sum over block row I's blocks q, in stored order, and j ascending of
    data[q, i, j] * v[indices[q] bs + j] (k_bsr_mult_f64; the plan from CGX_BSMV_PLAN).  ``data`` has shape
    (nnzb, bs, bs).  The structure comes as host arrays: it is checked (cgx_bsr_check) and only then uploaded, so
    the kernel never sees a block column outside v; the values are re-laid on the device (cgx_bsr_tile_values),
    then multiplied (cgx_spmv_bsr)."""
    rp, ci, va, bs = _bsr_arrays("spmv_bsr", indptr, indices, data)
    _need(isinstance(nb, (int, np.integer)) and isinstance(ncolb, (int, np.integer)) and nb >= 1 and ncolb >= 1,
          "spmv_bsr: need integers nb, ncolb >= 1")
    _need(rp.size == nb + 1, f"spmv_bsr: indptr has {rp.size} entries, nb + 1 = {nb + 1} needed")
    _need(v.dtype == np.float64 and out.dtype == np.float64, "spmv_bsr: float64 only")
    _fits([v], ncolb * bs, "spmv_bsr v")
    _fits([out], nb * bs, "spmv_bsr out")
    L = lib()
    # cgx_bsr_check takes a square block structure: fewer block rows than block columns are padded with empty
    # block rows, so the block columns are checked against ncolb; with more rows than columns they are checked here
    _csr_checked_with(L.cgx_bsr_check, "cgx_bsr_check", "spmv_bsr", rp, ci, nb, ncolb)
    if ci.size == 0:  # nothing to re-lay: one pad tile, so the pointers are real
        va = np.zeros((1, bs, bs))
    nnzb = int(ci.size)
    d_rp, d_ci = DeviceArray.from_host(rp), DeviceArray.from_host(ci if nnzb else np.zeros(1, np.int32))
    d_va, d_t = DeviceArray.from_host(va.reshape(-1)), DeviceArray((max(nnzb, 1) + 63) // 64 * 64 * bs * bs)
    try:
        _check(L.cgx_bsr_tile_values(nnzb, bs, d_va.ptr, d_t.ptr, None), "cgx_bsr_tile_values")
        _check(L.cgx_spmv_bsr(int(nb), int(ncolb), bs, d_rp.ptr, d_ci.ptr, d_t.ptr, v.ptr, out.ptr, None),
               "cgx_spmv_bsr")
        _check(L.cgx_dev_synchronize(), "cgx_dev_synchronize")
    finally:
        for d in (d_rp, d_ci, d_va, d_t):
            d.free()


def _halo_structure(what: str, indptr, indices, nshards):
    """(n, indptr int64, indices int32) of a host-only exchange-plan call."""
    rp = np.ascontiguousarray(indptr, np.int64)
    ci = np.ascontiguousarray(indices, np.int32)
    _need(rp.ndim == 1 and ci.ndim == 1 and rp.size >= 2, f"{what}: indptr needs n + 1 >= 2 entries")
    _need(isinstance(nshards, (int, np.integer)) and not isinstance(nshards, bool),
          f"{what}: nshards must be an integer (got {nshards!r})")
    # the library reads indices[0 .. indptr[n]): a longer claim than the array is caught here
    _need(int(rp[-1]) <= ci.size, f"{what}: indptr[n] = {int(rp[-1])} but {ci.size} indices")
    return rp.size - 1, rp, ci


def csr_halo_counts(indptr, indices, nshards: int) -> np.ndarray:
    """cgx_csr_halo_counts (host only, no GPU): the exchange plan of a CSR structure over ``nshards`` equal row
    blocks, an ``(nshards, nshards)`` int64 array whose entry ``[d, q]`` is how many distinct columns of block q's
    row range occur in block d's rows (0 on the diagonal) -- the entries of p block d pulls from block q per
    iteration.  CgxError(-4) when the structure fails cgx_csr_check or nshards does not divide n."""
    n, rp, ci = _halo_structure("csr_halo_counts", indptr, indices, nshards)
    out = np.zeros((max(int(nshards), 0), max(int(nshards), 0)), np.int64)
    _check(lib().cgx_csr_halo_counts(n, int(nshards), _ptr(rp), _ptr(ci), _ptr(out)), "cgx_csr_halo_counts")
    return out


def csr_halo_list(indptr, indices, nshards: int, dst: int, src: int) -> np.ndarray:
    """cgx_csr_halo_list (host only): the offsets into block ``src`` (column minus src's first row) that block
    ``dst``'s rows name, ascending, each once (int32)."""
    n, rp, ci = _halo_structure("csr_halo_list", indptr, indices, nshards)
    counts = csr_halo_counts(rp, ci, nshards)  # the list's length; raises on a bad structure or partition
    _need(all(isinstance(v, (int, np.integer)) for v in (dst, src)), "csr_halo_list: dst and src must be integers")
    _need(0 <= dst < nshards and 0 <= src < nshards, f"csr_halo_list: blocks ({dst}, {src}) outside [0, {nshards})")
    out = np.empty(int(counts[dst, src]), np.int32)
    _check(lib().cgx_csr_halo_list(n, int(nshards), _ptr(rp), _ptr(ci), int(dst), int(src), _ptr(out)),
           "cgx_csr_halo_list")
    return out


def gather_indexed(src: DeviceArray, idx: DeviceArray, dst: DeviceArray, count: int | None = None) -> None:
    """cgx_gather_indexed (k_gather_indexed alone): ``dst[idx[e]] = src[idx[e]]`` for e < count (float64 arrays,
    int32 ``idx`` with every value once).  The kernel does not range-check, so the indices are read back and
    checked against both arrays here before the launch, and the device is synchronised after it: a call for tests
    of the kernel's result, not one to time (tools/csr_multi_ab.py times the exchange inside a context)."""
    count = idx.count if count is None else int(count)
    _need(src.dtype == np.float64 and dst.dtype == np.float64 and idx.dtype == np.int32,
          "gather_indexed: float64 src and dst, int32 idx")
    _need(0 <= count <= idx.count, f"gather_indexed: count {count} outside [0, {idx.count}]")
    if count == 0:
        return
    ix = idx.to_host()[:count]
    _need(int(ix.min()) >= 0 and int(ix.max()) < min(src.count, dst.count),
          f"gather_indexed: an index outside [0, {min(src.count, dst.count)})")
    _check(lib().cgx_gather_indexed(src.ptr, idx.ptr, count, dst.ptr, None), "cgx_gather_indexed")
    _check(lib().cgx_dev_synchronize(), "cgx_dev_synchronize")


def _block_count(n: int, bs: int) -> int:
    return (n + bs - 1) // bs


def csr_diag_blocks(indptr, indices, data, bs: int) -> np.ndarray:
    """A's ``bs x bs`` diagonal blocks, extracted on the device (k_csr_diag_blocks): an
    ``(nblk, bs, bs)`` array, each entry the sum from +0.0 in stored order of the row's entries in
    that column, +0.0 where there is none.  The structure is checked on the host first."""
    rp, ci, va = _csr_arrays(indptr, indices, data)
    n = rp.size - 1
    _need(n >= 1, "csr_diag_blocks: indptr needs n + 1 >= 2 entries")
    _need(isinstance(bs, (int, np.integer)) and 2 <= bs <= CGX_MAX_PC_BLOCK,
          f"csr_diag_blocks: bs must be in [2, {CGX_MAX_PC_BLOCK}] (got {bs})")
    L = lib()
    _csr_checked("csr_diag_blocks", rp, ci, n, n)
    nblk = _block_count(n, int(bs))
    d_rp, d_ci, d_va = DeviceArray.from_host(rp), DeviceArray.from_host(ci), DeviceArray.from_host(va)
    d_D = DeviceArray(nblk * bs * bs)
    try:
        _check(L.cgx_csr_diag_blocks(n, int(bs), d_rp.ptr, d_ci.ptr, d_va.ptr, d_D.ptr, None), "cgx_csr_diag_blocks")
        return d_D.to_host().reshape(nblk, bs, bs)
    finally:
        for d in (d_rp, d_ci, d_va, d_D):
            d.free()


def precond_block_invert(D: np.ndarray, n: int) -> np.ndarray:
    """cgx_precond_block_invert (host only): the inverses of the ``(nblk, bs, bs)`` diagonal blocks
    of an n-row matrix, by Cholesky from each block's lower triangle; symmetric bit for bit.
    CgxError(-4) names the lowest block with a pivot that is not finite or not > 0."""
    D = np.asarray(D)
    _need(D.dtype == np.float64 and D.ndim == 3 and D.shape[1] == D.shape[2],
          f"precond_block_invert: float64 blocks of shape (nblk, bs, bs) needed (got {D.dtype}, {D.shape})")
    bs = D.shape[1]
    _need(n >= 1 and D.shape[0] == _block_count(n, max(bs, 1)),
          f"precond_block_invert: {D.shape[0]} blocks of {bs} rows do not cover n = {n}")
    W = np.empty_like(D, order="C")
    _check(lib().cgx_precond_block_invert(int(n), int(bs), _ptr(np.ascontiguousarray(D)), _ptr(W)),
           "cgx_precond_block_invert")
    return W


def vecVec(a: DeviceArray, b: DeviceArray, out: DeviceArray, n: int | None = None) -> None:
    """serialConjugate.c:145-155: out[0] = a . b (device scalar)."""
    n = n if n is not None else a.count
    _fits([a, b], n, "vecVec")
    _fits([out], 1, "vecVec out")
    _check(lib().cgx_dot(_dt_flag(a.dtype), n, a.ptr, b.ptr, out.ptr, None), "cgx_dot")


def residual(b, Ax, r, p, rr=None, n=None) -> None:
    """serialConjugate.c:210-212: r = p = b - Ax; rr[0] = r . r."""
    n = n if n is not None else b.count
    _fits([b, Ax, r, p], n, "residual")
    _fits([rr], 1, "residual rr")
    _check(lib().cgx_residual(_dt_flag(b.dtype), n, b.ptr, Ax.ptr, r.ptr, p.ptr,
                              rr.ptr if rr is not None else None, None), "cgx_residual")


def update_xr(x, r, p, Ap, rsold, pAp, rr, n=None) -> None:
    """serialConjugate.c:219-234: alpha = rsold/pAp; x += alpha p; r -= alpha Ap; rr = r.r."""
    n = n if n is not None else x.count
    _fits([x, r, p, Ap], n, "update_xr")
    _fits([rsold, pAp, rr], 1, "update_xr scalars")
    _check(lib().cgx_update_xr(_dt_flag(x.dtype), n, x.ptr, r.ptr, p.ptr, Ap.ptr,
                               rsold.ptr, pAp.ptr, rr.ptr, None), "cgx_update_xr")


def update_p(p, r, rr, rsold, n=None) -> None:
    """serialConjugate.c:239-243: p = r + (rr/rsold) p."""
    n = n if n is not None else p.count
    _fits([p, r], n, "update_p")
    _fits([rr, rsold], 1, "update_p scalars")
    _check(lib().cgx_update_p(_dt_flag(p.dtype), n, p.ptr, r.ptr, rr.ptr, rsold.ptr,
                              None), "cgx_update_p")


# ----------------------------------------------------------------------------
# the solver
# ----------------------------------------------------------------------------
class Solver:
    """A CG context: one GPU, several row-block shards in this process, or one
    rank of a one-process-per-GPU job (RCCL).

    Arrays handed in are cast silently (``np.ascontiguousarray``) to the
    context's types: float32 under CGX_F32_REF, float64 otherwise; under
    CGX_A_F32 A is cast to float32 (a float64 A is rounded to nearest) while
    b and x are cast to float64.

    ``nrhs=K`` (1..CGX_MAX_NRHS; cgx_create_nrhs): K systems on one matrix solved
    together, one read of A per iteration.  b and x arrays then have shape
    ``(K, n)`` (also for K = 1), the vector arguments of ``set_rows`` shape
    ``(K, nrows)``, and ``solve`` / ``get_x`` return ``(K, n)``.

    ``csr_nnz=nnz`` (cgx_create_csr): a sparse A in CSR storage with room for
    ``nnz`` entries, one GPU, fp64; the matrix goes in through :meth:`set_csr`
    (or build the solver with :meth:`from_csr`), b and x through ``set_rows``
    / ``set_x`` / ``fill``.  Several right-hand sides on a CSR matrix
    (cgx_create_csr_nrhs) are spelled ``Solver.csr(n, nnz, nrhs=K)`` or
    ``Solver.from_csr(..., nrhs=K)``; ``Solver(n, csr_nnz=..., nrhs=...)`` raises.  A sparse A over
    several row blocks (cgx_create_csr_multi) is spelled ``Solver.csr(n, nnz, devices=[...])`` or
    ``Solver.from_csr(..., devices=[...])``; ``Solver(n, csr_nnz=..., devices=...)`` raises."""

    def __init__(self, n: int, *, flags: int = CGX_F64, device: int = 0, devices=None,
                 rank: int | None = None, nranks: int | None = None, unique_id: bytes | None = None,
                 poisson_m: int | None = None, nrhs: int | None = None, csr_nnz: int | None = None):
        """Dense n x n system, or (poisson_m=m) the matrix-free 5-point Poisson
        operator on an m x m grid (n must then be m*m or None)."""
        self.nrhs = None
        if nrhs is not None:  # checked before any C call
            _need(devices is None and rank is None and poisson_m is None,
                  "Solver: nrhs runs on one GPU (not with devices=, rank= or poisson_m=)")
            _need(isinstance(nrhs, (int, np.integer)) and 1 <= nrhs <= CGX_MAX_NRHS,
                  f"Solver: nrhs must be in [1, {CGX_MAX_NRHS}] (got {nrhs})")
        self.csr_nnz = None
        if csr_nnz is not None:  # checked before any C call
            _need(devices is None and rank is None and poisson_m is None and nrhs is None,
                  "Solver: csr_nnz runs on one GPU (not with devices=, rank=, poisson_m= or nrhs=)")
            _need(isinstance(csr_nnz, (int, np.integer)) and csr_nnz >= 0,
                  f"Solver: csr_nnz must be an integer >= 0 (got {csr_nnz})")
        L = lib()
        self.poisson_m = poisson_m
        if poisson_m is not None:
            n = poisson_m * poisson_m
        self.n = int(n)
        self.flags = flags
        self.dtype = _dtype(flags)
        h = ctypes.c_void_p()
        if poisson_m is not None:
            if rank is not None:
                u = UniqueId()
                ctypes.memmove(ctypes.addressof(u), unique_id, 128)
                rc = L.cgx_create_poisson_rank(ctypes.byref(h), poisson_m, rank, nranks, ctypes.byref(u), device, flags)
            elif devices is not None:
                arr = (ctypes.c_int * len(devices))(*devices)
                rc = L.cgx_create_poisson_multi(ctypes.byref(h), poisson_m, len(devices), arr, flags)
            else:
                rc = L.cgx_create_poisson(ctypes.byref(h), poisson_m, device, flags)
        elif rank is not None:
            u = UniqueId()
            if unique_id is None or len(unique_id) != 128:
                raise ValueError("unique_id must be the 128 bytes from get_unique_id()")
            ctypes.memmove(ctypes.addressof(u), unique_id, 128)
            rc = L.cgx_create_rank(ctypes.byref(h), self.n, rank, nranks, ctypes.byref(u), device, flags)
        elif devices is not None:
            arr = (ctypes.c_int * len(devices))(*devices)
            rc = L.cgx_create_multi(ctypes.byref(h), self.n, len(devices), arr, flags)
        elif nrhs is not None:
            rc = L.cgx_create_nrhs(ctypes.byref(h), self.n, int(nrhs), device, flags)
            self.nrhs = int(nrhs) if rc == 0 else None
        elif csr_nnz is not None:
            rc = L.cgx_create_csr(ctypes.byref(h), self.n, int(csr_nnz), device, flags)
            self.csr_nnz = int(csr_nnz) if rc == 0 else None
        else:
            rc = L.cgx_create(ctypes.byref(h), self.n, device, flags)
        _check(rc, "cgx_create_nrhs" if nrhs is not None else "cgx_create_csr" if csr_nnz is not None else "cgx_create")
        self._h = h.value

    @classmethod
    def csr(cls, n: int, nnz: int, *, nrhs: int | None = None, device: int = 0, flags: int = CGX_F64,
            devices=None) -> "Solver":
        """An empty CSR solver with room for ``nnz`` entries (the matrix goes in through
        :meth:`set_csr`).  ``nrhs=K`` (cgx_create_csr_nrhs): K systems on the one matrix solved
        together, one read of the CSR arrays per iteration; b and x are then ``(K, n)`` arrays as
        on a dense ``nrhs`` solver.  ``devices=[...]`` (cgx_create_csr_multi): ``len(devices)`` equal
        row blocks in this process, one per listed device (a device may repeat), every block with
        room for ``nnz`` entries -- a safe bound; not with ``nrhs``.  Without either it is
        ``Solver(n, csr_nnz=nnz)``."""
        if devices is not None:  # checked before any C call
            _need(nrhs is None, "Solver.csr: several right-hand sides run on one GPU (not with devices=)")
            _need(device == 0, "Solver.csr: devices= lists every block's device (not with device=)")
            devs = [int(d) for d in devices]
            _need(isinstance(nnz, (int, np.integer)) and nnz >= 0,
                  f"Solver.csr: nnz must be an integer >= 0 (got {nnz})")
            _need(isinstance(n, (int, np.integer)) and n >= 1, f"Solver.csr: n must be an integer >= 1 (got {n})")
            h = ctypes.c_void_p()
            arr = (ctypes.c_int * max(len(devs), 1))(*devs)
            rc = lib().cgx_create_csr_multi(ctypes.byref(h), int(n), int(nnz), len(devs), arr, flags)
            _check(rc, "cgx_create_csr_multi")
            s = cls.__new__(cls)  # the fields __init__ sets
            s.nrhs, s.csr_nnz, s.poisson_m, s.devices = None, int(nnz), None, devs
            s.n, s.flags, s.dtype = int(n), flags, _dtype(flags)
            s._h = h.value
            return s
        if nrhs is None:
            return cls(n, flags=flags, device=device, csr_nnz=nnz)
        _need(isinstance(nrhs, (int, np.integer)) and 1 <= nrhs <= CGX_MAX_NRHS,
              f"Solver.csr: nrhs must be in [1, {CGX_MAX_NRHS}] (got {nrhs})")
        _need(isinstance(nnz, (int, np.integer)) and nnz >= 0, f"Solver.csr: nnz must be an integer >= 0 (got {nnz})")
        _need(isinstance(n, (int, np.integer)) and n >= 1, f"Solver.csr: n must be an integer >= 1 (got {n})")
        h = ctypes.c_void_p()
        rc = lib().cgx_create_csr_nrhs(ctypes.byref(h), int(n), int(nnz), int(nrhs), device, flags)
        _check(rc, "cgx_create_csr_nrhs")
        s = cls.__new__(cls)  # the fields __init__ sets
        s.nrhs, s.csr_nnz, s.poisson_m = int(nrhs), int(nnz), None
        s.n, s.flags, s.dtype = int(n), flags, _dtype(flags)
        s._h = h.value
        return s

    @classmethod
    def from_csr(cls, indptr, indices=None, data=None, *, device: int = 0, flags: int = CGX_F64,
                 precond=None, nrhs: int | None = None, a_f32: bool = False, devices=None) -> "Solver":
        """A CSR solver sized for this matrix, with the matrix set (b = 0, x0 = 0)
        and, with ``precond`` ("jacobi", an array or ``("block", bs)``), its preconditioner (:meth:`set_precond`).
        ``nrhs=K``: K systems on the matrix solved together (:meth:`csr`; no preconditioner).
        ``a_f32=True``: float-stored values (:meth:`set_csr`).
        ``devices=[...]``: equal row blocks over the listed devices (:meth:`csr`), each with room for the
        largest block's entries; no preconditioner and no ``nrhs``."""
        a_f32 = _a_f32_flag("from_csr", a_f32)
        rp, ci, va = _csr_arrays(indptr, indices, data, a_f32)
        _need(rp.size >= 2, "from_csr: indptr needs n + 1 >= 2 entries")
        _need(nrhs is None or precond is None, "from_csr: no preconditioner with several right-hand sides")
        nnz = int(ci.size)
        if devices is not None:  # checked before any C call
            _need(nrhs is None and precond is None,
                  "from_csr: row blocks (devices=) take no preconditioner and one right-hand side")
            P, n = len(devices), rp.size - 1
            if P >= 1 and n % P == 0:  # the largest block's exact count; any other partition the library refuses
                nnz = int(np.max(np.diff(rp[::n // P]), initial=0))
                nnz = max(nnz, 0)
        s = cls.csr(rp.size - 1, nnz, nrhs=nrhs, device=device, flags=flags, devices=devices)
        try:
            s.set_csr(rp, ci, va, a_f32=a_f32)
            if precond is not None:
                s.set_precond(precond)
        except Exception:
            s.close()
            raise
        return s

    def set_csr(self, indptr, indices=None, data=None, *, a_f32: bool = False) -> None:
        """cgx_set_csr: the matrix of a ``csr_nnz`` solver from host arrays (cast
        to int64 / int32 / float64).  The structure is checked before anything is
        uploaded: CgxError(-4) names the first offence and the earlier matrix stays.
        ``a_f32=True`` (cgx_set_csr_f32): data is cast to float32 (float64 rounds to
        nearest) and stays float32 on the device, 8 bytes per entry streamed in
        place of 12; all arithmetic is fp64 on the exactly widened values, so the
        solver gives the bits it gives for ``data.astype(float32).astype(float64)``.
        ``info().flags`` carries CGX_A_F32 until the next ``set_csr`` without it."""
        a_f32 = _a_f32_flag("set_csr", a_f32)
        _need(getattr(self, "csr_nnz", None) is not None, "set_csr: the solver was not created with csr_nnz=")
        rp, ci, va = _csr_arrays(indptr, indices, data, a_f32)
        _need(rp.size == self.n + 1, f"set_csr: indptr has {rp.size} entries, n + 1 = {self.n + 1} needed")
        if getattr(self, "devices", None) is None:  # row blocks: the room is per block, and the library checks it
            _need(ci.size <= self.csr_nnz, f"set_csr: {ci.size} entries, the solver has room for {self.csr_nnz}")
        else:
            _need(int(rp[-1]) <= ci.size, f"set_csr: indptr[n] = {int(rp[-1])} but {ci.size} indices")
        if a_f32:
            _check(lib().cgx_set_csr_f32(self._h, _ptr(rp), _ptr(ci), _ptr(va)), "cgx_set_csr_f32")
        else:
            _check(lib().cgx_set_csr(self._h, _ptr(rp), _ptr(ci), _ptr(va)), "cgx_set_csr")

    @classmethod
    def from_bsr(cls, indptr, indices=None, data=None, *, precond=None, device: int = 0,
                 flags: int = CGX_F64) -> "Solver":
        """A CSR solver sized for this block matrix (room for nnzb * bs * bs entries), with the matrix set through
        :meth:`set_bsr` (b = 0, x0 = 0) and, with ``precond`` ("jacobi", an array or ``("block", pbs)``), its
        preconditioner (:meth:`set_precond`).  ``data`` has shape (nnzb, bs, bs); or pass one object with
        ``.indptr / .indices / .data`` such as scipy's bsr_matrix."""
        rp, ci, va, bs = _bsr_arrays("from_bsr", indptr, indices, data)
        _need(rp.size >= 2, "from_bsr: indptr needs nb + 1 >= 2 entries")
        s = cls.csr((rp.size - 1) * bs, int(ci.size) * bs * bs, device=device, flags=flags)
        try:
            s.set_bsr(rp, ci, va)
            if precond is not None:
                s.set_precond(precond)
        except Exception:
            s.close()
            raise
        return s

    def set_bsr(self, indptr, indices=None, data=None) -> None:
        """cgx_set_bsr: the matrix of a ``csr_nnz`` solver as dense ``bs x bs`` blocks, scipy's bsr_matrix layout
        (``data`` of shape (nnzb, bs, bs), 2 <= bs <= 8, n = nb bs; or one object with
        ``.indptr / .indices / .data``), multiplied by the block kernel k_bsr_mult_f64.  The structure is checked
        before anything is uploaded: CgxError(-4) names the first offence and the earlier matrix stays.  The solver
        is block-valued (``info().flags`` carries CGX_BSR_ACTIVE) until the next :meth:`set_csr`; preconditioning
        is off afterwards, as after ``set_csr``.  One GPU, one right-hand side, float64 values."""
        _need(getattr(self, "csr_nnz", None) is not None, "set_bsr: the solver was not created with csr_nnz=")
        _need(getattr(self, "devices", None) is None and getattr(self, "nrhs", None) is None,
              "set_bsr: block storage runs on one GPU with one right-hand side (not with devices= or nrhs=)")
        rp, ci, va, bs = _bsr_arrays("set_bsr", indptr, indices, data)
        _need(self.n % bs == 0, f"set_bsr: n = {self.n} is not divisible by bs = {bs}")
        nb = self.n // bs
        _need(rp.size == nb + 1, f"set_bsr: indptr has {rp.size} entries, n / bs + 1 = {nb + 1} needed")
        _need(ci.size * bs * bs <= self.csr_nnz,
              f"set_bsr: {ci.size} blocks of {bs} x {bs} are {ci.size * bs * bs} entries, the solver has room for "
              f"{self.csr_nnz}")
        _check(lib().cgx_set_bsr(self._h, bs, _ptr(rp), _ptr(ci), _ptr(va)), "cgx_set_bsr")

    @classmethod
    def from_dia(cls, offsets, data=None, *, n: int | None = None, precond=None, device: int = 0,
                 flags: int = CGX_F64) -> "Solver":
        """A CSR solver sized for this matrix held by diagonals (room for ndiag * n entries), with the matrix set
        through :meth:`set_dia` (b = 0, x0 = 0) and, with ``precond`` ("jacobi", an array or ``("block", pbs)``),
        its preconditioner (:meth:`set_precond`).  ``data`` has shape (ndiag, ld); or pass one object with
        ``.offsets / .data`` such as scipy's dia_matrix.  ``n`` defaults to the object's ``shape[0]``, else to ld."""
        return _from_dia(cls, "from_dia", "set_dia", offsets, data, n, precond, device, flags)

    def set_dia(self, offsets, data=None) -> None:
        """cgx_set_dia: the matrix of a ``csr_nnz`` solver held by diagonals, scipy's dia_matrix layout (``data`` of
        shape (ndiag, ld), ld >= n, ``data[k, j] = A[j - offsets[k], j]``; or one object with ``.offsets / .data``),
        multiplied by the gather-free kernel k_dia_mult_f64.  Slots that hold no entry of A are never read and may
        hold NaN.  The offsets are checked before anything is uploaded: CgxError(-4) names the first offence and the
        earlier matrix stays.  The solver is diagonal-valued (``info().flags`` carries CGX_DIA_ACTIVE) until the
        next :meth:`set_csr` / :meth:`set_bsr`; preconditioning is off afterwards, as after ``set_csr``.  One GPU,
        one right-hand side, float64 values."""
        _set_dia(self, "set_dia", "diagonals", offsets, data)

    @classmethod
    def from_dia_sym(cls, offsets, data=None, *, n: int | None = None, precond=None, device: int = 0,
                     flags: int = CGX_F64) -> "Solver":
        """A CSR solver sized for this symmetric matrix held by its upper diagonals (room for ndiag * n entries, the
        stored count), with the matrix set through :meth:`set_dia_sym` (b = 0, x0 = 0) and, with ``precond``, its
        preconditioner (:meth:`set_precond`).  Arguments as :meth:`from_dia`'s."""
        return _from_dia(cls, "from_dia_sym", "set_dia_sym", offsets, data, n, precond, device, flags)

    def set_dia_sym(self, offsets, data=None) -> None:
        """cgx_set_dia_sym: the symmetric matrix of a ``csr_nnz`` solver held by the diagonals of its upper triangle,
        scipy's dia_matrix layout of triu(A) (offsets >= 0, ``data`` of shape (ndiag, ld), ld >= n,
        ``data[k, j] = A[j - offsets[k], j]`` for j in [offsets[k], n); or one object with ``.offsets / .data``).  The
        stored diagonal o > 0 also stands for the diagonal -o; the one-sided kernel k_dia_sym_mult_f64 reads each
        value once for both.  Symmetry cannot be checked: only one triangle is given.  Slots outside
        [offsets[k], n) are never read and may hold NaN.  The offsets are checked before anything is uploaded:
        CgxError(-4) names the first offence and the earlier matrix stays.  The solver is one-sided
        (``info().flags`` carries CGX_DIA_SYM_ACTIVE | CGX_DIA_ACTIVE) until the next :meth:`set_csr` /
        :meth:`set_bsr` / :meth:`set_dia`; preconditioning is off afterwards.  One GPU, one right-hand side,
        float64 values."""
        _set_dia(self, "set_dia_sym", "stored diagonals", offsets, data)

    def csr_halo(self) -> np.ndarray:
        """cgx_get_csr_halo: the ``(nshards, nshards)`` exchange counts in use on a CSR solver over row blocks
        (``devices=``) -- entry ``[d, q]`` is how many entries of p block d pulls from block q per iteration;
        :func:`csr_halo_counts` of the matrix that was set.  CgxError(-6) before the first :meth:`set_csr`,
        CgxError(-1) on any other solver."""
        P = len(getattr(self, "devices", None) or [0])
        out = np.zeros((P, P), np.int64)
        _check(lib().cgx_get_csr_halo(self._h, _ptr(out)), "cgx_get_csr_halo")
        return out

    def set_precond(self, precond) -> None:
        """Diagonal preconditioning of a ``csr_nnz`` solver: ``"jacobi"`` (1 / diag(A),
        taken from the matrix on the device; CgxError(-4) names the lowest row whose
        diagonal is missing, not finite or not > 0, and nothing changes), ``None``
        (off), or an array of n positive float64 values (cgx_set_precond_diag).
        ``("block", bs)`` is :meth:`set_precond_block` with that block size.
        Ends a solve in progress; :meth:`set_csr` turns it off again."""
        L = lib()
        if precond is None:
            _check(L.cgx_set_precond(self._h, PRECOND_KINDS["none"]), "cgx_set_precond")
        elif isinstance(precond, tuple) and len(precond) == 2 and precond[0] == "block":
            self.set_precond_block(precond[1])  # ("block", bs): block Jacobi
        elif isinstance(precond, str):
            _need(precond == "jacobi", f'set_precond: "jacobi", None or an array (got {precond!r})')
            _check(L.cgx_set_precond(self._h, PRECOND_KINDS["jacobi"]), "cgx_set_precond")
        else:
            m = np.asarray(precond)
            _need(m.dtype == np.float64, f"set_precond: the values must be float64 (got {m.dtype})")
            _need(m.shape == (self.n,), f"set_precond: {m.shape} values, ({self.n},) needed")
            _check(L.cgx_set_precond_diag(self._h, _ptr(np.ascontiguousarray(m))), "cgx_set_precond_diag")

    @property
    def precond(self) -> str:
        """"none", "jacobi", "diag" or "block" ("none" on every solver that is not a CSR one)."""
        k = ctypes.c_int(0)
        _check(lib().cgx_get_precond(self._h, ctypes.byref(k)), "cgx_get_precond")
        if k.value == PC_BLOCK:
            return "block"
        return next(name for name, kind in PRECOND_KINDS.items() if kind == k.value)

    def precond_diag(self) -> np.ndarray:
        """The n values of M^-1 in use (CgxError(-6) when preconditioning is off or block Jacobi)."""
        out = np.empty(self.n, np.float64)
        _check(lib().cgx_get_precond_diag(self._h, _ptr(out)), "cgx_get_precond_diag")
        return out

    def set_precond_block(self, bs: int, values=None) -> None:
        """Block-Jacobi preconditioning of a ``csr_nnz`` solver: M^-1 = the inverses of the
        matrix's ``bs x bs`` diagonal blocks (2 <= bs <= 8; the last block is smaller when bs does
        not divide n), extracted on the device and inverted on the host by Cholesky.  CgxError(-4)
        names the lowest block that is not positive definite, and nothing changes.  ``values``: the
        caller's inverse blocks instead, float64 of shape (ceil(n / bs), bs, bs); they are checked
        (finite, diagonal > 0), their symmetry and definiteness are the caller's business.
        Ends a solve in progress; :meth:`set_csr` turns it off again."""
        _need(isinstance(bs, (int, np.integer)) and not isinstance(bs, bool),
              f"set_precond_block: bs must be an integer (got {bs!r})")
        L = lib()
        if values is None:
            _check(L.cgx_set_precond_block(self._h, int(bs)), "cgx_set_precond_block")
            return
        w = np.asarray(values)
        _need(w.dtype == np.float64, f"set_precond_block: the values must be float64 (got {w.dtype})")
        if 2 <= bs <= CGX_MAX_PC_BLOCK:  # any other bs: the library refuses it before it reads the values
            shape = (_block_count(self.n, int(bs)), int(bs), int(bs))
            _need(w.shape == shape, f"set_precond_block: values of shape {w.shape}, {shape} needed")
        _check(L.cgx_set_precond_block_values(self._h, int(bs), _ptr(np.ascontiguousarray(w))),
               "cgx_set_precond_block_values")

    @property
    def precond_block(self) -> tuple:
        """(bs, W): the block size and the (nblk, bs, bs) inverse blocks in use; the unused rows
        and columns of a short last block are +0.0 (CgxError(-6) unless :attr:`precond` is "block")."""
        L = lib()
        b = ctypes.c_int(0)
        _check(L.cgx_get_precond_block(self._h, ctypes.byref(b), None), "cgx_get_precond_block")
        W = np.empty((_block_count(self.n, b.value), b.value, b.value), np.float64)
        _check(L.cgx_get_precond_block(self._h, ctypes.byref(b), _ptr(W)), "cgx_get_precond_block")
        return b.value, W

    def _vshape(self, rows: int | None = None) -> tuple:
        """The shape of a b or x argument: (n,), or (nrhs, n) on an nrhs context."""
        k = getattr(self, "nrhs", None)
        m = self.n if rows is None else rows
        return (m,) if k is None else (k, m)

    # lifetime
    def close(self) -> None:
        """cgx_destroy.  In rank mode it first drains the streams with the RCCL
        deadline; an error there (a peer died) is raised after the free."""
        if getattr(self, "_h", None):
            rc = lib().cgx_destroy(self._h)
            self._h = None
            _check(rc, "cgx_destroy")

    def __enter__(self):
        return self

    def __exit__(self, exc_type, *exc):
        if exc_type is None:
            self.close()
        else:  # keep the original error; the free still happens
            try:
                self.close()
            except CgxError:
                pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def info(self) -> Info:
        i = Info()
        _check(lib().cgx_get_info(self._h, ctypes.byref(i)), "cgx_get_info")
        return i

    # data
    def set_system(self, A: np.ndarray, b: np.ndarray, x0: np.ndarray | None = None) -> None:
        A = np.ascontiguousarray(A, _a_dtype(self.flags))
        b = np.ascontiguousarray(b, self.dtype)
        vs = self._vshape()
        x0 = np.zeros(vs, self.dtype) if x0 is None else np.ascontiguousarray(x0, self.dtype)
        _need(A.shape == (self.n, self.n), f"set_system: A has shape {A.shape}, ({self.n}, {self.n}) needed")
        _need(b.shape == vs, f"set_system: b has shape {b.shape}, {vs} needed")
        _need(x0.shape == vs, f"set_system: x0 has shape {x0.shape}, {vs} needed")
        _check(lib().cgx_set_system(self._h, _ptr(A), _ptr(b), _ptr(x0)), "cgx_set_system")

    def set_rows(self, row0: int, A_rows=None, b_rows=None, x_rows=None) -> None:
        arrs = [None if a is None else np.ascontiguousarray(a, dt)
                for a, dt in zip((A_rows, b_rows, x_rows), (_a_dtype(self.flags), self.dtype, self.dtype))]
        _need(any(a is not None for a in arrs), "set_rows: nothing to set")
        k = getattr(self, "nrhs", None)
        if k is not None:  # the vectors: (nrhs, nrows), system after system
            for a, name in zip(arrs[1:], ("b_rows", "x_rows")):
                if a is not None:
                    _need(a.ndim == 2 and a.shape[0] == k,
                          f"set_rows: {name} has shape {a.shape}, ({k}, nrows) needed")
            nrows = arrs[0].shape[0] if arrs[0] is not None else next(a.shape[1] for a in arrs[1:] if a is not None)
            if arrs[0] is not None:
                _need(arrs[0].ndim == 2 and arrs[0].shape[1] >= self.n,
                      f"set_rows: A_rows has shape {arrs[0].shape}, (nrows, >= {self.n}) needed")
            for a, name in zip(arrs[1:], ("b_rows", "x_rows")):
                if a is not None:
                    _need(a.shape[1] == nrows,
                          f"set_rows: {name} has shape {a.shape}; every argument needs the same {nrows} rows")
            _need(0 <= row0 and row0 + nrows <= self.n,
                  f"set_rows: rows [{row0}, {row0 + nrows}) outside [0, {self.n})")
            lda = arrs[0].shape[1] if arrs[0] is not None else self.n
            _check(lib().cgx_set_rows(self._h, row0, nrows, None if arrs[0] is None else _ptr(arrs[0]), lda,
                                      *(None if a is None else _ptr(a) for a in arrs[1:])), "cgx_set_rows")
            return
        nrows = next(a.shape[0] for a in arrs if a is not None)
        if arrs[0] is not None:
            _need(arrs[0].ndim == 2 and arrs[0].shape[1] >= self.n,
                  f"set_rows: A_rows has shape {arrs[0].shape}, (nrows, >= {self.n}) needed")
        for a, name in zip(arrs, ("A_rows", "b_rows", "x_rows")):
            if a is not None:
                _need(a.shape[0] == nrows and (a.ndim == 2 if name == "A_rows" else a.ndim == 1),
                      f"set_rows: {name} has shape {a.shape}; every argument needs the same {nrows} rows")
        _need(0 <= row0 and row0 + nrows <= self.n, f"set_rows: rows [{row0}, {row0 + nrows}) outside [0, {self.n})")
        lda = arrs[0].shape[1] if arrs[0] is not None else self.n
        _check(lib().cgx_set_rows(self._h, row0, nrows, *(None if a is None else _ptr(a) for a in arrs[:1]), lda,
                                  *(None if a is None else _ptr(a) for a in arrs[1:])), "cgx_set_rows")

    def fill(self, b_value: float, x_value: float = 0.0) -> None:
        _check(lib().cgx_fill(self._h, b_value, x_value), "cgx_fill")

    def generate_spd(self, seed: int = 42) -> None:
        _check(lib().cgx_generate_spd(self._h, seed), "cgx_generate_spd")

    def get_x(self) -> np.ndarray:
        x = np.empty(self._vshape(), self.dtype)
        _check(lib().cgx_get_x(self._h, _ptr(x)), "cgx_get_x")
        return x

    def set_x(self, x: np.ndarray) -> None:
        x = np.ascontiguousarray(x, self.dtype)
        _need(x.shape == self._vshape(), f"set_x: x has shape {x.shape}, {self._vshape()} needed")
        _check(lib().cgx_set_x(self._h, _ptr(x)), "cgx_set_x")

    # solve
    def solve(self, x0: np.ndarray | None = None, eps: float = 1e-6, max_iter: int = -1) -> tuple[np.ndarray, Stats]:
        st = Stats()
        if x0 is not None:
            x = np.array(x0, dtype=self.dtype, copy=True)
            _need(x.shape == self._vshape(), f"solve: x0 has shape {x.shape}, {self._vshape()} needed")
            _check(lib().cgx_solve(self._h, _ptr(x), eps, max_iter, ctypes.byref(st)), "cgx_solve")
        else:
            _check(lib().cgx_solve(self._h, None, eps, max_iter, ctypes.byref(st)), "cgx_solve")
            x = self.get_x()
        return x, st

    def begin(self) -> None:
        _check(lib().cgx_solve_begin(self._h), "cgx_solve_begin")

    def iterate(self, count: int, eps: float = -1.0) -> tuple[int, bool]:
        done = ctypes.c_int64(0)
        conv = ctypes.c_int(0)
        _check(lib().cgx_iterate(self._h, count, eps, ctypes.byref(done), ctypes.byref(conv)), "cgx_iterate")
        return done.value, bool(conv.value)

    def stats(self) -> Stats:
        st = Stats()
        _check(lib().cgx_get_stats(self._h, ctypes.byref(st)), "cgx_get_stats")
        return st

    def stats_rhs(self, j: int) -> Stats:
        """System j's iterations, converged and rr of the last solve (nrhs contexts; j = 0 otherwise)."""
        k = getattr(self, "nrhs", None) or 1
        _need(0 <= j < k, f"stats_rhs: system {j} not in [0, {k})")
        st = Stats()
        _check(lib().cgx_get_stats_rhs(self._h, j, ctypes.byref(st)), "cgx_get_stats_rhs")
        return st

    def residual_norms(self) -> tuple[np.ndarray, np.ndarray]:
        """(||b_j - A x_j||, ||b_j||) per system for the current x (ends a solve in progress)."""
        k = getattr(self, "nrhs", None) or 1
        rn, bn = np.zeros(k), np.zeros(k)
        pd = ctypes.POINTER(ctypes.c_double)
        _check(lib().cgx_residual_norms(self._h, rn.ctypes.data_as(pd), bn.ctypes.data_as(pd)), "cgx_residual_norms")
        return rn, bn

    def residual_norm(self) -> tuple[float, float]:
        """(||b - A x||, ||b||) for the current x (ends a solve in progress)."""
        rn, bn = ctypes.c_double(), ctypes.c_double()
        _check(lib().cgx_residual_norm(self._h, ctypes.byref(rn), ctypes.byref(bn)), "cgx_residual_norm")
        return rn.value, bn.value

    def set_matvec_plan(self, rows_per_wave: int, chunks_in_flight: int, nontemporal: int = 1,
                        blocks_per_cu: int = 0) -> None:
        _check(lib().cgx_set_matvec_plan(self._h, rows_per_wave, chunks_in_flight, nontemporal, blocks_per_cu),
               "cgx_set_matvec_plan")

    def matvec_plan(self) -> dict:
        v = [ctypes.c_int() for _ in range(4)]
        _check(lib().cgx_get_matvec_plan(self._h, *(ctypes.byref(x) for x in v)), "cgx_get_matvec_plan")
        return dict(zip(("R", "U", "nt", "blocks"), (x.value for x in v)))

    def phase_times(self) -> dict:
        """CGX_PHASES: {phase: {"median_us", "mean_us", "samples"}} since the last reset_timing()."""
        t = PhaseTimes()
        _check(lib().cgx_get_phase_times(self._h, ctypes.byref(t)), "cgx_get_phase_times")
        return {name: {"median_us": t.median_us[i], "mean_us": t.mean_us[i], "samples": int(t.samples[i])}
                for i, name in enumerate(PHASE_NAMES)}

    def comm_info(self) -> dict:
        """What the exchange runs on: RCCL's rank count / device / rank (rank mode) and the PCI bus id."""
        ci = CommInfo()
        _check(lib().cgx_get_comm_info(self._h, ctypes.byref(ci)), "cgx_get_comm_info")
        return {"rccl_nranks": ci.rccl_nranks, "rccl_device": ci.rccl_device, "rccl_rank": ci.rccl_rank,
                "device": ci.device, "pci_bus_id": ci.pci_bus_id.decode()}

    def overlap_info(self) -> dict:
        """How the p exchange was chosen at creation (aligned row blocks,
        cgx_get_overlap_info): both whole forms, exchange + matVec, timed end
        to end; the overlapped one runs when overlap_form_us < (1 - margin) *
        plain_form_us.  The parts (allgather alone, the split, the one
        launch) are reported too.  Values as the library decided on them (not
        rounded); None where not measured."""
        o = OverlapInfo()
        _check(lib().cgx_get_overlap_info(self._h, ctypes.byref(o)), "cgx_get_overlap_info")
        r = lambda v: None if v < 0 else float(v)  # noqa: E731
        return {"on": bool(o.active), "decided_by": OVERLAP_DECIDED_BY.get(o.decided_by, str(o.decided_by)),
                "overlap_form_us": r(o.overlap_form_us), "plain_form_us": r(o.plain_form_us), "margin": o.margin,
                "forms_ms": r(o.forms_ms),
                "allgather_us": r(o.allgather_us), "split_cost_us": r(o.split_cost_us), "split_us": r(o.split_us),
                "one_launch_us": r(o.one_launch_us)}

    def reset_timing(self) -> None:
        _check(lib().cgx_reset_timing(self._h), "cgx_reset_timing")

    def synchronize(self) -> None:
        _check(lib().cgx_synchronize(self._h), "cgx_synchronize")


def conjugrad(A: np.ndarray, b: np.ndarray, x: np.ndarray, *, eps: float = 1e-6, max_iter: int = -1,
              flags: int | None = None, shards=None) -> Stats:
    """serialConjugate.c:180-259 ``conjugrad(A, b, x)``: solves in place (x is
    x0 on entry, the solution on exit).  ``shards`` = list of device ids gives
    parallel_cg.c's row-block split with P = len(shards) (parallel_cg.c:248).
    The dtype of ``x`` picks the arithmetic unless ``flags`` is given:
    float32 -> CGX_F32_REF (the reference's float results bit for bit),
    float64 -> CGX_F64, or CGX_A_F32 when ``A`` is float32 (A stays float on
    the GPU, fp64 arithmetic)."""
    if flags is None:
        flags = CGX_F32_REF if x.dtype == np.float32 else CGX_F64
        if x.dtype == np.float64 and getattr(A, "dtype", None) == np.float32 and shards is None:
            flags = CGX_A_F32
    n = b.shape[0]
    with Solver(n, flags=flags, devices=shards) as s:
        s.set_system(A, b, x)
        xs, st = s.solve(None, eps=eps, max_iter=max_iter)
    x[...] = xs
    return st
