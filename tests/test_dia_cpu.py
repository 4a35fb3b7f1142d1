"""cgx_set_dia without a GPU: the CPU statement of k_dia_mult_f64's summation order (tests/_dia_order.py), the offset
check, the Python mirror's own checks, and the probe bars the GPU test rests on."""
import numpy as np
import pytest

import _dia_order as do
import _nrhs_probe as npr
import _pcg_probe as pp
import conjugate_gradient_amd as cg
from _spmv_order import fma

ERR_ARG, ERR_SHAPE = -1, -4
# None on a tree without the feature: every test then fails at its first use
DIA_ACTIVE = getattr(cg, "CGX_DIA_ACTIVE", None)
dia_check = getattr(cg, "dia_check", None)


@pytest.fixture(scope="module")
def L(built):
    assert hasattr(cg.Solver, "set_dia"), "the package has no diagonal storage"
    return cg.lib()


def _p(a):
    return a.ctypes.data


def _err(L):
    return L.cgx_last_error().decode()


# ---- the emulation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndiag", do.STRUCT_NDIAGS)
def test_emulation_agrees_with_a_dense_product(ndiag):
    offsets, data, v = do.structure_matrix(ndiag)
    assert data.shape == (ndiag, do.STRUCT_LD)
    A = do.dense(offsets, data, do.STRUCT_N)
    assert np.isfinite(A).all()  # no unused slot reached the matrix
    out = do.spmv_dia(offsets, data, v)
    assert out.shape == (do.STRUCT_N,) and np.isfinite(out).all()
    assert np.allclose(out, A @ v, rtol=0, atol=1e-13 * max(1, ndiag))
    if ndiag == 0:
        assert np.array_equal(out, np.zeros(do.STRUCT_N)) and not np.signbit(out).any()


def test_structure_matrix_holds_nan_in_every_unused_slot():
    offsets, data, _ = do.structure_matrix()
    n = do.STRUCT_N
    for k, o in enumerate(offsets):
        lo, hi = do.in_range(int(o), n)
        assert np.isnan(data[k, :lo]).all() and np.isnan(data[k, hi:]).all() and np.isfinite(data[k, lo:hi]).all()
    assert np.count_nonzero(data == 0.0) >= 5  # stored zeros among the entries


def test_one_diagonal_is_one_fma_per_row():
    """Offset 0 alone: each row is fma(d_i, v_i, +0.0) = the rounded product."""
    offsets, data, v = do.structure_matrix(1)
    assert list(offsets) == [0]
    want = np.array([fma(float(data[0, i]), float(v[i]), 0.0) for i in range(do.STRUCT_N)])
    assert np.array_equal(do.spmv_dia(offsets, data, v), want)


@pytest.mark.parametrize("mutation", do.MUTATIONS)
def test_mutations_change_bits(mutation):
    offsets, data, v = do.structure_matrix()
    good, bad = do.spmv_dia(offsets, data, v), do.spmv_dia(offsets, data, v, mutation=mutation)
    assert np.isfinite(bad).all() and not np.array_equal(good, bad), mutation


def test_expansion_round_trips_through_dense():
    offsets, data, _ = do.structure_matrix()
    n = do.STRUCT_N
    rp, ci, va = do.expand(offsets, data, n)
    assert rp.size == n + 1 and rp[-1] == sum(n - abs(int(o)) for o in offsets) and np.isfinite(va).all()
    A = np.zeros((n, n))
    np.add.at(A, (np.repeat(np.arange(n), np.diff(rp)), ci), va)
    assert np.array_equal(A, do.dense(offsets, data, n))
    # row 0 lists its entries diagonal after diagonal in stored order
    want0 = [int(o) for o in offsets if 0 <= int(o) < n]
    assert list(ci[rp[0]:rp[1]]) == want0
    # from_dense: the diagonals that hold a nonzero, ascending, and the same matrix
    o2, d2 = do.from_dense(A)
    assert np.all(np.diff(o2) > 0) and np.array_equal(do.dense(o2, d2, n), A)
    o3, d3 = do.from_csr(rp, ci, va, n)
    assert np.array_equal(o3, o2) and np.allclose(d3, d2, rtol=0, atol=1e-15)
    assert do.expand(np.zeros(0, np.int32), np.zeros((0, n)), n)[0].tolist() == [0] * (n + 1)


def test_vectorised_form_is_the_emulation():
    n = 211
    offsets = np.array([-37, -1, 0, 1, 2, 100], np.int32)
    data = np.random.default_rng(3).standard_normal((6, n))
    v = do.pow2_vector(n)
    a, b = do.spmv_dia_pow2(offsets, data, v), do.spmv_dia(offsets, data, v)
    assert np.array_equal(a, b)
    assert np.count_nonzero(a != do.spmv_dia(offsets, data, v, mutation="diagonals reversed")) >= n // 10


@pytest.mark.parametrize("n", [1, 2, 3, 64, 257])
def test_small_matrices(n):
    offsets, data, v = do.small_matrix(n)
    assert len(set(offsets.tolist())) == offsets.size and all(-n < o < n for o in offsets)
    assert np.allclose(do.spmv_dia(offsets, data, v), do.dense(offsets, data, n) @ v, rtol=0, atol=1e-13)


# ---- cgx_dia_check ---------------------------------------------------------------------------------------------------
def test_constants_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "cgx.h")) as f:
        src = f.read()
    hdr = dict((m.group(1), int(m.group(2), 0))
               for m in re.finditer(r"#define\s+(CGX_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)", src))
    assert hdr["CGX_DIA_ACTIVE"] == DIA_ACTIVE and 0x4 <= DIA_ACTIVE <= 0x80
    assert hdr["CGX_VERSION"] == 101
    others = [v for k, v in hdr.items() if k != "CGX_DIA_ACTIVE" and (k.endswith("_ACTIVE") or k in (
        "CGX_F32_REF", "CGX_A_F32", "CGX_TIMING", "CGX_NO_OVERLAP"))]
    assert all(v & DIA_ACTIVE == 0 for v in others)  # a bit of its own


def test_check_accepts(L):
    offs = np.array(do.STRUCT_OFFSETS, np.int32)  # unsorted, a duplicate, both corners
    assert L.cgx_dia_check(do.STRUCT_N, offs.size, _p(offs)) == 0
    assert L.cgx_dia_check(5, 0, None) == 0  # the zero matrix
    assert L.cgx_dia_check(1, 1, _p(np.zeros(1, np.int32))) == 0
    dia_check(offs, do.STRUCT_N)
    dia_check([], 7)


@pytest.mark.parametrize("offs,n,named", [
    ([0, 1, 5, -5], 5, "offsets[2] = 5"),
    ([0, -5, 5], 5, "offsets[1] = -5"),
    ([1], 1, "offsets[0] = 1"),
    ([0, 3, -200, 131], 131, "offsets[2] = -200"),  # the first offence, not the last
])
def test_check_names_the_first_offence(L, offs, n, named):
    o = np.array(offs, np.int32)
    assert L.cgx_dia_check(n, o.size, _p(o)) == ERR_SHAPE
    assert "cgx_dia_check" in _err(L) and named in _err(L), _err(L)
    with pytest.raises(cg.CgxError) as e:
        dia_check(o, n)
    assert e.value.code == ERR_SHAPE and named in str(e.value)


def test_check_null_and_sizes(L):
    o = np.zeros(2, np.int32)
    assert L.cgx_dia_check(0, 2, _p(o)) == ERR_ARG
    assert L.cgx_dia_check(-3, 0, None) == ERR_ARG
    assert L.cgx_dia_check(4, -1, _p(o)) == ERR_ARG
    assert L.cgx_dia_check(4, 2, None) == ERR_ARG
    assert L.cgx_set_dia(None, 1, _p(o), _p(np.zeros(4)), 4) == ERR_ARG and "ctx is NULL" in _err(L)


# ---- the Python mirror -----------------------------------------------------------------------------------------------
class _FakeSolver:
    """What Solver.set_dia reads before the C call: no context behind it, so a call that got through would fail."""
    _h = None

    def __init__(self, n, csr_nnz, **kw):
        self.n, self.csr_nnz = n, csr_nnz
        self.__dict__.update(kw)


@pytest.mark.parametrize("kw,offsets,data,match", [
    ({}, [0, 1], np.zeros((2, 9)), "columns"),  # ld < n
    ({}, [0, 1, 2], np.zeros((2, 10)), "offsets but"),
    ({}, [0, 1], np.zeros(20), "shape"),
    ({}, [0.5, 1], np.zeros((2, 10)), "integers"),
    ({}, [0, 1], np.zeros((2, 10), complex), "real"),
    ({}, [[0, 1]], np.zeros((2, 10)), "one-dimensional"),
    ({}, [0, 1, 2], np.zeros((3, 10)), "room for"),
    ({}, [0, 2 ** 31], np.zeros((2, 10)), "int32"),
    ({"csr_nnz": None}, [0], np.zeros((1, 10)), "csr_nnz"),
    ({"nrhs": 2}, [0], np.zeros((1, 10)), "one right-hand side"),
    ({"devices": [0, 0]}, [0], np.zeros((1, 10)), "one GPU"),
])
def test_mirror_refuses_before_the_c_call(built, kw, offsets, data, match):
    s = _FakeSolver(10, kw.pop("csr_nnz", 20), **kw)
    with pytest.raises(ValueError, match=match):
        cg.Solver.set_dia(s, offsets, data)


def test_mirror_takes_an_object_with_offsets_and_data(built):
    class Dia:
        offsets, data, shape = np.array([0, 1]), np.zeros((2, 9)), (10, 10)

    with pytest.raises(ValueError, match="columns"):  # read from the object, then refused: ld = 9 < n
        cg.Solver.set_dia(_FakeSolver(10, 20), Dia())
    with pytest.raises(ValueError, match="columns"):
        cg.Solver.from_dia(Dia())
    with pytest.raises(ValueError, match="needed"):
        cg.Solver.from_dia([0, 1])
    with pytest.raises(ValueError):
        cg.dia_check([[0]], 3)
    with pytest.raises(ValueError):
        cg.dia_check([0.5], 3)


# ---- the probe bars the GPU test rests on ------------------------------------------------------------------------------
PROBE_SIZES = (257, 2049)
PROBE_KINDS = (("diag", 0), ("jacobi", 0), ("block", 2), ("block", 8))


class DiaSystem:
    """_pcg_probe.system(n) with the matVec in the diagonal order, in numpy float64: the 7 diagonals ascending, one
    accumulator per row (a product and an add in place of the FMA: one more rounding per term)."""

    def __init__(self, n):
        self.sys, self.n = pp.system(n), n
        self.b = self.sys.b
        self.offsets, self.data = do.from_csr(*self.sys.csr(), n)
        assert list(self.offsets) == [-37, -2, -1, 0, 1, 2, 37]

    def apply(self, p):
        assert p.dtype == np.float64
        acc = np.zeros(self.n)
        for k, o in enumerate(self.offsets):
            lo, hi = do.in_range(int(o), self.n)
            acc[lo - o:hi - o] = acc[lo - o:hi - o] + self.data[k, lo:hi] * p[lo:hi]
        return acc


@pytest.mark.parametrize("n", PROBE_SIZES)
def test_probe_bars_are_reachable(n):
    ds = DiaSystem(n)
    worst = 0.0
    for zero in (False, True):
        x0 = np.zeros(n) if zero else ds.sys.x0
        for kind, bs in PROBE_KINDS:
            case = pp.Case(kind, bs, n, zero)
            pr = pp.probe(case)
            for dot in pp.DOTS.values():
                X = pp.pcg(ds, x0, pp.precond(case), np.float64, dot)
                for k in pp.KS:
                    ratio, bar = float(np.max(pp.ratios(X[k - 1], pr.X[k], pr.S[k]))), pp.bar(case, k)
                    worst = max(worst, ratio / bar)
                    assert ratio <= bar <= pp.CAP, (case, k, ratio, bar)
        # plain CG: _nrhs_probe's column 0 of the same banded system
        col = npr.Col("csr", n, 0, zero)
        ref = npr.column(col)
        b, x0 = npr.start(col)
        ds_plain = DiaSystem(n)
        ds_plain.b = b
        for dot in npr.DOTS.values():
            X, _ = npr.cg(ds_plain, b, x0, np.float64, dot)
            for k in pp.KS:
                ratio, bar = float(np.max(npr.ratios(X[k - 1], ref.X[k], ref.S[k]))), npr.bar(col, k)
                worst = max(worst, ratio / bar)
                assert ratio <= bar <= npr.CAP, (col, k, ratio, bar)
    print(f"\n[dia probe bars] n={n}: worst ratio {worst:.3g} of its bar")


# ---- `cg_hip --csr --dia`'s refusals (before any file or device is touched) --------------------------------------------
@pytest.mark.parametrize("opts", [("--dia",), ("--csr-a32", "--dia"), ("--csr", "--dia", "--bsr", "2"),
                                  ("--dia", "--jacobi"), ("--gpus", "2", "--dia")])
def test_cli_refuses_dia_without_plain_csr(built, opts):
    import subprocess
    r = subprocess.run([cg.CLI_PATH, *opts, "A.txt", "b.txt", "x0.txt"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--dia holds a --csr matrix by its diagonals" in r.stderr, r.stderr


def test_cli_usage_names_dia(built):
    import subprocess
    r = subprocess.run([cg.CLI_PATH, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--csr --dia" in r.stdout + r.stderr
