"""cgx_set_dia_sym without a GPU: the expansion the order contract is stated against (tests/_dia_sym.py), the offset
check, the Python mirror's own checks and `cg_hip --dia-sym`'s refusals."""
import numpy as np
import pytest

import _dia_order as do
import _dia_sym as ds
import conjugate_gradient_amd as cg

ERR_ARG, ERR_SHAPE = -1, -4
# None on a tree without the feature: every test then fails at its first use
DIA_SYM_ACTIVE = getattr(cg, "CGX_DIA_SYM_ACTIVE", None)
dia_sym_check = getattr(cg, "dia_sym_check", None)
set_dia_sym = getattr(cg.Solver, "set_dia_sym", None)
from_dia_sym = getattr(cg.Solver, "from_dia_sym", None)


@pytest.fixture(scope="module")
def L(built):
    assert hasattr(cg.Solver, "set_dia_sym"), "the package has no one-sided diagonal storage"
    return cg.lib()


def _p(a):
    return a.ctypes.data


def _err(L):
    return L.cgx_last_error().decode()


# ---- the expansion ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndiag", ds.STRUCT_NDIAGS)
def test_expansion_is_symmetric_and_is_triu_plus_its_transpose(ndiag):
    offsets, data, v = ds.structure_matrix(ndiag)
    n = ds.STRUCT_N
    assert data.shape == (ndiag, ds.STRUCT_LD)
    A = ds.dense(offsets, data, n)
    assert np.isfinite(A).all() and np.array_equal(A, A.T)  # no unused slot reached the matrix
    T = do.dense(offsets, data, n) if ndiag else np.zeros((n, n))  # the stored matrix read as a full DIA one: triu(A)
    assert np.array_equal(T, np.triu(T)) and np.array_equal(A, T + T.T - np.diag(np.diag(T)))
    eo, ed = ds.expand(offsets, data, n)
    assert eo.size == ndiag + sum(1 for o in offsets if o > 0)
    out = do.spmv_dia(eo, ed, v)
    assert np.isfinite(out).all() and np.allclose(out, A @ v, rtol=0, atol=1e-13 * max(1, 2 * ndiag))
    assert np.array_equal(out, ds.spmv(offsets, data, v))  # upper then lower is the expansion's order


def test_expansion_order_and_slots():
    offsets, data, _ = ds.structure_matrix()
    n = ds.STRUCT_N
    eo, ed = ds.expand(offsets, data, n)
    want = []
    for o in offsets:
        want += [int(o), -int(o)] if o > 0 else [0]
    assert eo.tolist() == want
    for k, o in enumerate(eo):
        lo, hi = do.in_range(int(o), n)
        assert np.isnan(ed[k, :lo]).all() and np.isnan(ed[k, hi:]).all() and np.isfinite(ed[k, lo:hi]).all()
    k37 = want.index(-37)
    assert np.array_equal(ed[k37, :n - 37], data[1, 37:n])  # data'[j] = data[k][j + o]


def test_structure_matrix_holds_nan_in_every_unused_slot():
    offsets, data, _ = ds.structure_matrix()
    n = ds.STRUCT_N
    for k, o in enumerate(offsets):
        assert np.isnan(data[k, :o]).all() and np.isnan(data[k, n:]).all() and np.isfinite(data[k, o:n]).all()
    assert np.count_nonzero(data == 0.0) >= 5  # stored zeros among the entries


@pytest.mark.parametrize("mutation", ds.MUTATIONS)
def test_mutations_change_bits(mutation):
    offsets, data, v = ds.structure_matrix()
    good, bad = ds.spmv(offsets, data, v), ds.spmv(offsets, data, v, mutation=mutation)
    assert np.isfinite(bad).all() and not np.array_equal(good, bad), mutation


def test_upper_of_round_trips():
    import _pcg_probe as pp
    n = 130
    full = do.from_csr(*pp.system(n).csr(), n)
    offsets, data = ds.upper_of(*full, n)
    assert offsets.tolist() == [0, 1, 2, 37]
    assert np.array_equal(ds.dense(offsets, data, n), pp.system(n).dense())


@pytest.mark.parametrize("n", [1, 2, 3, 64, 257])
def test_small_matrices(n):
    offsets, data, v = ds.small_matrix(n)
    assert data.shape == (offsets.size, n + 1) and all(0 <= o < n for o in offsets)
    out = do.spmv_dia(*ds.expand(offsets, data, n), v)
    assert np.allclose(out, ds.dense(offsets, data, n) @ v, rtol=0, atol=1e-13)


# ---- cgx_dia_sym_check -----------------------------------------------------------------------------------------------
def test_constants_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "cgx.h")) as f:
        src = f.read()
    hdr = dict((m.group(1), int(m.group(2), 0))
               for m in re.finditer(r"#define\s+(CGX_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)", src))
    assert hdr["CGX_DIA_SYM_ACTIVE"] == DIA_SYM_ACTIVE == 0x8
    assert hdr["CGX_VERSION"] == 101
    others = [v for k, v in hdr.items() if k != "CGX_DIA_SYM_ACTIVE" and (k.endswith("_ACTIVE") or k in (
        "CGX_F32_REF", "CGX_A_F32", "CGX_TIMING", "CGX_NO_OVERLAP"))]
    assert all(v & DIA_SYM_ACTIVE == 0 for v in others)  # a bit of its own
    assert {"CGX_DIA_SYM_ACTIVE", "dia_sym_check", "spmv_dia_sym"} <= set(cg.__all__)


def test_check_accepts(L):
    offs = np.array(ds.STRUCT_OFFSETS, np.int32)  # unsorted, duplicates, the corner
    assert L.cgx_dia_sym_check(ds.STRUCT_N, offs.size, _p(offs)) == 0
    assert L.cgx_dia_sym_check(5, 0, None) == 0  # the zero matrix
    assert L.cgx_dia_sym_check(1, 1, _p(np.zeros(1, np.int32))) == 0
    dia_sym_check(offs, ds.STRUCT_N)
    dia_sym_check([], 7)


@pytest.mark.parametrize("offs,n,named,negative", [
    ([0, 1, 5, -5], 5, "offsets[2] = 5", False),
    ([0, -1, 5], 5, "offsets[1] = -1", True),
    ([1], 1, "offsets[0] = 1", False),
    ([0, 3, -200, 131], 131, "offsets[2] = -200", True),  # the first offence, not the last
])
def test_check_names_the_first_offence(L, offs, n, named, negative):
    o = np.array(offs, np.int32)
    assert L.cgx_dia_sym_check(n, o.size, _p(o)) == ERR_SHAPE
    assert "cgx_dia_sym_check" in _err(L) and named in _err(L), _err(L)
    assert ("one-sided storage holds offsets >= 0" in _err(L)) == negative, _err(L)
    with pytest.raises(cg.CgxError) as e:
        dia_sym_check(o, n)
    assert e.value.code == ERR_SHAPE and named in str(e.value)


def test_check_null_and_sizes(L):
    o = np.zeros(2, np.int32)
    assert L.cgx_dia_sym_check(0, 2, _p(o)) == ERR_ARG
    assert L.cgx_dia_sym_check(-3, 0, None) == ERR_ARG
    assert L.cgx_dia_sym_check(4, -1, _p(o)) == ERR_ARG
    assert L.cgx_dia_sym_check(4, 2, None) == ERR_ARG
    assert L.cgx_set_dia_sym(None, 1, _p(o), _p(np.zeros(4)), 4) == ERR_ARG and "ctx is NULL" in _err(L)


# ---- the Python mirror -----------------------------------------------------------------------------------------------
class _FakeSolver:
    """What Solver.set_dia_sym reads before the C call: no context behind it, so a call that got through would fail."""
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
        set_dia_sym(s, offsets, data)


def test_mirror_refusals_are_worded_as_set_dia_words_them(built):
    """A solver created with devices= or nrhs=: the same sentence after the method's name."""
    for kw in ({"nrhs": 2}, {"devices": [0, 0]}):
        msgs = []
        for method in (cg.Solver.set_dia, set_dia_sym):
            with pytest.raises(ValueError) as e:
                method(_FakeSolver(10, 20, **kw), [0], np.zeros((1, 10)))
            msgs.append(str(e.value).split(": ", 1)[1])
        assert msgs[0] == msgs[1], msgs


def test_mirror_takes_an_object_with_offsets_and_data(built):
    class Dia:
        offsets, data, shape = np.array([0, 1]), np.zeros((2, 9)), (10, 10)

    with pytest.raises(ValueError, match="columns"):  # read from the object, then refused: ld = 9 < n
        set_dia_sym(_FakeSolver(10, 20), Dia())
    with pytest.raises(ValueError, match="columns"):
        from_dia_sym(Dia())
    with pytest.raises(ValueError, match="needed"):
        from_dia_sym([0, 1])
    with pytest.raises(ValueError):
        dia_sym_check([[0]], 3)
    with pytest.raises(ValueError):
        dia_sym_check([0.5], 3)


# ---- `cg_hip --csr --dia-sym`'s refusals (before any file or device is touched) ------------------------------------------
@pytest.mark.parametrize("opts", [("--dia-sym",), ("--csr-a32", "--dia-sym"), ("--csr", "--dia-sym", "--bsr", "2"),
                                  ("--csr", "--dia", "--dia-sym"), ("--dia-sym", "--jacobi")])
def test_cli_refuses_dia_sym_without_plain_csr(built, opts):
    import subprocess
    r = subprocess.run([cg.CLI_PATH, *opts, "A.txt", "b.txt", "x0.txt"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stderr
    assert r.stderr.startswith("--dia-sym holds a --csr matrix by its upper diagonals") and r.stderr.count("\n") == 1


def test_cli_usage_names_dia_sym(built):
    import subprocess
    r = subprocess.run([cg.CLI_PATH, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--csr --dia-sym" in r.stdout + r.stderr
