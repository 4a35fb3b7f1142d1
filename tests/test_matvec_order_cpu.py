"""The CPU statement of the matVec kernels' summation order (_matvec_order.py)
checked on its own: it is a matVec, it is exact where every order is, and it
is an order -- on random data its bits differ from numpy's A @ v, so a GPU
test that demands equality with it can tell one order from another."""
import numpy as np
import pytest

import _matvec_order as mo

F64_TOL = 1e-13  # as test_gpu_kernels.py: a reordered fp64 sum of <= 8192 terms, relative to sum|a_i v_i|

CASES = [("f64", c) for c in mo.F64_COLS + (2048, 2560)] + [("a32", c) for c in mo.A32_COLS]


def emulate(kind, cols, vector_path=True):
    if kind == "f64":
        A, v = mo.f64_case(cols, cols)
        vc = mo.vec_cols_f64(cols, 0, 0, (cols + 1) & ~1 if vector_path else cols | 1)
        return A, v, np.array(mo.matvec_f64(A, v, cols, vc))
    lda = (cols + 3) & ~3
    A, v = mo.a32_case(cols, lda)
    vc = mo.vec_cols_a32(cols, 0, 0 if vector_path else 16, lda)
    return A[:, :cols].astype(np.float64), v, np.array(mo.matvec_a32(A, v, cols, vc))


def test_fma_and_wave_sum():
    assert mo.fma(3.0, 5.0, 7.0) == 22.0
    # one rounding: (1 + 2^-30)^2 - 1 keeps the 2^-60 term a separate multiply and add lose
    x = 1.0 + 2.0 ** -30
    assert mo.fma(x, x, -1.0) == 2.0 ** -29 + 2.0 ** -60 != x * x - 1.0
    assert mo.wave_sum(range(64)) == 2016.0
    # the butterfly's pairing: ((v0 + v32) + (v16 + v48)) + ..., not a left-to-right chain
    v = [0.0] * 64
    v[0], v[32], v[16] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert mo.wave_sum(v) == 1.0 and sum(v[i] for i in (32, 16, 0)) != 1.0


@pytest.mark.parametrize("kind,cols", CASES)
def test_emulator_is_a_matvec_in_its_own_order(kind, cols):
    A, v, y = emulate(kind, cols)
    ref = A @ v
    assert np.all(np.abs(y - ref) <= F64_TOL * (np.abs(A) @ np.abs(v)))
    assert np.any(y != ref), "the emulated order gives numpy's bits in every row: equality with it would pin nothing"
    if cols in (389, 517):  # the scalar path (every column a tail column) is an order of its own
        _, _, ys = emulate(kind, cols, vector_path=False)
        assert np.all(np.abs(ys - ref) <= F64_TOL * (np.abs(A) @ np.abs(v)))
        assert np.any(ys != y)


@pytest.mark.parametrize("kind,cols", [("f64", 389), ("f64", 1153), ("a32", 517), ("a32", 1285)])
def test_emulator_exact_on_small_integers(kind, cols):
    rng = np.random.default_rng(cols)
    A = rng.integers(-8, 9, (mo.ROWS, cols)).astype(np.float32 if kind == "a32" else np.float64)
    v = rng.integers(-8, 9, cols).astype(np.float64)
    want = (A.astype(np.int64) @ v.astype(np.int64)).astype(np.float64)
    for vc in (0, cols & ~255):
        got = mo.matvec_a32(A, v, cols, vc) if kind == "a32" else mo.matvec_f64(A, v, cols, vc)
        assert np.array_equal(np.array(got), want)
