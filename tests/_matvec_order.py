"""The summation order of the dense row-streaming matVec kernels, on the CPU.

An exact emulation of the order DESIGN.md s3 documents, independent of the
GPU code: every plan of every kernel of the family must give these bits.

fp64 row (k_matvec_f64 non-rotated, k_matvec_small_f64, each column of
k_matvec_nrhs_f64): lane l of the wave adds columns 128c + 2l into .x and
128c + 2l + 1 into .y for the chunks c = 0, 1, ... of the first vec_cols
columns, then the tail columns vec_cols + l, + 64, ... into .x, each with one
FMA; then x + y, then the wave sum.

float-A row (k_matvec_a32): chunks of 256 columns, lane l adds columns
256c + 4l + {0, 1, 2, 3} into .x .y .z .w (the float widened to double, one
FMA each), tail columns into .x; then (x + y) + (z + w), then the wave sum.

vec_cols is the whole chunks of the row when the kernel may use 16-byte loads
(vec_cols_f64 / vec_cols_a32 below), otherwise 0: every column is a tail
column.
"""
from fractions import Fraction

import numpy as np

# The shapes the CPU and GPU order tests share.  11 rows: no multiple of 2, 4
# or 8, so the last row group is clamped, and fewer than one block's waves
# times R.  fp64 columns (128 per chunk): 127 no whole chunk; 389 three chunks
# and a tail; 1024 one U = 8 step, no remainder; 1153 one step, one remaining
# chunk, a tail; 2176 = 17 chunks, both ping-pong halves and a remainder; 3277
# three steps, a chunk and a tail (the loop leaves through its second exit).
# Float-A columns (256 per chunk) likewise for U = 2 and 4.
ROWS = 11
F64_COLS = (127, 389, 1024, 1153, 2176, 3277)
A32_COLS = (255, 517, 1024, 1285, 2307)


def fma(a, b, c):
    """a * b + c with one rounding: the Fractions are exact, float() of one rounds correctly."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def wave_sum(v):
    """cgx_device.h wave_sum over the 64 lanes' values: v[l] += v[l ^ o] for o = 32, 16, ..., 1."""
    v = [float(x) for x in v]
    assert len(v) == 64
    o = 32
    while o:
        v = [v[l] + v[l ^ o] for l in range(64)]
        o >>= 1
    assert all(x == v[0] or x != x for x in v)
    return v[0]


def vec_cols_f64(cols, a_ptr, v_ptr, lda):
    return cols & ~127 if (a_ptr | v_ptr) % 16 == 0 and lda % 2 == 0 else 0


def vec_cols_a32(cols, a_ptr, v_ptr, lda):
    return cols & ~255 if a_ptr % 16 == 0 and v_ptr % 32 == 0 and lda % 4 == 0 else 0


def _row(a, v, cols, vec_cols, width):
    """One row: `width` accumulators per lane (2: fp64 A, 4: float A), chunks of 64 * width columns."""
    a = [float(x) for x in a[:cols]]
    v = [float(x) for x in v[:cols]]
    chunk = 64 * width
    assert vec_cols % chunk == 0 and 0 <= vec_cols <= cols
    lanes = []
    for l in range(64):
        acc = [0.0] * width
        for c in range(vec_cols // chunk):
            j = chunk * c + width * l
            for e in range(width):
                acc[e] = fma(a[j + e], v[j + e], acc[e])
        for j in range(vec_cols + l, cols, 64):
            acc[0] = fma(a[j], v[j], acc[0])
        lanes.append(acc[0] + acc[1] if width == 2 else (acc[0] + acc[1]) + (acc[2] + acc[3]))
    return wave_sum(lanes)


def matvec_f64(A, v, cols, vec_cols):
    """Rows of A (any 2-D indexable, row i's first `cols` entries used) times v, in the fp64 kernels' order."""
    return [_row(row, v, cols, vec_cols, 2) for row in A]


def matvec_a32(A, v, cols, vec_cols):
    """As matvec_f64 for a float32 A (its values widen to double exactly), in k_matvec_a32's order."""
    return [_row(row, v, cols, vec_cols, 4) for row in A]


def f64_case(cols, lda):
    """(A, v) of the order tests: ROWS x lda doubles (NaN in the pitch padding, which is never read) and cols."""
    rng = np.random.default_rng(7 * cols + lda)
    A = np.full((ROWS, lda), np.nan)
    A[:, :cols] = rng.random((ROWS, cols)) - 0.5
    return A, rng.random(cols)


def a32_case(cols, lda):
    rng = np.random.default_rng(5 * cols + lda)
    A = np.full((ROWS, lda), np.nan, np.float32)
    A[:, :cols] = rng.standard_normal((ROWS, cols)).astype(np.float32)
    return A, rng.standard_normal(cols)
