"""CPU checks of the preconditioned-CG probe's reference and data (tests/_pcg_probe.py): the long-double band operator
against the explicit matrix, the recurrence against a direct solve, W's properties, the cap on every bar, and that the
bar tells a wrong preconditioner from a right one.  `pytest -s` prints the table that _pcg_probe's docstring quotes."""
import numpy as np
import pytest

import _pcg_probe as pp

LD_EPS = float(np.finfo(pp.LD).eps)
SMALL_BLOCK_CASES = [pp.block_case(bs, t) for bs, t in pp.BLOCK_CASES]


def test_apply_ld_is_the_explicit_matrix():
    """n = 80: every band is there, the 37-band twice per row in the middle rows."""
    s = pp.system(80)
    A, p = s.dense(), s.x0
    assert np.array_equal(A, A.T) and np.count_nonzero(A) == 80 + 2 * (79 + 78 + 43)
    assert np.all(np.diag(A) - (np.abs(A).sum(axis=1) - np.diag(A)) > 1.0)  # strictly diagonally dominant
    want = A.astype(pp.LD) @ p.astype(pp.LD)
    got = s.apply(p.astype(pp.LD))
    assert got.dtype == pp.LD
    # seven products and six sums per row in long double: a few of its ulps of |A| |p|
    assert np.all(np.abs(got - want) <= 8 * LD_EPS * (np.abs(A) @ np.abs(p)))
    assert np.all(np.abs(s.apply(p) - A @ p) <= 8 * pp.ULP * (np.abs(A) @ np.abs(p)))
    # the CSR arrays of a matrix with fewer rows than a band is far: the band is absent
    indptr, indices, data = pp.system(3).csr()
    assert indptr.tolist() == [0, 3, 6, 9] and indices.tolist() == [0, 1, 2] * 3 and indices.dtype == np.int32
    assert pp.system(1).csr()[1].tolist() == [0]


def by_hand(s, W, loops):
    """x after each loop of the recurrence of tests/_bpcg_ref.py from the system's x0, in long double."""
    x = s.x0.astype(pp.LD)
    r = s.b.astype(pp.LD) - s.apply(x)
    p = pp.apply_m(W, r)
    rz = np.dot(r, p)
    X = []
    for _ in range(loops):
        Ap = s.apply(p)
        alpha = rz / np.dot(p, Ap)
        x, r = x + alpha * p, r - alpha * Ap
        X.append(x)
        z = pp.apply_m(W, r)
        rz_new = np.dot(r, z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return X


def test_recurrence_solves_a_small_system():
    """n = 12, bs = 3, W the exact inverses of A's diagonal blocks: exact PCG ends after at most n loops; in long
    double 12 loops leave a residual far below fp64 rounding of |b|.  pp.pcg's three loops are that recurrence's."""
    n, bs = 12, 3
    s = pp.system(n)
    A = s.dense()
    W = np.stack([np.linalg.inv(A[k:k + bs, k:k + bs]) for k in range(0, n, bs)])
    X = by_hand(s, W, n)
    assert np.max(np.abs(s.b.astype(pp.LD) - s.apply(X[-1]))) <= 1e-17 * np.max(np.abs(s.b))
    assert np.allclose(X[-1].astype(np.float64), np.linalg.solve(A, s.b), rtol=0, atol=1e-13)
    got = pp.pcg(s, s.x0, W, pp.LD, np.dot)
    assert len(got) == 3 and all(np.array_equal(got[k], X[k]) for k in range(3))


def test_apply_m_is_the_block_product():
    ref, _ = pp.blocks(23, 4)  # five full blocks and one of three rows
    r = pp.system(23).b
    want = np.concatenate([ref[k] @ np.pad(r, (0, 1))[4 * k:4 * k + 4] for k in range(6)])[:23]
    assert np.allclose(pp.apply_m(ref, r), want, rtol=0, atol=4 * pp.ULP)
    assert pp.apply_m(ref, r.astype(pp.LD)).dtype == pp.LD
    m = pp.minv(23, "diag")
    assert np.array_equal(pp.apply_m(m, r), m * r)


@pytest.mark.parametrize("case", SMALL_BLOCK_CASES + [pp.Case("block", bs, bs - 1, False) for bs in pp.BLOCK_SIZES], ids=str)
def test_w_properties(case):
    bs, n = case.bs, case.n
    ref, given = pp.blocks(n, bs)
    nblk = pp.nblocks(n, bs)
    t = n - (nblk - 1) * bs  # the last block's used rows, 1..bs
    assert ref.shape == given.shape == (nblk, bs, bs) and not ref.flags.writeable and not given.flags.writeable
    used = np.ones((nblk, bs, bs), bool)
    used[-1, t:, :] = used[-1, :, t:] = False
    assert np.array_equal(np.isnan(given), ~used)  # NaN exactly in the unused slots
    assert np.array_equal(given[used], ref[used]) and not ref[~used].any()
    d = np.arange(bs)
    diag = ref[:, d, d][used[:, d, d]]
    assert diag.min() >= 0.5 and diag.max() < 2.0
    off = ref[used & ~np.eye(bs, dtype=bool)[None]]
    assert np.all(np.abs(off) <= 0.4 / bs) and (off.size == 0 or np.all(off != 0.0))
    for k in range(nblk):
        tk = t if k == nblk - 1 else bs
        B = ref[k, :tk, :tk]
        if tk >= 2:
            assert not np.array_equal(B, B.T), k  # unsymmetric
        assert np.linalg.eigvalsh(0.5 * (B + B.T)).min() >= 0.1, k


def test_minv_and_diagonal_blocks():
    for n in pp.DIAG_SIZES:
        m = pp.minv(n, "diag")
        assert m.shape == (n,) and m.min() >= 0.5 and m.max() < 2.0
        assert np.array_equal(pp.minv(n, "jacobi"), 1.0 / pp.system(n).diag)
    for bs in pp.DIAGONAL_BLOCK_SIZES:
        n = pp.block_n(bs, 1)
        W = pp.diagonal_blocks(n, bs)
        i = np.arange(n)
        assert np.array_equal(W[i // bs, i % bs, i % bs], pp.minv(n, "diag"))
        assert np.isnan(W).sum() == bs * bs - 1 and np.isnan(W[-1]).sum() == bs * bs - 1
        assert np.count_nonzero(np.nan_to_num(W)) == n
        # the reference of these blocks is the "diag" case's: the same z with the zeros in
        ref = np.nan_to_num(W)
        r = pp.system(n).b
        assert np.array_equal(pp.apply_m(ref, r), pp.minv(n, "diag") * r)


def test_scale_is_the_sum_of_the_terms():
    """S_1 = |x0| + alpha_0 |W| |r_0| on a small case, by hand; S grows with k; x0 = 0 leaves only the steps."""
    case = pp.block_case(3, 2)
    pr = pp.probe(case)
    s, x0 = pp.start(case)
    ref = pp.blocks(case.n, 3)[0].astype(pp.LD)
    r0 = s.b.astype(pp.LD) - s.apply(x0.astype(pp.LD))
    z0 = pp.apply_m(ref, r0)
    alpha0 = np.dot(r0, z0) / np.dot(z0, s.apply(z0))
    S1 = np.abs(x0) + alpha0 * pp.apply_m(np.abs(ref), np.abs(r0))
    assert np.allclose(pr.S[1], S1.astype(np.float64), rtol=4 * pp.ULP, atol=0)
    assert np.array_equal(pr.X[1], x0.astype(pp.LD) + alpha0 * z0)
    assert np.all(pr.S[1] < pr.S[2]) and np.all(pr.S[2] < pr.S[3])
    for k in pp.KS:
        assert np.all(np.abs(pr.X[k]) <= pr.S[k] * (1 + 1e-15))  # x is a sum of the terms S adds up in magnitude
    zero = pp.probe(case._replace(zero=True))
    bl = s.b.astype(pp.LD)
    zb = pp.apply_m(ref, bl)
    a0 = np.dot(bl, zb) / np.dot(zb, s.apply(zb))
    assert np.array_equal(zero.X[1], a0 * zb)
    assert np.allclose(zero.S[1], (a0 * pp.apply_m(np.abs(ref), np.abs(bl))).astype(np.float64), rtol=4 * pp.ULP, atol=0)


def test_bars_are_capped():
    cases = pp.all_cases()
    assert len(cases) == len(set(cases)) == 2 * (35 + 7 + 20 + 2) + 2  # the two grid-stride cases: x0 rough only
    for c in cases:
        for k in pp.KS:
            sp = pp.spreads(c)[k]
            assert len(sp) == 3 and pp.bar(c, k) == 100.0 * max(*sp, pp.FLOOR)
            assert pp.FLOOR * 100 <= pp.bar(c, k) <= pp.CAP, (c, k, sp)
    # the floor is taken from the smallest cases: a few ulps, between what they measure and what two thread blocks do
    worst = lambda pick: max(max(max(v) for v in pp.spreads(c).values()) for c in cases if pick(c))  # noqa: E731
    tiny, two_blocks = worst(lambda c: c.n <= 7), worst(lambda c: 255 <= c.n <= pp.SMALL)
    assert tiny <= pp.FLOOR <= two_blocks <= 64 * pp.ULP, (tiny, two_blocks)
    print("\n" + pp.table())


# ---- the probe discriminates ----------------------------------------------------------------------------------------
def misses_by(case, M):
    """The largest |x_1 - x_ld| / (bar S_1) of the fp64 restatement run with the preconditioner M."""
    pr = pp.probe(case)
    x1 = pp.restate(case, pp.DOTS["d_at"], M)[0]
    return float(np.max(pp.ratios(x1, pr.X[1], pr.S[1]))) / pp.bar(case, 1)


def block_mutants(case):
    ref = pp.blocks(case.n, case.bs)[0]
    bs = case.bs
    t = case.n - (ref.shape[0] - 1) * bs
    out = {"transposed": ref.transpose(0, 2, 1).copy()}
    for name, where in (("last used row", (-1, t - 1, 0)), ("block 0 [0][bs-1]", (0, 0, bs - 1))):
        out[name] = ref.copy()
        assert out[name][where] != 0.0
        out[name][where] = 0.0
    if t < bs:  # a short last block, applied with t - 1 rows
        out["short block, t - 1 rows"] = ref.copy()
        out["short block, t - 1 rows"][-1, t - 1, :] = 0.0
        out["short block, t - 1 rows"][-1, :, t - 1] = 0.0
    return out


@pytest.mark.parametrize("case", SMALL_BLOCK_CASES, ids=str)
def test_probe_discriminates_blocks(case):
    assert misses_by(case, pp.precond(case)) <= 0.01 + 1e-12  # the right W: within the measured spread
    muts = block_mutants(case)
    assert len(muts) == (4 if case.n % case.bs else 3)
    for name, M in muts.items():
        q = misses_by(case, M)
        assert q >= 1000.0, (name, q)


@pytest.mark.parametrize("kind", pp.DIAG_KINDS)
@pytest.mark.parametrize("n", [n for n in pp.DIAG_SIZES if n > 1])
def test_probe_discriminates_diagonal_kinds(kind, n):
    case = pp.Case(kind, 0, n, False)
    assert misses_by(case, pp.precond(case)) <= 0.01 + 1e-12
    q = misses_by(case, np.roll(pp.precond(case), 1))  # minv shifted by one element
    assert q >= 1000.0, q
