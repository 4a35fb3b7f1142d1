"""CGX_A_F32: A stored as float on the GPU, b / x / r / p / Ap and all
arithmetic in fp64 (k_matvec_a32).  A float widens to double exactly, so the
bar is the project's fp64 one against the oracle on A32.astype(float64): the
same loop count, ||x - x_oracle|| <= 1e-10 ||x_oracle||, ||b - A64 x|| <=
1e-10 ||b||.  The loop-count condition is safe for a reordered sum on every
system here: sqrt(r.r)/eps at the stopping iteration and one before it are far
from 1 on each of them (a factor of 3 at the least, 0.33 / 51 at spd1024 and
hash n = 1000)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import conjugate_gradient_amd as cg
import oracle
import _matvec_order as mo
from _cases import case

pytestmark = pytest.mark.gpu
TOL = 1e-10
A_F32 = getattr(cg, "CGX_A_F32", None)  # None on a tree without the feature: every test then fails at its first use

# (rows per wave, 256-column chunks in flight) x load policy: every plan k_matvec_a32 is instantiated for
PLANS = [(R, U, nt) for (R, U) in ((1, 4), (1, 8), (2, 4), (4, 2), (4, 4), (8, 2)) for nt in (2, 8)]


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"


def rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)


@functools.lru_cache(maxsize=None)
def hash_system(n, seed):
    """(A32, A64 = A32 widened, b, oracle x, oracle loop count) of spd_hash(n, seed) with A rounded to float."""
    A, b = oracle.spd_hash(n, seed=seed)
    A32 = A.astype(np.float32)
    A64 = A32.astype(np.float64)
    xo, so = oracle.cg_f64(A64, b, np.zeros(n), eps=1e-10)
    for a in (A32, A64, b, xo):
        a.setflags(write=False)
    return A32, A64, b, xo, so.iterations


def meets_bar(x, iters, A64, b, xo, K):
    assert iters == K, (iters, K)
    assert rel(x, xo) <= TOL, rel(x, xo)
    assert np.linalg.norm(b - A64 @ x) <= TOL * np.linalg.norm(b)


@pytest.mark.parametrize("name", ["kat4", "spd512", "spd1024", "spd2048", "spd4096", "spd8192"])
def test_solve_parity_on_reference_matrices(name):
    """The reference's own matrices as it holds them (float), b and x0 widened:
    Solver(flags=CGX_A_F32) and conjugrad(float32 A, float64 x) meet the fp64
    bar, agree bit for bit, and a second solve repeats the bits."""
    A32, b32, x032 = case(name, np.float32)
    n = b32.size
    A64, b, x0 = A32.astype(np.float64), b32.astype(np.float64), x032.astype(np.float64)
    xo, so = oracle.cg_f64(A64, b, x0, eps=1e-10)
    with cg.Solver(n, flags=A_F32) as s:
        info = s.info
        assert info.elem_bytes == 8 and info.flags & A_F32 and info.lda % 256 == 0 and info.lda >= n
        s.set_system(A32, b, x0)
        x1, st1 = s.solve(x0, eps=1e-10)
        x2, st2 = s.solve(x0, eps=1e-10)
    xc = x0.copy()
    stc = cg.conjugrad(A32, b, xc, eps=1e-10)
    meets_bar(x1, st1.iterations, A64, b, xo, so.iterations)
    assert st1.converged == 1
    assert st2.iterations == st1.iterations and np.array_equal(x1, x2)
    assert stc.iterations == st1.iterations and np.array_equal(x1, xc)


@pytest.mark.parametrize("n,seed", [(1, 3), (5, 3), (130, 5), (255, 4), (256, 4), (257, 4), (1000, 2), (2100, 8),
                                    (2304, 1), (5000, 9), (8193, 4)])
def test_every_chunk_and_tail_boundary_every_iteration_form(monkeypatch, n, seed):
    """Below one 256-column chunk, one chunk -1 / 0 / +1, chunk counts that are
    no multiple of U (2100: 9, 2304: 9, 5000: 20 chunks of which U = 8 leaves
    4), odd n, and 8193 (past the two-launch limit): three launches
    (CGX_FUSE_P=0) and two (=1), device-gated and host-checked, a fixed count
    and a solve in pieces all give the same x bit for bit and meet the bar;
    the folded and LDS-staged forms are never on."""
    A32, A64, b, xo, K = hash_system(n, seed)
    res = {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("CGX_FUSE_P", fuse)
        for gated in ("1", "0"):
            monkeypatch.setenv("CGX_GATED", gated)
            with cg.Solver(n, flags=A_F32) as s:
                info = s.info
                assert info.elem_bytes == 8 and info.flags & A_F32
                assert bool(info.flags & cg.CGX_FUSED_ACTIVE) == (fuse == "1")
                assert not info.flags & (cg.CGX_FOLD_ACTIVE | cg.CGX_SMALL_ACTIVE)
                s.set_system(A32, b)
                x, st = s.solve(np.zeros(n), eps=1e-10)
                xf, stf = s.solve(np.zeros(n), eps=-1.0, max_iter=9)
                s.set_x(np.zeros(n))
                s.begin()
                d1, _ = s.iterate(3)
                d2, conv = s.iterate(100, eps=1e-10)
                xp = s.get_x()
            res[(fuse, gated)] = (x, st.iterations, xf, stf.iterations, xp, d1 + d2, conv)
    ref = res[("0", "0")]
    meets_bar(ref[0], ref[1], A64, b, xo, K)
    for key, (x, it, xf, itf, xp, dp, conv) in res.items():
        assert it == ref[1] and np.array_equal(x, ref[0]), key
        assert itf == 9 and np.array_equal(xf, ref[2]), key
        # the pieces: 3 fixed iterations, then to convergence (n = 1 has converged exactly by then: r = p = 0,
        # alpha = beta = 0, x stays; the next tested iteration stops)
        assert conv and dp == max(it, 4) and np.array_equal(xp, ref[0]), key


SHAPES = [(1, 1, 1), (3, 5, 7), (37, 255, 255), (64, 256, 256), (129, 257, 260), (300, 1000, 1024), (8, 4352, 4352),
          (2048, 4096, 4096)]


@pytest.mark.parametrize("rows,cols,lda", SHAPES)
def test_kernel_level_matvec_every_plan(monkeypatch, rows, cols, lda):
    """cg.matVec with a float32 A and float64 v / out against
    A32.astype(float64) @ v: a sum of `cols` exact products in any order is
    within cols * 2^-53 * (|A||v|)_i of the exact value to first order (the
    derived bound; both this kernel's and numpy's sums stay far inside it, the
    error of a sum growing like sqrt(cols) in practice).  Pitches that are no
    multiple of 4 floats ((3,5,7), (37,255,255)) take the scalar path
    throughout; then every plan the kernel offers, through
    CGX_MV_A32_PLAN: the same row sums bit for bit."""
    rng = np.random.default_rng(1000 * rows + cols)
    A = np.zeros((rows, lda), np.float32)
    A[:, :cols] = rng.standard_normal((rows, cols)).astype(np.float32)
    A[:, cols:] = np.nan  # the pitch padding is never read
    v = rng.standard_normal(cols)
    dA, dv = cg.DeviceArray.from_host(A), cg.DeviceArray.from_host(v)
    A64 = A[:, :cols].astype(np.float64)
    ref = A64 @ v
    bound = cols * 2.0 ** -53 * (np.abs(A64) @ np.abs(v))
    monkeypatch.delenv("CGX_MV_A32_PLAN", raising=False)
    out = cg.DeviceArray(rows, np.float64)
    cg.matVec(dA, dv, out, rows, cols, lda)
    y = out.to_host()
    assert np.all(np.abs(y - ref) <= bound), np.max(np.abs(y - ref) / bound)
    for R, U, nt in PLANS:
        monkeypatch.setenv("CGX_MV_A32_PLAN", f"R={R},U={U},nt={nt}")
        o2 = cg.DeviceArray(rows, np.float64)
        cg.matVec(dA, dv, o2, rows, cols, lda)
        assert np.array_equal(o2.to_host(), y), (R, U, nt)


# The order itself against its CPU statement (_matvec_order.py; shapes there), which the plan-against-plan
# test above cannot see.  (cols, lda, v's offset in doubles from the 32-byte grid): a v 16 bytes off it or a
# pitch that is no multiple of 4 floats sends every column through the scalar tail.
ORDER_A32 = [(c, (c + 3) & ~3, 0) for c in mo.A32_COLS] + [(517, 520, 2), (517, 519, 0)]


@pytest.mark.parametrize("plan", [None, "R=8,U=2,nt=8"])
@pytest.mark.parametrize("cols,lda,voff", ORDER_A32)
def test_kernel_level_matvec_is_the_documented_order(monkeypatch, cols, lda, voff, plan):
    """k_matvec_a32's row sums are the CPU emulation of the documented order bit for bit: four accumulators
    per lane over 256-column chunks, tail columns into .x, (x + y) + (z + w), the wave sum."""
    if plan:
        monkeypatch.setenv("CGX_MV_A32_PLAN", plan)
    else:
        monkeypatch.delenv("CGX_MV_A32_PLAN", raising=False)
    A, v = mo.a32_case(cols, lda)
    dA, dv, out = cg.DeviceArray.from_host(A), cg.DeviceArray.from_host(np.concatenate([np.zeros(voff), v])), \
        cg.DeviceArray(mo.ROWS, np.float64)
    L = cg.lib()
    assert L.cgx_matvec(A_F32, dA.ptr, lda, mo.ROWS, cols, dv.ptr + 8 * voff, out.ptr, None) == 0, L.cgx_last_error()
    assert L.cgx_dev_synchronize() == 0, L.cgx_last_error()
    vec_cols = mo.vec_cols_a32(cols, dA.ptr, dv.ptr + 8 * voff, lda)
    assert vec_cols == (cols & ~255 if voff == 0 and lda % 4 == 0 else 0)
    want = np.array(order_a32(cols, lda, vec_cols))
    got = out.to_host()
    assert np.array_equal(got, want), np.flatnonzero(got != want)


@functools.lru_cache(maxsize=None)
def order_a32(cols, lda, vec_cols):
    A, v = mo.a32_case(cols, lda)
    return mo.matvec_a32(A, v, cols, vec_cols)


def test_solver_plans_accepted_and_reported():
    """set_matvec_plan on an A_F32 context takes every instantiated plan and
    matvec_plan reports it back; each solves to the bar.  (The row sums are the
    same bits under every plan -- the kernel-level test above -- while the
    fused p.Ap adds per-block partials, whose number follows R, as
    k_matvec_f64's does.)"""
    n = 2304
    A32, A64, b, xo, K = hash_system(n, 1)
    with cg.Solver(n, flags=A_F32) as s:
        s.set_system(A32, b)
        for R, U, nt in PLANS:
            s.set_matvec_plan(R, U, nt)
            pl = s.matvec_plan()
            assert (pl["R"], pl["U"], pl["nt"]) == (R, U, nt) and pl["blocks"] >= 1
            x, st = s.solve(np.zeros(n), eps=1e-10)
            meets_bar(x, st.iterations, A64, b, xo, K)


@pytest.mark.parametrize("n,seed", [(1000, 2), (2304, 1), (5000, 9)])
def test_device_generator(n, seed):
    """generate_spd under CGX_A_F32 stores (float) of the fp64 generator's
    A_ij and b as in fp64 mode: the solve of spd_hash(n, seed)[0] rounded to
    float, bit for bit the set_system one."""
    A32, A64, b, xo, K = hash_system(n, seed)
    with cg.Solver(n, flags=A_F32) as s:
        s.generate_spd(seed)
        xg, stg = s.solve(None, eps=1e-10)
        s.set_system(A32, b)
        xs, sts = s.solve(np.zeros(n), eps=1e-10)
    meets_bar(xg, stg.iterations, A64, b, xo, K)
    assert sts.iterations == stg.iterations and np.array_equal(xg, xs)


def test_rows_in_pieces_and_timing():
    """set_rows over ragged row ranges of float rows with a host pitch > n gives
    set_system's bits; CGX_TIMING counts the matVec launches (x0 = 0: one per
    fixed-count iteration; any other x0: the initial A x0 too)."""
    A32, b32, _ = case("spd2048", np.float32)
    n = 2048
    b = b32.astype(np.float64)
    with cg.Solver(n, flags=A_F32) as s:
        s.set_system(A32, b)
        x_ref, st_ref = s.solve(np.zeros(n), eps=1e-10)
    wide = np.full((n, n + 24), np.float32(np.nan))
    wide[:, :n] = A32
    with cg.Solver(n, flags=A_F32 | cg.CGX_TIMING) as s:
        for lo, hi in ((0, 700), (700, 1500), (1500, 2048)):
            s.set_rows(lo, wide[lo:hi], b[lo:hi], np.zeros(hi - lo))
        x, st = s.solve(None, eps=1e-10)
        assert st.matvec_count >= st.iterations and st.matvec_ms > 0.0  # a gated solve may enqueue one launch past the stop
        s.reset_timing()
        s.solve(np.zeros(n), eps=-1.0, max_iter=5)
        assert s.stats().matvec_count == 5  # x0 = 0: no initial matVec
        s.reset_timing()
        s.solve(np.full(n, 0.5), eps=-1.0, max_iter=5)
        assert s.stats().matvec_count == 6  # initial residual + 5 iterations
    assert st.iterations == st_ref.iterations and np.array_equal(x, x_ref)


def test_byte_offsets_past_4gib():
    """n = 33024: A is 4.36 GB as float, generated on the device.  Three row
    blocks -- the first 128 rows, rows [32448, 32576) whose bytes straddle
    offset 2^32 in A, and the last 128 -- against the unrounded generator
    (oracle.hash_matvec_f64, no n^2 memory).  The residual of the float-stored
    system is below the stop (<= 1e-10 in norm, so below 1e-9 per entry with
    room) and |a32 - a64| <= 2^-24 |a64| entry by entry, hence
    |b_i - (A64 x)_i| <= 2^-24 (A64 |x|)_i + 1e-9 (the generator's entries are
    positive).  A kernel that indexes in 32 bits misses by O(1)."""
    n, seed = 33024, 42
    with cg.Solver(n, flags=A_F32) as s:
        s.generate_spd(seed)
        x, st = s.solve(None, eps=1e-10)
    assert st.converged == 1
    ax = np.abs(x)
    for row0 in (0, 32448, n - 128):
        _, b = oracle.spd_hash(n, seed=seed, row0=row0, nrows=128)
        got = oracle.hash_matvec_f64(n, x, seed, row0, 128)
        bound = 2.0 ** -24 * oracle.hash_matvec_f64(n, ax, seed, row0, 128) + 1e-9
        assert np.all(np.abs(b - got) <= bound), (row0, np.max(np.abs(b - got) / bound))


@pytest.mark.parametrize("n", [512, 4096])
def test_warmup_neutral(monkeypatch, n):
    """CGX_WARM=0 and the default: idle with no iterations after create, then x
    bit for bit and equal stats."""
    A32, b32, _ = case(f"spd{n}", np.float32)
    b = b32.astype(np.float64)
    res = {}
    for warm in (None, "0"):
        if warm is None:
            monkeypatch.delenv("CGX_WARM", raising=False)
        else:
            monkeypatch.setenv("CGX_WARM", warm)
        with cg.Solver(n, flags=A_F32) as s:
            st0 = s.stats()
            assert st0.iterations == 0 and st0.total_iterations == 0
            s.set_system(A32, b)
            x, _ = s.solve(None, eps=1e-10)
            st = s.stats()
        res[warm] = (x, (st.iterations, st.total_iterations, st.converged, st.rr))
    assert np.array_equal(res[None][0], res["0"][0]) and res[None][1] == res["0"][1]


@pytest.mark.parametrize("kw", [dict(flags=cg.CGX_F32_REF), dict(flags=cg.CGX_SYMMETRIC), dict(flags=cg.CGX_HOST_STREAM),
                                dict(flags=cg.CGX_PHASES), dict(devices=[0, 0]), dict(devices=[0]),
                                dict(rank=0, nranks=1, unique_id=b"\0" * 128), dict(poisson_m=16),
                                dict(poisson_m=16, devices=[0, 0])],
                         ids=["f32ref", "symmetric", "host_stream", "phases", "multi2", "multi1", "rank", "poisson",
                              "poisson_multi"])
def test_refused_combinations(kw):
    kw = dict(kw)
    flags = A_F32 | kw.pop("flags", 0)
    with pytest.raises(cg.CgxError, match="CGX_A_F32") as ei:
        cg.Solver(None if "poisson_m" in kw else 512, flags=flags, **kw)
    assert ei.value.code == -1


@pytest.mark.parametrize("plan", [(2, 8, 8), (4, 4, 0), (4, 4, 1), (8, 4, 8), (3, 4, 8), (1, 2, 2)])
def test_plan_not_instantiated_is_refused(plan):
    with cg.Solver(512, flags=A_F32) as s:
        before = s.matvec_plan()
        with pytest.raises(cg.CgxError) as ei:
            s.set_matvec_plan(*plan)
        assert ei.value.code == -1
        assert s.matvec_plan() == before


ONE_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="0")


def test_cli_a_fp32(tmp_path):
    """cg_hip --a-fp32 on generateSPDmatrix(512) written as the MATLAB script
    writes it: A parsed as initialize() does (float), b and x0 as double; the
    reference's lines, and x within 1e-10 of the oracle on float32(the written
    decimals) widened.  The refused combinations exit 2."""
    n = 512
    A, b = oracle.spd_matlab(n, np.float64)
    for name, arr, dec in (("A.txt", A, 4), ("b.txt", b, 4), ("x0.txt", np.zeros(n), 1)):
        oracle.write_text(str(tmp_path / name), arr, dec)
    paths = [str(tmp_path / f) for f in ("A.txt", "b.txt", "x0.txt")]
    r = subprocess.run([cg.CLI_PATH, "--a-fp32", "--eps", "1e-10", "--print-x", "--stats", *paths],
                       capture_output=True, text=True, timeout=300, env=ONE_GPU)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"Computing cg of matrix size : {n * n}" in r.stdout      # serialConjugate.c:58
    assert "average clock execution time in seconds:" in r.stdout    # serialConjugate.c:250
    x = np.array([float(v) for v in r.stdout.strip().splitlines()[-n:]])
    A64 = cg.read_text(paths[0], n * n, np.float32).astype(np.float64).reshape(n, n)
    bw = cg.read_text(paths[1], n, np.float64)
    xo, so = oracle.cg_f64(A64, bw, np.zeros(n), eps=1e-10)
    assert f"iterations: {so.iterations} converged: 1" in r.stdout
    assert np.linalg.norm(x - xo) <= 1e-10 * np.linalg.norm(xo)
    for extra in (["--fp32-ref"], ["--symmetric"], ["--gpus", "2"]):
        r = subprocess.run([cg.CLI_PATH, "--a-fp32", *extra, *paths], capture_output=True, text=True, env=ONE_GPU)
        assert r.returncode == 2 and len(r.stderr.strip().splitlines()) == 1, (extra, r.returncode, r.stderr)
    r = subprocess.run([cg.CLI_PATH, "--spd", "1000", "--seed", "2", "--a-fp32", "--eps", "1e-10", "--stats"],
                       capture_output=True, text=True, timeout=300, env=ONE_GPU)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"iterations: {hash_system(1000, 2)[4]} converged: 1" in r.stdout
