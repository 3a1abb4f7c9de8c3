"""One-flip local search stage of the QUBO objective (Island::local_search on
BINARY / OBJ_QUBO, csrc/kernels/qubo_ls.hip, csrc/cpu/cpu_qubo.cpp
qubo_local_search).

The contract (csrc/include/pga/qubo_ops.hpp): with q = the rounded int8
matrix, g_p = sum_j (q[p][j] + q[j][p]) x_j, flipping bit p changes
f = x^T q x by (1 - 2 x_p) g_p + q[p][p]; one move takes the largest gain in
score over p < L, ties to the smallest p, and flips when it is > 0.  Exact
integers end to end: CPU tests pin the CPU backend against a plain numpy int64
oracle, GPU tests pin the kernel against the CPU backend bit for bit."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import libpga_amd as pga
from libpga_amd import models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "build", "libpga.so")


# ------------------------------------------------------------------ oracle ---
def gains(q, s, X):
    """[S, L] int64 gains in score of every single-bit flip of every row."""
    W = q + q.T
    return s * ((1 - 2 * X) * (X @ W) + np.diag(q)[None, :])


def fvalue(q, X):
    return np.einsum("si,ij,sj->s", X, q, X)


def score_of(q, sign, X):
    """What MODE_EVAL stores: sign * (float)(int32) f."""
    return (np.float32(sign) * fvalue(q, X).astype(np.int32).astype(np.float32)).astype(np.float32)


def oracle(q, s, X0, cap, snaps=()):
    """Best-improvement one-flip, up to `cap` moves per row, one row at a time.
    Returns the final rows, the moves each made, whether each stopped by
    itself, and the rows after min(m, its own) moves for every m in snaps."""
    S, L = X0.shape
    W = q + q.T
    d = np.diag(q)
    final, made, stopped = X0.copy(), np.zeros(S, dtype=np.int64), np.zeros(S, dtype=bool)
    out = {m: X0.copy() for m in snaps}
    for r in range(S):
        x = X0[r].copy()
        g = W @ x
        for m in range(cap + 1):
            if m in snaps:
                out[m][r] = x
            if m == cap:
                break
            gain = s * ((1 - 2 * x) * g + d)
            p = int(gain.argmax())  # the first maximum: the smallest p
            if not gain[p] > 0:
                stopped[r] = True
                break
            g += (1 - 2 * x[p]) * W[:, p]
            x[p] ^= 1
            made[r] += 1
        assert np.array_equal(g, W @ x)
        final[r] = x
        for m in snaps:
            if m > made[r]:
                out[m][r] = x
    return final, made, stopped, out


def qmat(p):
    q = p.Q.numpy().astype(np.int64)
    return q, (1 if p.sign > 0 else -1)


def bits(ga):
    return ga.genomes().cpu().numpy().astype(np.int64)


ORACLE_CASES = [(5, -128, 127, False), (64, -8, 8, True), (65, -128, 127, False), (100, -8, 8, False),
                (200, -128, 127, True), (1000, -128, 127, False)]


@functools.lru_cache(maxsize=None)
def oracle_case(L, lo, hi, mx):
    p = M.QUBO.random(L, seed=2, lo=lo, hi=hi, maximize=mx)
    q, s = qmat(p)
    assert not np.array_equal(q, q.T)
    ga = pga.GeneticAlgorithm(p, 64, seed=4, device="cpu")
    X0 = bits(ga)
    final, made, stopped, snaps = oracle(q, s, X0, 4 * L, snaps=(1, 3, 256))
    snaps[4 * L] = final
    return p, q, s, X0, snaps, made, stopped


@pytest.mark.parametrize("L,lo,hi,mx", ORACLE_CASES)
@pytest.mark.parametrize("moves", [1, 3, "4L"])
def test_oracle_equality(L, lo, hi, mx, moves):
    p, q, s, X0, snaps, made, stopped = oracle_case(L, lo, hi, mx)
    m = 4 * L if moves == "4L" else moves
    ga = pga.GeneticAlgorithm(p, 64, seed=4, device="cpu")
    assert np.array_equal(bits(ga), X0)
    ga.local_search(m, 1.0)
    want = snaps[m]
    assert np.array_equal(bits(ga), want)
    assert np.array_equal(ga.scores.numpy(), score_of(q, p.sign, want))
    assert ga.generation == 0
    assert ga.best_score() == float(ga.scores.max())
    if moves == "4L":
        # the oracle stopped by itself on every row, inside the cap: no hidden truncation
        assert stopped.all() and made.max() < m
        assert gains(q, s, bits(ga)).max() <= 0  # one-flip optimal


def set_rows(ga, X):
    ga.rows.copy_(ga.problem.encode(torch.as_tensor(X, dtype=torch.uint8), int(ga.island.row_words)))
    ga.evaluate()


def test_known_answer_tie_takes_lowest_bit():
    p = M.QUBO(-torch.eye(8, dtype=torch.int64), maximize=False)
    ga = pga.GeneticAlgorithm(p, 4, seed=1, device="cpu")
    set_rows(ga, np.zeros((4, 8)))
    assert ga.scores.tolist() == [0.0] * 4
    ga.local_search(3, 1.0)  # every bit gains 1: bits 0, 1, 2 in that order
    assert bits(ga).tolist() == [[1, 1, 1, 0, 0, 0, 0, 0]] * 4
    assert ga.scores.tolist() == [3.0] * 4


@pytest.mark.parametrize("mx", [False, True])
def test_known_answer_diagonal_reaches_the_optimum(mx):
    gen = torch.Generator().manual_seed(3)
    d = torch.randint(1, 128, (64,), generator=gen) * (2 * torch.randint(0, 2, (64,), generator=gen) - 1)
    p = M.QUBO(torch.diag(d), maximize=mx)
    ga = pga.GeneticAlgorithm(p, 32, seed=2, device="cpu")
    ga.local_search(64, 1.0)
    s = 1 if mx else -1
    want = (s * d.numpy() > 0).astype(np.int64)
    assert np.array_equal(bits(ga), np.tile(want, (32, 1)))
    assert ga.scores.tolist() == [float(np.abs(d.numpy()[want == 1]).sum())] * 32


def test_known_answer_maxcut_triangle_with_pendant():
    w = torch.zeros(4, 4, dtype=torch.int64)
    for i, j in [(0, 1), (1, 2), (0, 2), (2, 3)]:
        w[i, j] = w[j, i] = 1
    p = M.MaxCut(w)
    ga = pga.GeneticAlgorithm(p, 4, seed=1, device="cpu")
    set_rows(ga, np.zeros((4, 4)))
    ga.local_search(8, 1.0)
    assert ga.scores.tolist() == [3.0] * 4
    assert p.cut_value(ga.genomes()).tolist() == [3] * 4
    assert bits(ga).tolist() == [[0, 0, 1, 0]] * 4  # the degree-3 vertex gains most; then no flip gains


@pytest.mark.parametrize("prob", ["qubo", "maxcut"])
def test_invariants(prob):
    p = {"qubo": lambda: M.QUBO.random(50), "maxcut": lambda: M.MaxCut.random_graph(50)}[prob]()
    ga = pga.GeneticAlgorithm(p, 200, seed=3, device="cpu")
    r0, s0 = ga.rows.clone(), ga.scores.clone()
    x0 = bits(ga)
    ga.local_search(2, 0.5)
    r1, s1 = ga.rows.clone(), ga.scores.clone()
    x1 = bits(ga)
    assert (s1 >= s0).all()
    same = s1 == s0
    assert 0 < int(same.sum()) < 200
    assert torch.equal(r1[same], r0[same])
    nd = (x1 != x0).sum(axis=1)
    assert set(nd[~same.numpy()].tolist()) <= {1, 2} and (nd[same.numpy()] == 0).all()
    assert ga.best_score() == float(s1.max())
    # bits >= L stay zero: re-encoding the decoded genomes gives the rows back
    assert torch.equal(p.encode(ga.genomes(), int(ga.island.row_words)), r1)
    ga.evaluate()
    assert torch.equal(ga.scores, s1) and torch.equal(ga.rows, r1)


def changed_rows(ga, moves, prob):
    r0 = ga.rows.clone()
    ga.local_search(moves, prob)
    return (ga.rows != r0).any(dim=1)


def test_selection():
    p = M.QUBO.random(16, seed=1)
    new = lambda: pga.GeneticAlgorithm(p, 4096, seed=9, device="cpu")  # noqa: E731
    ga = new()
    r0, s0 = ga.rows.clone(), ga.scores.clone()
    ga.local_search(1, 0.0)
    assert torch.equal(ga.rows, r0) and torch.equal(ga.scores, s0)
    part = changed_rows(ga, 1, 0.25)
    full = changed_rows(new(), 1, 1.0)
    assert not (part & ~full).any()  # a subset of what prob = 1 changes
    assert 0.15 <= float(part.sum()) / float(full.sum()) <= 0.35
    # the same generation selects the same individuals (also on a second call) ...
    again = new()
    assert torch.equal(changed_rows(again, 1, 0.25), part)
    assert not (changed_rows(again, 1, 0.25) & ~part).any()
    # ... another generation does not
    later = new()
    later.run(1)
    assert not torch.equal(changed_rows(later, 1, 0.25), part)


LOOP_KW = dict(seed=5, crossover="uniform", mutation="bit_flip", mutation_rate=0.05, elitism=1)
LS_KW = dict(local_search="one_flip", ls_moves=2, ls_prob=0.5)


def test_loop_equals_manual_stages():
    p = M.MaxCut.random_graph(40)
    a = pga.GeneticAlgorithm(p, 256, device="cpu", **LS_KW, **LOOP_KW)
    b = pga.GeneticAlgorithm(p, 256, device="cpu", **LOOP_KW)
    assert a.run(3) == 3
    for _ in range(3):
        b.run(1)
        b.local_search(2, 0.5)
    assert a.generation == b.generation == 3
    assert torch.equal(a.rows, b.rows) and torch.equal(a.scores, b.scores)
    # set_operators switches the option on as well, and the stage defaults to the operators' values
    b.set_operators(**LS_KW)
    a.run(1)
    b.run(1)
    assert torch.equal(a.rows, b.rows) and torch.equal(a.scores, b.scores)
    c = pga.GeneticAlgorithm(p, 256, device="cpu", ls_moves=2, ls_prob=0.5, **LOOP_KW)
    d = pga.GeneticAlgorithm(p, 256, device="cpu", **LOOP_KW)
    c.local_search()
    d.local_search(2, 0.5)
    assert torch.equal(c.rows, d.rows)


def test_loop_history_describes_the_population_after_the_stage():
    p = M.MaxCut.random_graph(40)
    ga = pga.GeneticAlgorithm(p, 256, device="cpu", **LS_KW, **LOOP_KW)
    ga.record_history()
    bests = []
    for _ in range(3):
        ga.run(1)
        bests.append(ga.best_score())
    h = ga.history()
    assert h.shape[0] == 3 and h[:, 1].tolist() == bests


def test_loop_checkpoint_resume(tmp_path):
    p = M.MaxCut.random_graph(40)
    kw = dict(device="cpu", **LS_KW, **LOOP_KW)
    a = pga.GeneticAlgorithm(p, 256, **kw)
    a.run(2)
    a.save(str(tmp_path / "ls.ckpt"))
    a.run(2)
    b = pga.GeneticAlgorithm(p, 256, **kw)
    b.load(str(tmp_path / "ls.ckpt"))
    b.run(2)
    assert b.generation == 4
    assert torch.equal(a.rows, b.rows) and torch.equal(a.scores, b.scores)


class TorchQUBO(M.QUBO):
    def __init__(self, Q):
        super().__init__(Q)
        self.torch_objective = lambda g: self.reference_fitness(g)


def test_errors():
    for p in (M.OneMax(64), M.Knapsack01.random(32), M.TSP.random_euclidean(12)):
        with pytest.raises(Exception, match="QUBO"):
            pga.GeneticAlgorithm(p, 64, device="cpu", local_search="one_flip")
        with pytest.raises(Exception, match="QUBO"):
            pga.GeneticAlgorithm(p, 64, device="cpu").set_operators(local_search="one_flip")
    with pytest.raises(Exception, match="PERMUTATION"):
        pga.GeneticAlgorithm(M.QUBO.random(12), 64, device="cpu", local_search="two_opt")
    tq = TorchQUBO(M.QUBO.random(12).Q)
    with pytest.raises(Exception, match="torch objective"):
        pga.GeneticAlgorithm(tq, 64, device="cpu").local_search(1, 1.0)
    with pytest.raises(Exception, match="torch objective"):
        pga.GeneticAlgorithm(tq, 64, device="cpu", local_search="one_flip")
    with pytest.raises(Exception, match="unknown local search"):
        pga.GeneticAlgorithm(M.QUBO.random(12), 64, device="cpu", local_search="three_opt")
    with pytest.raises(Exception, match="LocalIslands"):
        pga.parallel.LocalIslands(M.QUBO.random(12), 2, 64, device="cpu", local_search="one_flip")


# ------------------------------------------------------------------- C API ---
@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "build/libpga.so not built (python tools/build.py)"
    L = C.CDLL(LIB)
    vp = C.c_void_p
    L.pga_init_device.restype = vp
    L.pga_init_device.argtypes = [C.c_int]
    L.pga_deinit.argtypes = [vp]
    L.pga_set_seed.argtypes = [vp, C.c_uint64]
    L.pga_set_quiet.argtypes = [vp, C.c_int]
    L.pga_set_abort_on_error.argtypes = [vp, C.c_int]
    L.pga_last_error.restype = C.c_char_p
    L.pga_create_population_ext.restype = vp
    L.pga_create_population_ext.argtypes = [vp, C.c_ulong, C.c_uint, C.c_int]
    L.pga_set_objective_builtin.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_float), C.c_size_t,
                                            C.POINTER(C.c_float), C.c_size_t, C.c_int, C.c_float, C.c_float]
    L.pga_set_operators.argtypes = [vp, vp, C.c_int, C.c_uint, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float,
                                    C.c_uint]
    L.pga_run.argtypes = [vp, C.c_uint]
    L.pga_get_scores.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.pga_get_genome.argtypes = [vp, vp, C.c_ulong, C.c_void_p]
    L.pga_row_bytes.restype = C.c_size_t
    L.pga_row_bytes.argtypes = [vp]
    L.pga_generation.argtypes = [vp]
    L.pga_set_local_search.argtypes = [vp, vp, C.c_int, C.c_uint, C.c_float]
    L.pga_local_search.argtypes = [vp, vp]
    return L


def capi_pop(lib, prob, S, sign):
    p = lib.pga_init_device(-1)
    assert p
    lib.pga_set_seed(p, 5)
    lib.pga_set_quiet(p, 1)
    lib.pga_set_abort_on_error(p, 0)
    pop = lib.pga_create_population_ext(p, S, prob.length, 0)  # PGA_BINARY
    flat = prob.Q.reshape(-1).tolist()
    arr = (C.c_float * len(flat))(*flat)
    assert lib.pga_set_objective_builtin(p, pop, 5, arr, len(flat), None, 0, 0, sign, 0.0) == 0  # PGA_OBJ_QUBO
    # tournament-2, uniform crossover, bit-flip at 0.05, one elite: LOOP_KW
    assert lib.pga_set_operators(p, pop, 0, 2, 0, 1.0, 0, 0.05, 0.1, 1) == 0
    return p, pop


def capi_state(lib, p, pop, S):
    sc = (C.c_float * S)()
    assert lib.pga_get_scores(p, pop, sc) == 0
    rb = lib.pga_row_bytes(pop)
    rows = torch.empty(S, rb // 4, dtype=torch.int32)
    for i in range(S):
        assert lib.pga_get_genome(p, pop, i, C.c_void_p(rows[i].data_ptr())) == 0
    return rows, torch.tensor(list(sc))


def test_capi_matches_python(lib):
    prob = M.MaxCut.random_graph(40)
    p, pop = capi_pop(lib, prob, 256, 1.0)
    ga = pga.GeneticAlgorithm(prob, 256, device="cpu", **LS_KW, **LOOP_KW)
    assert lib.pga_set_local_search(p, pop, 2, 2, 0.5) == 0
    lib.pga_run(p, 2)
    ga.run(2)
    assert lib.pga_generation(pop) == 2
    rows, sc = capi_state(lib, p, pop, 256)
    assert torch.equal(rows, ga.rows) and torch.equal(sc, ga.scores)
    assert lib.pga_local_search(p, pop) == 0  # the values set above
    ga.local_search()
    rows, sc = capi_state(lib, p, pop, 256)
    assert torch.equal(rows, ga.rows) and torch.equal(sc, ga.scores)
    assert lib.pga_generation(pop) == 2
    assert lib.pga_set_local_search(p, pop, 7, 1, 1.0) != 0
    assert b"unknown local search" in lib.pga_last_error()
    lib.pga_deinit(p)


def test_capi_zero_sign_fails(lib):
    prob = M.QUBO.random(20)
    p, pop = capi_pop(lib, prob, 64, 0.0)
    assert lib.pga_local_search(p, pop) != 0
    assert b"obj_f0" in lib.pga_last_error()
    lib.pga_deinit(p)


# --------------------------------------------------------------------- GPU ---
def instance(kind, L):
    return M.QUBO.random(L, seed=2, lo=-128, hi=127) if kind == "qubo" else M.MaxCut.random_graph(L)


def assert_same(g, c):
    torch.cuda.synchronize()
    assert torch.equal(g.rows.cpu(), c.rows)
    assert torch.equal(g.scores.cpu(), c.scores)
    assert g.best_score() == c.best_score() and g.best_index() == c.best_index()


GPU_CASES = [(L, S, moves, 1.0) for L, S in [(5, 64), (64, 333), (65, 1000), (100, 500), (200, 300), (512, 130),
                                             (1000, 64), (1024, 70), (64, 1)]
             for moves in (1, 5)] + [(65, 1000, 5, 0.3)]
# smaller shares: the kernel draws runs of 3 x 64 and 4 x 64 individuals per wave
GPU_CASES += [(65, 1000, 2, 0.1), (200, 3000, 3, 0.05), (1000, 700, 2, 0.02)]


@functools.lru_cache(maxsize=None)
def cpu_stage(kind, L, S, moves, prob):
    """The CPU backend's population before and after the stage (computed once, never modified)."""
    c = pga.GeneticAlgorithm(instance(kind, L), S, seed=5, device="cpu")
    r0 = c.rows.clone()
    c.local_search(moves, prob)
    return c, r0


@pytest.mark.gpu
@pytest.mark.parametrize("L,S,moves,prob", GPU_CASES)
@pytest.mark.parametrize("kind", ["qubo", "maxcut"])
def test_gpu_bitexact(kind, L, S, moves, prob):
    c, r0 = cpu_stage(kind, L, S, moves, prob)
    g = pga.GeneticAlgorithm(instance(kind, L), S, seed=5, device="cuda:0")
    assert torch.equal(g.rows.cpu(), r0)
    g.local_search(moves, prob)
    assert_same(g, c)
    assert (c.rows != r0).any()


@pytest.mark.gpu
def test_gpu_scores_beyond_2_24():
    """|f| ~ 3e7 > 2^24: the new score comes from the integer f, not from the stored float."""
    p = M.QUBO(torch.full((1024, 1024), 127, dtype=torch.int64), maximize=True)
    g = pga.GeneticAlgorithm(p, 64, seed=5, device="cuda:0")
    c = pga.GeneticAlgorithm(p, 64, seed=5, device="cpu")
    assert float(c.scores.abs().max()) > 2 ** 24
    g.local_search(3, 1.0)
    c.local_search(3, 1.0)
    assert_same(g, c)
    r1, s1 = g.rows.clone(), g.scores.clone()
    g.evaluate()
    torch.cuda.synchronize()
    assert torch.equal(g.rows, r1) and torch.equal(g.scores, s1)


@pytest.mark.gpu
@pytest.mark.parametrize("elitism", [1, 2])
def test_gpu_loop_bitexact(elitism):
    p = M.MaxCut.random_graph(128)
    kw = dict(seed=5, crossover="uniform", mutation="bit_flip", mutation_rate=0.05, elitism=elitism, **LS_KW)
    g = pga.GeneticAlgorithm(p, 1000, device="cuda:0", **kw)
    c = pga.GeneticAlgorithm(p, 1000, device="cpu", **kw)
    g.record_history()
    for _ in range(3):
        assert_same(g, c)
        g.run(1)
        c.run(1)
    assert_same(g, c)
    assert g.history()[:, 1].tolist()[-1] == c.best_score()


@pytest.mark.gpu
def test_gpu_oracle_to_convergence():
    p, q, s, X0, snaps, made, stopped = oracle_case(64, -8, 8, True)
    g = pga.GeneticAlgorithm(p, 64, seed=4, device="cuda:0")
    g.local_search(256, 1.0)
    torch.cuda.synchronize()
    want = snaps[256]
    assert np.array_equal(bits(g), want)
    assert np.array_equal(g.scores.cpu().numpy(), score_of(q, p.sign, want))
