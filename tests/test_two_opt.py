"""2-opt local search stage of the PERMUTATION encoding (Island::local_search,
csrc/kernels/perm_ls.hip, csrc/cpu/cpu_perm.cpp perm_local_search).

The contract (csrc/include/pga/perm_ops.hpp): one move takes, over every pair
(i, j) with i + 2 <= j < L (closed tours: not (0, L - 1)), the largest
gain = (d(a,b) + d(c,e)) - (d(a,c) + d(b,e)) in f32, ties to the smallest i
then j, and reverses t[i+1 .. j] when it is > 0; an open path is a closed tour
whose closing edge has length 0.  CPU tests pin the CPU backend against a
plain numpy oracle on integer matrices (every f32 sum exact); GPU tests pin
the kernel against the CPU backend bit for bit."""
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


def is_perm(t):
    return bool((torch.sort(t, dim=1).values == torch.arange(t.shape[1])).all())


# ------------------------------------------------------------------ oracle ---
def gains(D, t, open_path):
    """[S, L, L] f32 gains of every pair of every tour; -inf where (i, j) is no pair."""
    S, L = t.shape
    nx = np.roll(t, -1, axis=1)
    el = D[t, nx]
    dac = D[t[:, :, None], t[:, None, :]]
    dbe = D[nx[:, :, None], nx[:, None, :]]
    if open_path:  # the closing edge has length 0
        el[:, L - 1] = 0
        dbe[:, :, L - 1] = 0
    g = (el[:, :, None] + el[:, None, :]) - (dac + dbe)
    assert g.dtype == np.float32
    i, j = np.meshgrid(np.arange(L), np.arange(L), indexing="ij")
    pair = j >= i + 2
    if not open_path:
        pair &= ~((i == 0) & (j == L - 1))
    g[:, ~pair] = -np.inf
    return g


def oracle(D, tours, open_path, cap, snaps=()):
    """Best-improvement 2-opt, up to `cap` moves per tour, one tour at a time.
    Returns the final tours, the moves each made, whether each stopped by
    itself, and the tours after min(m, its own) moves for every m in snaps.
    P[i, j] = d(t[i], t[j]) follows the reversals (checked at the end), so a
    move costs a few passes over one L x L matrix."""
    S, L = tours.shape
    ar = np.arange(L)
    i, j = np.meshgrid(ar, ar, indexing="ij")
    pair = j >= i + 2
    if not open_path:
        pair &= ~((i == 0) & (j == L - 1))
    final, made, stopped = tours.copy(), np.zeros(S, dtype=np.int64), np.zeros(S, dtype=bool)
    out = {m: tours.copy() for m in snaps}
    for s in range(S):
        t = tours[s].copy()
        P = D[t][:, t].copy()
        Q = np.zeros((L, L), dtype=np.float32)  # Q[i, j] = d(t[i+1], t[(j+1) % L])
        for m in range(cap + 1):
            if m in snaps:
                out[m][s] = t
            if m == cap:
                break
            el = P[ar, (ar + 1) % L].copy()
            Q[:-1, :-1] = P[1:, 1:]
            Q[:-1, -1] = P[1:, 0]
            if open_path:  # the closing edge has length 0
                el[L - 1] = 0
                Q[:, -1] = 0
            g = np.where(pair, (el[:, None] + el[None, :]) - (P + Q), -np.inf)
            assert g.dtype == np.float32
            k = int(g.argmax())  # the first maximum: smallest i, then smallest j
            if not g.flat[k] > 0:
                stopped[s] = True
                break
            a, b = divmod(k, L)
            t[a + 1:b + 1] = t[a + 1:b + 1][::-1].copy()
            P[a + 1:b + 1, :] = P[a + 1:b + 1, :][::-1].copy()
            P[:, a + 1:b + 1] = P[:, a + 1:b + 1][:, ::-1].copy()
            made[s] += 1
        assert np.array_equal(P, D[t][:, t])
        final[s] = t
        for m in snaps:
            if m > made[s]:
                out[m][s] = t
    return final, made, stopped, out


def length(D, t, open_path):
    nx = np.roll(t, -1, axis=1)
    el = D[t, nx]
    if open_path:
        el = el[:, :-1]
    return el.astype(np.float64).sum(axis=1)


ORACLE_CASES = [(5, False), (9, False), (9, True), (64, False), (100, True), (257, False)]


@functools.lru_cache(maxsize=None)
def oracle_case(n, op):
    p = M.TSP.random_integer_euclidean(n, seed=2, open_path=op)
    D = p.dist.numpy()
    assert np.array_equal(D, np.round(D)) and np.array_equal(D, D.T)
    ga = pga.GeneticAlgorithm(p, 64, seed=4, device="cpu")
    t0 = ga.genomes().numpy().astype(np.int64)
    final, made, stopped, snaps = oracle(D, t0, op, 4 * n, snaps=(1, 3))
    snaps[4 * n] = final
    return p, D, t0, snaps, made, stopped


@pytest.mark.parametrize("n,op", ORACLE_CASES)
@pytest.mark.parametrize("moves", [1, 3, "4n"])
def test_oracle_equality(n, op, moves):
    p, D, t0, snaps, made, stopped = oracle_case(n, op)
    m = 4 * n if moves == "4n" else moves
    ga = pga.GeneticAlgorithm(p, 64, seed=4, device="cpu")
    assert np.array_equal(ga.genomes().numpy(), t0)
    ga.local_search(m, 1.0)
    want = snaps[m]
    assert np.array_equal(ga.genomes().numpy(), want)
    assert np.array_equal(ga.scores.numpy(), (-length(D, want, op)).astype(np.float32))
    assert ga.generation == 0
    assert ga.best_score() == float(ga.scores.max())
    if moves == "4n":
        # the oracle stopped by itself, well inside the cap
        assert stopped.all() and made.max() < m
        assert gains(D, ga.genomes().numpy(), op).max() <= 0  # 2-optimal
        assert (length(D, want, op) <= length(D, t0, op)).all()


def set_rows(ga, tours):
    ga.rows.copy_(ga.problem.encode(torch.as_tensor(tours), int(ga.island.row_words)))
    ga.evaluate()


def test_known_answer_unit_square():
    xy = torch.tensor([[0., 0.], [1., 0.], [1., 1.], [0., 1.]])
    for p in (M.TSPEuclidean(xy), M.TSP(torch.cdist(xy.double(), xy.double()).float())):
        ga = pga.GeneticAlgorithm(p, 4, seed=1, device="cpu")
        set_rows(ga, [[0, 2, 1, 3]] * 4)
        assert torch.allclose(ga.scores, torch.full((4,), -(2 + 2 * 2 ** 0.5)))
        ga.local_search(1, 1.0)
        assert ga.genomes().tolist() == [[0, 1, 2, 3]] * 4  # pair (0, 2): t[1..2] reversed
        assert ga.scores.tolist() == [-4.0] * 4
        ga.local_search(5, 1.0)  # 2-optimal: nothing moves
        assert ga.genomes().tolist() == [[0, 1, 2, 3]] * 4


def test_known_answer_tie_takes_first_pair():
    """Every distance 10 but d(1, 4) = 5: on the identity tour the pairs
    (0, 3) (new edge b-e = 1-4) and (1, 4) (new edge a-c = 1-4) both gain 5,
    every other pair gains 0: the first one in (i, j) order is taken."""
    d = 10.0 * (1 - torch.eye(8))
    d[1, 4] = d[4, 1] = 5.0
    p = M.TSP(d)
    tour = list(range(8))
    g = gains(p.dist.numpy(), np.array([tour]), False)[0]
    assert g[0, 3] == g[1, 4] == g.max() == 5 and int((g == 5).sum()) == 2
    ga = pga.GeneticAlgorithm(p, 2, seed=1, device="cpu")
    set_rows(ga, [tour] * 2)
    ga.local_search(1, 1.0)
    assert ga.genomes().tolist() == [[0, 3, 2, 1, 4, 5, 6, 7]] * 2  # t[1..3] reversed, not t[2..4]
    assert ga.scores.tolist() == [-75.0] * 2


@pytest.mark.parametrize("prob", ["matrix", "euc", "open"])
def test_invariants_float_instance(prob):
    p = {"matrix": lambda: M.TSP.random_euclidean(50), "euc": lambda: M.TSPEuclidean.random(50),
         "open": lambda: M.TSP.random_euclidean(50, open_path=True)}[prob]()
    ga = pga.GeneticAlgorithm(p, 200, seed=3, device="cpu")
    r0, s0 = ga.rows.clone(), ga.scores.clone()
    ga.local_search(2, 0.5)
    r1, s1 = ga.rows.clone(), ga.scores.clone()
    assert is_perm(ga.genomes())
    assert (s1 >= s0).all()
    same = s1 == s0
    assert 0 < int(same.sum()) < 200
    assert torch.equal(r1[same], r0[same])
    assert (r1[~same] != r0[~same]).any(dim=1).all()
    assert ga.best_score() == float(s1.max())
    ga.evaluate()
    assert torch.equal(ga.scores, s1) and torch.equal(ga.rows, r1)


def changed_rows(ga, moves, prob):
    r0 = ga.rows.clone()
    ga.local_search(moves, prob)
    return (ga.rows != r0).any(dim=1)


def test_selection():
    p = M.TSPEuclidean.random(16, seed=1)
    new = lambda: pga.GeneticAlgorithm(p, 4096, seed=9, device="cpu")  # noqa: E731
    ga = new()
    r0, s0 = ga.rows.clone(), ga.scores.clone()
    ga.local_search(1, 0.0)
    assert torch.equal(ga.rows, r0) and torch.equal(ga.scores, s0)
    part = changed_rows(ga, 1, 0.25)
    full = changed_rows(new(), 1, 1.0)
    assert not (part & ~full).any()  # a subset of what prob = 1 changes
    assert 0.15 <= float(part.float().mean()) <= 0.35
    # the same generation selects the same individuals (also on a second call) ...
    again = new()
    assert torch.equal(changed_rows(again, 1, 0.25), part)
    assert not (changed_rows(again, 1, 0.25) & ~part).any()
    # ... another generation does not
    later = new()
    later.run(1)
    assert not torch.equal(changed_rows(later, 1, 0.25), part)


LOOP_KW = dict(seed=5, crossover="ox", mutation="inversion", mutation_rate=0.4, elitism=1)


def test_loop_equals_manual_stages():
    p = M.TSP.random_euclidean(40, seed=2)
    a = pga.GeneticAlgorithm(p, 256, device="cpu", local_search="two_opt", ls_moves=2, ls_prob=0.5, **LOOP_KW)
    a.record_history()
    b = pga.GeneticAlgorithm(p, 256, device="cpu", **LOOP_KW)
    assert a.run(3) == 3
    for _ in range(3):
        b.run(1)
        b.local_search(2, 0.5)
    assert a.generation == b.generation == 3
    assert torch.equal(a.rows, b.rows) and torch.equal(a.scores, b.scores)
    # set_operators switches the option on as well, and the stage defaults to the operators' values
    b.set_operators(local_search="two_opt", ls_moves=2, ls_prob=0.5)
    a.run(1)
    b.run(1)
    assert torch.equal(a.rows, b.rows) and torch.equal(a.scores, b.scores)
    c = pga.GeneticAlgorithm(p, 256, device="cpu", ls_moves=2, ls_prob=0.5, **LOOP_KW)
    d = pga.GeneticAlgorithm(p, 256, device="cpu", **LOOP_KW)
    c.local_search()
    d.local_search(2, 0.5)
    assert torch.equal(c.rows, d.rows)


def test_loop_history_describes_the_population_after_the_stage():
    p = M.TSP.random_euclidean(40, seed=2)
    ga = pga.GeneticAlgorithm(p, 256, device="cpu", local_search="two_opt", ls_moves=2, ls_prob=0.5, **LOOP_KW)
    ga.record_history()
    bests = []
    for _ in range(3):
        ga.run(1)
        bests.append(ga.best_score())
    h = ga.history()
    assert h.shape[0] == 3 and h[:, 1].tolist() == bests


def test_loop_checkpoint_resume(tmp_path):
    p = M.TSP.random_euclidean(40, seed=2)
    kw = dict(device="cpu", local_search="two_opt", ls_moves=2, ls_prob=0.5, **LOOP_KW)
    a = pga.GeneticAlgorithm(p, 256, **kw)
    a.run(2)
    a.save(str(tmp_path / "ls.ckpt"))
    a.run(2)
    b = pga.GeneticAlgorithm(p, 256, **kw)
    b.load(str(tmp_path / "ls.ckpt"))
    b.run(2)
    assert b.generation == 4
    assert torch.equal(a.rows, b.rows) and torch.equal(a.scores, b.scores)


def test_loop_target_stops():
    p = M.TSPEuclidean.circle(24)
    ga = pga.GeneticAlgorithm(p, 256, device="cpu", local_search="two_opt", ls_moves=48, **LOOP_KW)
    opt = float(p.tour_length(torch.arange(24)[None])[0])
    done = ga.run(200, target=-1.0001 * opt, check_every=1)
    assert done < 200 and ga.best_score() >= -1.0001 * opt


def test_loop_circle_reaches_the_hull():
    """A 2-optimal tour of points in convex position is their hull: with 48 >=
    the moves a 24-city tour needs, ten memetic generations hold the optimum;
    the plain GA is nowhere near after ten."""
    p = M.TSPEuclidean.circle(24)
    opt = float(p.tour_length(torch.arange(24)[None])[0])
    on = pga.GeneticAlgorithm(p, 256, device="cpu", local_search="two_opt", ls_moves=48, **LOOP_KW)
    off = pga.GeneticAlgorithm(p, 256, device="cpu", **LOOP_KW)
    on.run(10)
    off.run(10)
    assert -on.best_score() <= 1.0001 * opt
    assert not (-off.best_score() <= 1.0001 * opt)


class TorchTSP(M.TSP):
    def __init__(self, dist):
        super().__init__(dist)
        self.torch_objective = lambda g: -self.tour_length(g)


def test_errors():
    e3 = M.TSP.reference_e3(20)
    with pytest.raises(Exception, match="symmetric"):
        pga.GeneticAlgorithm(e3, 64, device="cpu").local_search(1, 1.0)
    with pytest.raises(Exception, match="symmetric"):
        pga.GeneticAlgorithm(e3, 64, device="cpu", local_search="two_opt").run(1)
    with pytest.raises(Exception, match="PERMUTATION"):
        pga.GeneticAlgorithm(M.OneMax(64), 64, device="cpu").local_search(1, 1.0)
    with pytest.raises(Exception, match="PERMUTATION"):
        pga.GeneticAlgorithm(M.OneMax(64), 64, device="cpu", local_search="two_opt")
    tt = TorchTSP(M.TSP.random_euclidean(12).dist)
    with pytest.raises(Exception, match="torch objective"):
        pga.GeneticAlgorithm(tt, 64, device="cpu").local_search(1, 1.0)
    with pytest.raises(Exception, match="torch objective"):
        pga.GeneticAlgorithm(tt, 64, device="cpu", local_search="two_opt")
    with pytest.raises(Exception, match="unknown local search"):
        pga.GeneticAlgorithm(M.TSP.random_euclidean(12), 64, device="cpu", local_search="three_opt")
    with pytest.raises(Exception, match="LocalIslands"):
        pga.parallel.LocalIslands(M.TSP.random_euclidean(12), 2, 64, device="cpu", local_search="two_opt")


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


def capi_pop(lib, dist, S, open_path=False):
    p = lib.pga_init_device(-1)
    assert p
    lib.pga_set_seed(p, 5)
    lib.pga_set_quiet(p, 1)
    lib.pga_set_abort_on_error(p, 0)
    n = dist.shape[0]
    pop = lib.pga_create_population_ext(p, S, n, 2)  # PGA_PERMUTATION
    flat = dist.reshape(-1).tolist()
    arr = (C.c_float * len(flat))(*flat)
    assert lib.pga_set_objective_builtin(p, pop, 33 if open_path else 32, arr, len(flat), None, 0, 0, 0.0, 0.0) == 0
    # tournament-4, OX, inversion at 0.4, one elite: LOOP_KW
    assert lib.pga_set_operators(p, pop, 0, 4, 6, 1.0, 5, 0.4, 0.1, 1) == 0
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
    prob = M.TSP.random_euclidean(40, seed=2)
    p, pop = capi_pop(lib, prob.dist, 256)
    ga = pga.GeneticAlgorithm(prob, 256, device="cpu", local_search="two_opt", ls_moves=2, ls_prob=0.5, **LOOP_KW)
    assert lib.pga_set_local_search(p, pop, 1, 2, 0.5) == 0
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
    lib.pga_deinit(p)


def test_capi_asymmetric_matrix_fails(lib):
    prob = M.TSP.reference_e3(20)
    p, pop = capi_pop(lib, prob.dist, 64, open_path=True)
    assert lib.pga_local_search(p, pop) != 0
    assert b"symmetric" in lib.pga_last_error()
    assert lib.pga_set_local_search(p, pop, 7, 1, 1.0) != 0
    assert b"unknown local search" in lib.pga_last_error()
    lib.pga_deinit(p)


# --------------------------------------------------------------------- GPU ---
def problem(kind, n, seed=2):
    return {"matrix": lambda: M.TSP.random_euclidean(n, seed=seed), "euc": lambda: M.TSPEuclidean.random(n, seed=seed),
            "open": lambda: M.TSP.random_euclidean(n, seed=seed, open_path=True)}[kind]()


def assert_same(g, c):
    torch.cuda.synchronize()
    assert torch.equal(g.rows.cpu(), c.rows)
    assert torch.equal(g.scores.cpu(), c.scores)
    assert g.best_score() == c.best_score() and g.best_index() == c.best_index()


GPU_CASES = [(n, S, moves, 1.0) for n, S in [(5, 64), (9, 333), (64, 1000), (100, 500), (257, 300), (1000, 64)]
             for moves in (1, 5)] + [(64, 1000, 5, 0.3)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,S,moves,prob", GPU_CASES)
@pytest.mark.parametrize("kind", ["matrix", "euc", "open"])
def test_gpu_bitexact(kind, n, S, moves, prob):
    p = problem(kind, n)
    g = pga.GeneticAlgorithm(p, S, seed=5, device="cuda:0")
    c = pga.GeneticAlgorithm(p, S, seed=5, device="cpu")
    r0 = c.rows.clone()
    g.local_search(moves, prob)
    c.local_search(moves, prob)
    assert_same(g, c)
    assert n < 4 or (c.rows != r0).any()
    assert is_perm(g.genomes().cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("inst", ["int_euc256", "f32_sym256", "int_euc100_open"])
def test_gpu_distance_sources(inst, monkeypatch):
    """The u16 triangle, the f32 triangle (both in LDS, 16-wave blocks) and
    the f32 matrix through L2 give the CPU backend's rows and scores."""
    p = {"int_euc256": lambda: M.TSP.random_integer_euclidean(256, seed=2),
         "f32_sym256": lambda: M.TSP.random_euclidean(256, seed=2),
         "int_euc100_open": lambda: M.TSP.random_integer_euclidean(100, seed=5, open_path=True)}[inst]()
    g = pga.GeneticAlgorithm(p, 2000, seed=8, device="cuda:0")
    c = pga.GeneticAlgorithm(p, 2000, seed=8, device="cpu")
    monkeypatch.setenv("PGA_TSP_NO_LDS", "1")
    f = pga.GeneticAlgorithm(p, 2000, seed=8, device="cuda:0")
    monkeypatch.delenv("PGA_TSP_NO_LDS")
    for ga in (g, c, f):
        ga.local_search(3, 1.0)
    assert_same(g, c)
    assert_same(f, c)


@pytest.mark.gpu
def test_gpu_longest_genome():
    """kPermMaxL cities, the stage's limit on the GPU.  The GPU population is
    a copy of the CPU one: the 4-per-block init / eval kernel does not launch
    for 4096 cities given as coordinates (its four arrays and the coordinates
    need 164 416 B of LDS), and the stage rewrites every score here anyway
    (every random tour of this size has an improving move)."""
    p = M.TSPEuclidean.random(4096, seed=3)
    c = pga.GeneticAlgorithm(p, 8, seed=2, device="cpu")
    g = pga.GeneticAlgorithm(p, 8, seed=2, device="cuda:0", initialize=False)
    g.rows.copy_(c.rows)
    g.scores.copy_(c.scores)
    s0 = c.scores.clone()
    g.local_search(1, 1.0)
    c.local_search(1, 1.0)
    assert (c.scores > s0).all()
    assert_same(g, c)


def test_cpu_has_no_length_limit():
    p = M.TSPEuclidean.random(4097, seed=3)
    c = pga.GeneticAlgorithm(p, 8, seed=2, device="cpu")
    s0 = c.scores.clone()
    c.local_search(1, 1.0)
    assert (c.scores > s0).all() and is_perm(c.genomes())


@pytest.mark.gpu
def test_gpu_too_long_raises():
    p = M.TSPEuclidean.random(4097, seed=3)
    g = pga.GeneticAlgorithm(p, 8, seed=2, device="cuda:0")
    with pytest.raises(Exception, match="too long"):
        g.local_search(1, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("xo", ["ox", "pmx"])
@pytest.mark.parametrize("elitism", [1, 2])
def test_gpu_loop_bitexact(xo, elitism):
    p = M.TSP.random_euclidean(64, seed=2)
    kw = dict(seed=5, crossover=xo, mutation="inversion", mutation_rate=0.4, elitism=elitism,
              local_search="two_opt", ls_moves=2, ls_prob=0.5)
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
    p, D, t0, snaps, made, stopped = oracle_case(64, False)
    g = pga.GeneticAlgorithm(p, 64, seed=4, device="cuda:0")
    g.local_search(4 * 64, 1.0)
    torch.cuda.synchronize()
    want = snaps[4 * 64]
    assert np.array_equal(g.genomes().cpu().numpy(), want)
    assert np.array_equal(g.scores.cpu().numpy(), (-length(D, want, False)).astype(np.float32))
