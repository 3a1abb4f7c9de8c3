"""One PERMUTATION generation (TSP: PMX / OX1, swap / inversion) against a
plain numpy oracle.

The oracle shares no code with either backend: Philox4x32-10 (philox_np.py),
the ST_CHILD / ST_INIT word layouts, the Fisher-Yates initial tours, the
tournament, the crossover-probability test, the segment, the mutation
positions and both crossovers are written out here from their definitions --
PMX in the forward Goldberg-Lingle form (walk the mapping chain of every
displaced gene of B out of the segment), OX1 as list filtering (B read
cyclically from the segment end, minus A's segment, laid into the free slots)
-- not the way cpu_perm.cpp writes them.  The stream ids and word indices are
read out of core.hpp.  The oracle reads rows(0) and scores(0) before a step and
predicts the child rows exactly; scores are checked against a float64 tour
length of the predicted row.

Without a GPU the oracle is proved against the CPU backend; on the GPU the
kernel's rows must equal the oracle's and the CPU backend's bit for bit.
Forged parents (rotations of one tour, two tours only, identical rows, a tour
and its reverse) make every PMX mapping chain as long as the segment.  The
census asserts, from the oracle's own record of every child, that each edge
(empty and full segments, segments touching either end, equal mutation
positions, skipped crossovers, a parent mated with itself, long chains) did
occur, so that none is covered by luck.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import libpga_amd as pga
from philox_np import MASK, U64, philox

M = pga.models
F32 = np.float32
SEED = 0x5EED5 | (91 << 32)  # both Philox key words in use
S_POP = 4096
GENS = 2


def _core_constants():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "csrc", "include", "pga", "core.hpp")
    with open(path) as f:
        text = f.read()
    names = ("ST_INIT", "ST_CHILD", "W_XOPROB", "W_CUT1", "W_CUT2", "W_MUTIND", "W_MUTPOS", "W_SEL")
    return {n: int(re.search(rf"\b{n}\s*=\s*(\d+)", text).group(1)) for n in names}


K = _core_constants()


# ------------------------------------------------------------ plain oracle ---
def _blocks(stream, seed, gen, island, S, nblocks):
    """Philox blocks 0..nblocks-1 of a stream for individuals 0..S-1: a list of
    4-register lists.  counter = {block | stream << 24, ind_lo, ind_hi | island << 16, gen}."""
    ind = np.arange(S, dtype=U64)
    return [philox(np.full(S, b | (stream << 24), dtype=U64), ind & MASK, (ind >> U64(32)) | U64(island << 16),
                   np.full(S, gen, dtype=U64), seed & 0xFFFFFFFF, seed >> 32) for b in range(nblocks)]


def child_words(seed, gen, S, n, island=0):
    """Child words 0..n-1: word t = register t % 3 of ST_CHILD block t // 3."""
    blocks = _blocks(K["ST_CHILD"], seed, gen, island, S, (n + 2) // 3)
    return [blocks[t // 3][t % 3] for t in range(n)]


def idx(w, n):
    return ((w * U64(n)) >> U64(32)).astype(np.int64)


def oracle_init(seed, S, L, island=0, gen=0):
    """Fisher-Yates (Durstenfeld) from the identity: for i = L-1 .. 1 swap
    positions i and j = (w_i * (i + 1)) >> 32, w_i = register i % 4 of ST_INIT
    block i // 4."""
    blocks = _blocks(K["ST_INIT"], seed, gen, island, S, (L + 3) // 4)
    C = np.tile(np.arange(L, dtype=np.int64), (S, 1))
    r = np.arange(S)
    for i in range(L - 1, 0, -1):
        j = idx(blocks[i // 4][i % 4], i + 1)
        ci, cj = C[:, i].copy(), C[r, j].copy()
        C[r, j] = ci
        C[:, i] = cj  # (after C[r, j]: i == j leaves the gene in place)
    return C


def prob_thresh(p):
    """floor(p * 2^32) of the f32 probability, capped at 2^32 - 1."""
    v = int(np.floor(float(F32(p)) * 4294967296.0))
    return min(max(v, 0), 0xFFFFFFFF)


def oracle_tournament(scores, words, k):
    """Tournament-k winner from k words: the first contestant stays unless it
    is strictly below the challenger."""
    S = len(scores)
    b = idx(words[0], S)
    for w in words[1:k]:
        c = idx(w, S)
        b = np.where(scores[b] < scores[c], c, b)
    return b


def oracle_ox(A, B, lo, hi):
    """OX1 as list filtering: B read cyclically from hi, minus the cities of
    A[lo:hi], laid into the slots hi .. L-1, 0 .. lo-1; A[lo:hi] stays."""
    S, L = A.shape
    pos = np.arange(L)[None, :]
    r = np.arange(S)[:, None]
    seg = (pos >= lo[:, None]) & (pos < hi[:, None])
    city_in_seg = np.zeros((S, L), dtype=bool)
    city_in_seg[r, A] = seg
    Brot = B[r, (hi[:, None] + pos) % L]                       # B from hi, cyclically
    keep = ~city_in_seg[r, Brot]
    order = np.argsort(~keep, axis=1, kind="stable")           # the kept cities first, in order
    filt = Brot[r, order]
    return np.where(seg, A, filt[r, (pos - hi[:, None]) % L])  # slot t is position (hi + t) % L


def oracle_pmx(A, B, lo, hi):
    """PMX, forward Goldberg-Lingle: the child is B with A[lo:hi] copied in;
    every B[i], i in the segment, whose city is not in A's segment is placed
    where its mapping chain j = posB[A[j]] leaves the segment.  Returns the
    child and the longest chain walked (steps) per child."""
    S, L = A.shape
    pos = np.arange(L)[None, :]
    r = np.arange(S)[:, None]
    lo2, hi2 = lo[:, None], hi[:, None]
    seg = (pos >= lo2) & (pos < hi2)
    city_in_seg = np.zeros((S, L), dtype=bool)
    city_in_seg[r, A] = seg
    posB = np.zeros((S, L), dtype=np.int64)
    posB[r, B] = pos
    C = np.where(seg, A, B)
    longest = np.zeros(S, dtype=np.int64)
    rr, ii = np.nonzero(seg & ~city_in_seg[r, B])   # the displaced genes B[i]
    gene = B[rr, ii]
    jj, steps = ii.copy(), 0
    while rr.size:
        jj = posB[rr, A[rr, jj]]
        steps += 1
        out = (jj < lo[rr]) | (jj >= hi[rr])
        C[rr[out], jj[out]] = gene[out]
        np.maximum.at(longest, rr[out], steps)
        rr, jj, gene = rr[~out], jj[~out], gene[~out]
        assert steps <= L, "a mapping chain longer than the tour"
    return C, longest


def oracle_generation(rows, scores, seed, gen, *, xo, mut, p_xo, p_mut, k):
    """The children of one generation (no elites) of the [S, L] tours `rows`
    with f32 `scores`, and the record of what every child met."""
    S, L = rows.shape
    nsel = 2 * k
    w = child_words(seed, gen, S, K["W_SEL"] + nsel + 1)
    pa = oracle_tournament(scores, w[K["W_SEL"]:K["W_SEL"] + k], k)
    pb = oracle_tournament(scores, w[K["W_SEL"] + k:K["W_SEL"] + 2 * k], k)
    A, B = rows[pa], rows[pb]
    crossed = np.full(S, xo != "none")
    if xo != "none" and F32(p_xo) < F32(1.0):
        crossed = w[K["W_XOPROB"]] < U64(prob_thresh(p_xo))
    a, b = idx(w[K["W_CUT1"]], L), idx(w[K["W_CUT2"]], L + 1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    chain = np.zeros(S, dtype=np.int64)
    C = A.copy()
    if xo == "ox":
        C = np.where(crossed[:, None], oracle_ox(A, B, lo, hi), A)
    elif xo == "pmx":
        X, chain = oracle_pmx(A, B, lo, hi)
        C = np.where(crossed[:, None], X, A)
        chain = np.where(crossed, chain, 0)
    mutated = np.zeros(S, dtype=bool)
    i, j = idx(w[K["W_MUTPOS"]], L), idx(w[K["W_SEL"] + nsel], L)
    i, j = np.minimum(i, j), np.maximum(i, j)
    if mut != "none":
        mutated = w[K["W_MUTIND"]] < U64(prob_thresh(p_mut))
        pos = np.arange(L)[None, :]
        if mut == "swap":
            src = np.where(pos == i[:, None], j[:, None], np.where(pos == j[:, None], i[:, None], pos))
        else:  # inversion of [i, j], both ends included
            src = np.where((pos >= i[:, None]) & (pos <= j[:, None]), i[:, None] + j[:, None] - pos, pos)
        C = np.where(mutated[:, None], C[np.arange(S)[:, None], src], C)
    return C, dict(L=L, pa=pa, pb=pb, lo=lo, hi=hi, crossed=crossed, uses_xo=xo != "none", mutated=mutated, mi=i, mj=j,
                   chain=chain)


def tour_length64(tours, problem):
    """float64 tour length from the f32 matrix entries / f32 coordinates, and
    the score tolerance (L + 8) * 2^-24 * sum d_e: the f32 summation bound of
    L non-negative terms in any order, plus rounding room for sqrt(fma)."""
    L = tours.shape[1]
    nxt = np.roll(tours, -1, axis=1)
    if isinstance(problem, M.TSPEuclidean):
        c = problem.coords.numpy().astype(np.float64)
        d = np.sqrt(((c[tours] - c[nxt]) ** 2).sum(-1))
    else:
        d = problem.dist.numpy().astype(np.float64)[tours, nxt]
        if problem.open_path:
            d = d[:, :-1]
    total = d.sum(-1)
    return total, (L + 8) * 2.0 ** -24 * total


# ------------------------------------------------------------- the cases ---
def make_problem(kind, L):
    if kind == "matrix":
        return M.TSP.random_euclidean(L, seed=L)
    if kind == "euc":
        return M.TSPEuclidean.random(L, seed=L)
    if kind == "open":
        return M.TSP.random_euclidean(L, seed=L, open_path=True)
    if kind == "int":
        return M.TSP.random_integer_euclidean(L, seed=L)
    raise KeyError(kind)


def tours_of(ga):
    """([S, L] city ids, [S, padding] the genes beyond L) of the current rows."""
    L = ga.problem.length
    g = ga.rows.cpu().numpy().view(np.uint16)
    return g[:, :L].astype(np.int64), g[:, L:]


def scores_of(ga):
    return ga.scores.cpu().numpy().copy()


def make_ga(device, problem, *, xo, mut, p_xo, k, p_mut=0.5, S=S_POP):
    return pga.GeneticAlgorithm(problem, S, seed=SEED, device=device, crossover=xo, mutation=mut, crossover_prob=p_xo,
                                mutation_rate=p_mut, tournament_k=k, selection="tournament", elitism=0)


def forge(ga, tours):
    """Write the [S, L] tours into rows(0) (zero padding) and score them."""
    rows = ga.island.rows(0)
    g = np.zeros((rows.shape[0], 2 * rows.shape[1]), dtype=np.uint16)
    g[:, :tours.shape[1]] = tours
    rows.copy_(torch.from_numpy(g.view(np.int32)))
    ga.evaluate()


def check_scores(problem, tours, scores, what):
    total, tol = tour_length64(tours, problem)
    err = np.abs(-scores.astype(np.float64) - total)
    bad = np.flatnonzero(err > tol)
    assert bad.size == 0, f"{what}: {bad.size} scores off the float64 tour length, first {bad[:8]}, worst {err.max()}"
    d = problem.coords if isinstance(problem, M.TSPEuclidean) else problem.dist
    if not isinstance(problem, M.TSPEuclidean) and bool((d == d.round()).all()) and total.max() < 2 ** 24:
        assert np.array_equal(-scores.astype(np.float64), total), f"{what}: integer tour lengths not exact"


def run_against_oracle(ga, gens, ops, what, records=None):
    """Step `ga` generation by generation; before each step the oracle reads
    rows(0) / scores(0) and predicts the children.  Returns the oracle's rows
    after every generation."""
    out = []
    for _ in range(gens):
        tours, _ = tours_of(ga)
        gen = ga.generation
        exp, rec = oracle_generation(tours, scores_of(ga), SEED, gen, p_mut=0.5, **ops)
        ga.run(1)
        if ga.device.type != "cpu":
            torch.cuda.synchronize()
        got, pad = tours_of(ga)
        bad = np.flatnonzero((got != exp).any(-1))
        assert bad.size == 0, (f"{what}, generation {gen}: {bad.size} children differ from the oracle, first {bad[:8]}: "
                               f"lo {rec['lo'][bad[:4]]} hi {rec['hi'][bad[:4]]}")
        assert not pad.any(), f"{what}: padding genes are not zero"
        check_scores(ga.problem, exp, scores_of(ga), f"{what}, generation {gen}")
        out.append(exp)
        if records is not None:
            records.append(rec)
    return out


GRID_L = [2, 3, 5, 8, 9, 16, 17, 64, 100, 256]
GPU_L = [2, 5, 8, 17, 64, 100, 256]
XOS = ["ox", "pmx", "none"]
MUTS = ["swap", "inversion", "none"]
P_XO = [1.0, 0.7]
TOUR_K = [2, 3]


@functools.lru_cache(maxsize=None)
def cpu_case(kind, L, xo, mut, p_xo, k):
    """The CPU backend through GENS generations, checked against the oracle at
    every step: (rows after every generation, scores after the last, the
    oracle's records)."""
    problem = make_problem(kind, L)
    ga = make_ga("cpu", problem, xo=xo, mut=mut, p_xo=p_xo, k=k)
    tours, pad = tours_of(ga)
    assert np.array_equal(tours, _init(L)) and not pad.any(), "initial tours differ from the Fisher-Yates oracle"
    check_scores(problem, tours, scores_of(ga), "initial population")
    records = []
    rows = run_against_oracle(ga, GENS, dict(xo=xo, mut=mut, p_xo=p_xo, k=k), f"cpu {kind} L={L}", records)
    return rows, scores_of(ga), records


@functools.lru_cache(maxsize=None)
def _init(L):
    return oracle_init(SEED, S_POP, L)


# ------------------------------------------------------- CPU tests (no GPU) ---
def test_core_constants():
    assert K["ST_INIT"] == 1 and K["ST_CHILD"] == 3
    assert len({K[n] for n in K if n.startswith("W_")}) == 6  # six distinct word indices


def test_oracle_crossover_textbook():
    """The oracle's own operators on the textbook parents of test_perm.py."""
    A = np.array([[0, 1, 2, 3, 4, 5, 6, 7, 8]])
    B = np.array([[8, 2, 6, 7, 1, 5, 4, 0, 3]])
    lo, hi = np.array([3]), np.array([7])
    assert oracle_ox(A, B, lo, hi)[0].tolist() == [2, 7, 1, 3, 4, 5, 6, 0, 8]
    assert oracle_pmx(A, B, lo, hi)[0][0].tolist() == [8, 2, 1, 3, 4, 5, 6, 0, 7]
    for f in (oracle_ox, lambda *a: oracle_pmx(*a)[0]):
        assert np.array_equal(f(A, B, np.array([4]), np.array([4])), B)
        assert np.array_equal(f(A, B, np.array([0]), np.array([9])), A)


@pytest.mark.parametrize("k", TOUR_K)
@pytest.mark.parametrize("p_xo", P_XO)
@pytest.mark.parametrize("mut", MUTS)
@pytest.mark.parametrize("xo", XOS)
@pytest.mark.parametrize("L", GRID_L)
def test_cpu_matches_oracle(L, xo, mut, p_xo, k):
    cpu_case("matrix", L, xo, mut, p_xo, k)


def test_cpu_integer_matrix_scores_exact():
    """Integer matrices whose tours stay below 2^24: scores equal the float64 sum exactly."""
    for L in (9, 100):
        cpu_case("int", L, "pmx", "inversion", 1.0, 2)


# ------------------------------------------------------------ forged parents ---
FORGED = ["rotations", "two_tours", "identical", "reverse"]
FORGED_L = [8, 64, 100, 256]


def forged_tours(kind, L, S=S_POP):
    r = np.arange(S)[:, None]
    pos = np.arange(L)[None, :]
    if kind == "rotations":   # row r: the identity rotated by r mod L
        return (pos + r) % L
    if kind == "two_tours":   # the identity and its rotation by one, alternating
        return (pos + (r & 1)) % L
    if kind == "identical":
        return np.tile((pos * 3 + 1) % L if L % 3 else pos, (S, 1))
    if kind == "reverse":     # the identity and its reverse, alternating
        return np.where((r & 1) == 0, pos, L - 1 - pos)
    raise KeyError(kind)


def forged_ops(kind, xo):
    return dict(xo=xo, mut="none" if kind == "identical" else "inversion", p_xo=1.0, k=2)


def forged_run(device, kind, L, xo, records=None):
    problem = make_problem("matrix", L)
    ops = forged_ops(kind, xo)
    ga = make_ga(device, problem, **ops)
    parents = forged_tours(kind, L)
    forge(ga, parents)
    check_scores(problem, parents, scores_of(ga), f"forged {kind} L={L}")
    rows = run_against_oracle(ga, GENS, ops, f"{device} forged {kind} {xo} L={L}", records)
    if kind == "identical":
        assert all(np.array_equal(g, parents) for g in rows), "a child of identical parents differs from them"
    return rows, scores_of(ga)


@functools.lru_cache(maxsize=None)
def cpu_forged(kind, L, xo):
    records = []
    rows, scores = forged_run("cpu", kind, L, xo, records)
    return rows, scores, records


@pytest.mark.parametrize("xo", ["ox", "pmx"])
@pytest.mark.parametrize("L", FORGED_L)
@pytest.mark.parametrize("kind", FORGED)
def test_cpu_forged_parents(kind, L, xo):
    cpu_forged(kind, L, xo)


# -------------------------------------------------------------------- census ---
def _any(records, f):
    return any(bool(np.any(f(r))) for r in records)


def _grid_records(L):
    return [r for xo in XOS for mut in MUTS for p in P_XO for k in TOUR_K
            for r in cpu_case("matrix", L, xo, mut, p, k)[2]]


@pytest.mark.parametrize("L", GRID_L)
def test_census_of_the_grid(L):
    """Over all children of the grid cases at this L, from the oracle's records
    alone: every edge of the segment, of the mutation positions, of the
    crossover test and of the selection occurred at least once."""
    recs = _grid_records(L)
    xo = [r for r in recs if r["uses_xo"]]  # the segment matters where a crossover reads it
    assert _any(xo, lambda r: r["crossed"] & (r["lo"] == r["hi"])), "no empty segment"
    if L <= 16:
        assert _any(xo, lambda r: r["crossed"] & (r["lo"] == 0) & (r["hi"] == L)), "no full segment (0, L)"
    assert _any(xo, lambda r: r["crossed"] & (r["hi"] == L) & (r["lo"] > 0)), "no segment ending at L"
    assert _any(xo, lambda r: r["crossed"] & (r["lo"] == 0) & (r["hi"] < L)), "no segment starting at 0"
    assert _any(recs, lambda r: r["mutated"] & (r["mi"] == r["mj"])), "no mutation with i == j"
    assert _any(xo, lambda r: ~r["crossed"]), "no crossover skipped by probability"
    assert _any(xo, lambda r: r["crossed"] & (r["pa"] == r["pb"])), "no child of one parent mated with itself"


@pytest.mark.parametrize("L", FORGED_L)
def test_census_of_the_rotations(L):
    """The rotation cases did walk PMX mapping chains of at least half the tour."""
    for kind in ("rotations", "two_tours"):
        recs = cpu_forged(kind, L, "pmx")[2]
        longest = max(int(r["chain"].max()) for r in recs[:1])  # generation 0: the forged parents themselves
        assert 2 * longest >= L, f"{kind}: longest PMX chain {longest} of {L}"


# ----------------------------------------------------------------- GPU tests ---
@pytest.mark.gpu
@pytest.mark.parametrize("k", TOUR_K)
@pytest.mark.parametrize("p_xo", P_XO)
@pytest.mark.parametrize("mut", MUTS)
@pytest.mark.parametrize("xo", XOS)
@pytest.mark.parametrize("kind", ["matrix", "euc", "open"])
@pytest.mark.parametrize("L", GPU_L)
def test_gpu_matches_oracle_and_cpu(L, kind, xo, mut, p_xo, k):
    """Initial tours and GENS generations on the GPU: rows equal to the oracle's
    (which reads the GPU's own rows(0) / scores(0)) and to the CPU backend's."""
    problem = make_problem(kind, L)
    ga = make_ga("cuda:0", problem, xo=xo, mut=mut, p_xo=p_xo, k=k)
    tours, pad = tours_of(ga)
    assert np.array_equal(tours, _init(L)) and not pad.any(), "initial tours differ from the Fisher-Yates oracle"
    check_scores(problem, tours, scores_of(ga), "initial population")
    run_against_oracle(ga, GENS, dict(xo=xo, mut=mut, p_xo=p_xo, k=k), f"gpu {kind} L={L}")
    cpu_rows, cpu_scores, _ = cpu_case(kind, L, xo, mut, p_xo, k)
    assert np.array_equal(tours_of(ga)[0], cpu_rows[-1]), "rows differ from the CPU backend"
    assert np.array_equal(scores_of(ga).view(np.int32), cpu_scores.view(np.int32)), "scores differ from the CPU backend"


@pytest.mark.gpu
@pytest.mark.parametrize("xo", ["ox", "pmx"])
@pytest.mark.parametrize("L", FORGED_L)
@pytest.mark.parametrize("kind", FORGED)
def test_gpu_forged_parents(kind, L, xo):
    rows, scores = forged_run("cuda:0", kind, L, xo)
    cpu_rows, cpu_scores, _ = cpu_forged(kind, L, xo)
    assert np.array_equal(rows[-1], cpu_rows[-1]), "rows differ from the CPU backend"
    assert np.array_equal(scores.view(np.int32), cpu_scores.view(np.int32)), "scores differ from the CPU backend"
