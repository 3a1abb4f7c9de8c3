"""Or-opt local search stage of the PERMUTATION encoding (Island::local_search
with LS_OR_OPT, csrc/kernels/perm_ls.hip perm_oropt_kernel, csrc/cpu/cpu_perm.cpp).

The contract (csrc/include/pga/perm_ops.hpp or_opt_*): a candidate (p, s, q, r)
takes the segment t[p .. p+s), s in {1, 2, 3}, p + s <= L, s <= L - 2, out of the
tour and puts it back behind t[q], reversed when r = 1 (s >= 2); q is neither in
the segment nor the edge in front of it.  With el[k] = d(t[k], t[(k+1) % L]):
  removed = (el[p-1] + el[p+s-1]) + el[q]
  r = 0: gain = removed - ((d(a,b) + d(c,x)) + d(y,e))
  r = 1: gain = (removed + If) - (((d(a,b) + d(c,y)) + d(x,e)) + Ir)
in f32; an open path is a closed tour whose closing edge has length 0, and so
has every new edge that lands on the closing position.  The largest gain wins,
ties to the smallest (p, q, s, r); a gain > 0 is applied.  CPU tests pin the
CPU backend against a plain numpy oracle on integer matrices (every f32 sum
exact), symmetric and not; GPU tests pin the kernel against the CPU backend bit
for bit."""
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

SR = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1)]  # (s, r) in tie-break order


def is_perm(t):
    return bool((torch.sort(t, dim=1).values == torch.arange(t.shape[1])).all())


def ls(ga, moves, prob=1.0):
    ga.local_search(moves, prob, kind="or_opt")


# ------------------------------------------------------------------ oracle ---
def gains(D, t, open_path):
    """[L, L, 5] f32 gains of one tour's candidates, axes (p, q, SR); -inf where
    (p, s, q, r) is no candidate."""
    L = len(t)
    ar = np.arange(L)
    P = D[np.ix_(t, t)]  # P[i, j] = d(t[i], t[j])
    nxt = (ar + 1) % L
    el = P[ar, nxt].copy()
    if open_path:
        el[L - 1] = 0
    pm = (ar - 1) % L
    p, q = ar[:, None], ar[None, :]
    G = np.full((L, L, len(SR)), -np.inf, dtype=np.float32)
    for col, (s, r) in enumerate(SR):
        if s > L - 2:
            continue
        yi, bi = (ar + s - 1) % L, (ar + s) % L  # (rows with p + s > L are masked below)
        removed = (el[pm] + el[yi])[:, None] + el[None, :]
        dab = P[pm, bi].copy()
        if open_path:
            dab[(ar == 0) | (ar + s == L)] = 0
        first, last = (yi, ar) if r else (ar, yi)  # the segment's first and last city once inserted
        dcf = P[:, first].T  # [p, q] = d(t[q], t[first[p]])
        dle = P[last][:, nxt].copy()  # [p, q] = d(t[last[p]], t[(q+1) % L])
        if open_path:
            dle[:, L - 1] = 0
        added = (dab[:, None] + dcf) + dle
        if r == 0:
            g = removed - added
        else:
            fwd, rev = el[ar].copy(), P[nxt, ar].copy()
            if s == 3:
                fwd = fwd + el[nxt]
                rev = rev + P[(ar + 2) % L, nxt]
            g = (removed + fwd[:, None]) - (added + rev[:, None])
        assert g.dtype == np.float32
        ok = (p + s <= L) & (q != pm[:, None]) & ((q < p) | (q >= p + s))
        G[:, :, col] = np.where(ok, g, -np.inf)
    return G


def apply_move(t, p, s, q, r):
    seg = t[p:p + s][::-1] if r else t[p:p + s]
    rest = np.concatenate([t[:p], t[p + s:]])
    at = (q if q < p else q - s) + 1  # behind the city that was t[q]
    return np.concatenate([rest[:at], seg, rest[at:]])


def length(D, t, open_path):
    t = np.atleast_2d(t)
    nx = np.roll(t, -1, axis=1)
    el = D[t, nx]
    if open_path:
        el = el[:, :-1]
    return el.astype(np.float64).sum(axis=1)


def oracle(D, tours, open_path, cap, snaps=()):
    """Best-improvement Or-opt, up to `cap` moves per tour, one tour at a time.
    Returns the final tours, the moves each made, whether each stopped by
    itself, the tours after min(m, its own) moves for every m in snaps, and the
    record (p, s, q, r) of every applied move.  Every applied gain is checked
    against the float64 change of the tour's length."""
    S, L = tours.shape
    final, made, stopped = tours.copy(), np.zeros(S, dtype=np.int64), np.zeros(S, dtype=bool)
    out = {m: tours.copy() for m in snaps}
    record = []
    for i in range(S):
        t = tours[i].copy()
        for m in range(cap + 1):
            if m in snaps:
                out[m][i] = t
            if m == cap:
                break
            G = gains(D, t, open_path)
            k = int(G.argmax())  # the first maximum: smallest p, then q, then (s, r)
            if not G.flat[k] > 0:
                stopped[i] = True
                break
            p, q, col = np.unravel_index(k, G.shape)
            s, r = SR[col]
            new = apply_move(t, p, s, q, r)
            assert float(G.flat[k]) == length(D, t, open_path)[0] - length(D, new, open_path)[0]
            assert sorted(new) == list(range(L))
            record.append((int(p), s, int(q), r))
            t = new
            made[i] += 1
        final[i] = t
        for m in snaps:
            if m > made[i]:
                out[m][i] = t
    return final, made, stopped, out, record


def asym_int(n, seed=3):
    """Asymmetric closed instance: integer entries in [1, 1000), zero diagonal."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randint(1, 1000, (n, n), generator=g).float()
    d.fill_diagonal_(0.0)
    return M.TSP(d)


def instance(fam, n):
    return {"sym": lambda: M.TSP.random_integer_euclidean(n, seed=2), "e3": lambda: M.TSP.reference_e3(n, seed=1),
            "asym": lambda: asym_int(n)}[fam]()


ORACLE_N = [4, 5, 9, 64, 65, 100]
ORACLE_FAMILIES = ["sym", "e3", "asym"]


@functools.lru_cache(maxsize=None)
def oracle_case(fam, n):
    p = instance(fam, n)
    D = p.dist.numpy()
    assert np.array_equal(D, np.round(D)) and np.array_equal(D, D.T) == (fam == "sym")
    ga = pga.GeneticAlgorithm(p, 64, seed=4, device="cpu")
    t0 = ga.genomes().numpy().astype(np.int64)
    final, made, stopped, snaps, record = oracle(D, t0, p.open_path, 4 * n, snaps=(1, 3))
    snaps[4 * n] = final
    return p, D, t0, snaps, made, stopped, record


@pytest.mark.parametrize("n", ORACLE_N)
@pytest.mark.parametrize("fam", ORACLE_FAMILIES)
@pytest.mark.parametrize("moves", [1, 3, "4n"])
def test_oracle_equality(fam, n, moves):
    p, D, t0, snaps, made, stopped, _ = oracle_case(fam, n)
    op = p.open_path
    m = 4 * n if moves == "4n" else moves
    ga = pga.GeneticAlgorithm(p, 64, seed=4, device="cpu")
    assert np.array_equal(ga.genomes().numpy(), t0)
    ls(ga, m)
    want = snaps[m]
    assert np.array_equal(ga.genomes().numpy(), want)
    assert np.array_equal(ga.scores.numpy(), (-length(D, want, op)).astype(np.float32))
    assert ga.generation == 0
    assert ga.best_score() == float(ga.scores.max())
    if moves == "4n":
        # the oracle stopped by itself, well inside the cap
        assert stopped.all() and made.max() < m
        assert max(gains(D, t, op).max() for t in want) <= 0  # Or-optimal
        assert (length(D, want, op) <= length(D, t0, op)).all()


def set_rows(ga, tours):
    ga.rows.copy_(ga.problem.encode(torch.as_tensor(tours), int(ga.island.row_words)))
    ga.evaluate()


# Forged tours for the classes random tours rarely reach: on an open path, a
# segment at the array's end that goes far down (p + s = L, a right shift of
# more than 64 positions); the identity tours of E3 with one stretch displaced
# have exactly one improving move each.
def forged_e3_100():
    idt = list(range(100))
    back = idt[3:] + idt[:3]          # 0 1 2 at the end: p + s = L, q < p, 96 positions move up
    front = idt[90:92] + idt[:90] + idt[92:]  # 90 91 in front: p = 0, q > p, 88 positions move down
    tail = idt[:50] + idt[51:] + [50]         # 50 at the end: p + s = L, s = 1
    return np.array([back, front, tail], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def forged_case():
    p = M.TSP.reference_e3(100, seed=1)
    D = p.dist.numpy()
    t0 = forged_e3_100()
    final, made, stopped, snaps, record = oracle(D, t0, True, 400, snaps=(1,))
    return p, D, t0, final, snaps, record


def test_forged_tours_match_the_oracle():
    p, D, t0, final, snaps, _ = forged_case()
    for m, want in ((1, snaps[1]), (400, final)):
        ga = pga.GeneticAlgorithm(p, 3, seed=4, device="cpu")
        set_rows(ga, t0)
        ls(ga, m)
        assert np.array_equal(ga.genomes().numpy(), want)
        assert np.array_equal(ga.scores.numpy(), (-length(D, want, True)).astype(np.float32))


def test_census():
    """Every class of move occurred in the cases above (the oracle's record)."""
    seen = set()
    for fam in ORACLE_FAMILIES:
        for n in ORACLE_N:
            p, _, _, _, _, _, record = oracle_case(fam, n)
            cases = [(n, p.open_path, record)]
            if fam == "e3" and n == 100:
                cases.append((n, True, forged_case()[5]))
            for L, op, rec in cases:
                for (pp, s, q, r) in rec:
                    seen |= {f"s{s}", f"r{r}", "q<p" if q < pp else "q>p"}
                    if q > pp and q + 1 - (pp + s) > 64:
                        seen.add("down>64")
                    if q < pp and pp - 1 - q > 64:
                        seen.add("up>64")
                    if pp == 0:
                        seen.add("p=0")
                    if pp + s == L:
                        seen.add("p+s=L")
                    if q == L - 1:
                        seen.add("q=L-1")
                    if op:
                        if pp == 0:
                            seen.add("open:p=0")
                        if pp + s == L:
                            seen.add("open:p+s=L")
                        if q == L - 1:
                            seen.add("open:q=L-1")
    want = {"s1", "s2", "s3", "r0", "r1", "q<p", "q>p", "down>64", "up>64", "p=0", "p+s=L", "q=L-1",
            "open:p=0", "open:p+s=L", "open:q=L-1"}
    assert want - seen == set()


# ----------------------------------------------------------- known answers ---
def circle_ga(tour, n=12):
    p = M.TSPEuclidean.circle(n)
    ga = pga.GeneticAlgorithm(p, 2, seed=1, device="cpu")
    set_rows(ga, [list(range(n))] * 2)
    best = ga.scores.clone()
    set_rows(ga, [tour] * 2)
    assert (ga.scores < best).all()
    return ga, best


def test_known_answer_displaced_city():
    """City 5 of the 12-gon sits between 9 and 10: the one move (p, s, q, r) =
    (9, 1, 4, 0) puts it back behind city 4, and the hull is Or-optimal."""
    ga, best = circle_ga([0, 1, 2, 3, 4, 6, 7, 8, 9, 5, 10, 11])
    ls(ga, 1)
    assert ga.genomes().tolist() == [list(range(12))] * 2
    assert torch.equal(ga.scores, best)
    ls(ga, 5)
    assert ga.genomes().tolist() == [list(range(12))] * 2


def test_known_answer_reversed_pair():
    """Cities 5, 6 sit as 6, 5 between 10 and 11: (9, 2, 4, 1) turns the pair
    round and puts it behind city 4; no orientation-keeping move gets there."""
    tour = [0, 1, 2, 3, 4, 7, 8, 9, 10, 6, 5, 11]
    ga, best = circle_ga(tour)
    G = gains(torch.cdist(ga.problem.coords.double(), ga.problem.coords.double()).float().numpy(), np.array(tour), False)
    assert np.unravel_index(int(G.argmax()), G.shape) == (9, 4, SR.index((2, 1)))
    ls(ga, 1)
    assert ga.genomes().tolist() == [list(range(12))] * 2
    assert torch.equal(ga.scores, best)


def test_known_answer_tie_takes_first_candidate():
    """Every distance 10 but d(1, 4) = d(4, 1) = 5: on the identity tour every
    move that makes 1 and 4 neighbours gains 5 and nothing gains more.  In
    (p, q, s, r) order these are (0, 3, 2, 0) -- the pair 0 1 between 3 and 4:
    removed = d(7,0) + d(1,2) + d(3,4) = 30, added = d(7,2) + d(3,0) + d(1,4)
    = 25 --, then (0, 4, 2, 1) -- the pair as 1 0 behind 4 --, then city 1 alone
    to either side of 4, (1, 3, 1, 0) and (1, 4, 1, 0), and more.  The first
    is taken."""
    d = 10.0 * (1 - torch.eye(8))
    d[1, 4] = d[4, 1] = 5.0
    p = M.TSP(d)
    tour = list(range(8))
    G = gains(p.dist.numpy(), np.array(tour), False)
    two = [SR.index((2, 0)), SR.index((2, 1))]
    assert G[0, 3, two[0]] == G[0, 4, two[1]] == G[1, 3, 0] == G[1, 4, 0] == G.max() == 5
    assert np.unravel_index(int(G.argmax()), G.shape) == (0, 3, two[0])
    ga = pga.GeneticAlgorithm(p, 2, seed=1, device="cpu")
    set_rows(ga, [tour] * 2)
    ls(ga, 1)
    assert ga.genomes().tolist() == [[2, 3, 0, 1, 4, 5, 6, 7]] * 2
    assert ga.scores.tolist() == [-75.0] * 2


# --------------------------------------------------------------- asymmetry ---
def test_asymmetric_matrix_works_where_two_opt_refuses():
    e3 = M.TSP.reference_e3(20)
    ga = pga.GeneticAlgorithm(e3, 64, seed=2, device="cpu")
    s0 = ga.scores.clone()
    ls(ga, 40)
    assert (ga.scores >= s0).all() and (ga.scores > s0).any() and is_perm(ga.genomes())
    with pytest.raises(Exception, match="symmetric"):
        ga.local_search(1, 1.0, kind="two_opt")
    # the configured kind is what local_search() runs
    on = pga.GeneticAlgorithm(e3, 64, seed=2, device="cpu", local_search="or_opt")
    on.local_search(40, 1.0)
    assert torch.equal(on.rows, ga.rows) and torch.equal(on.scores, ga.scores)
    with pytest.raises(Exception, match="unknown local search"):
        ga.local_search(1, 1.0, kind="three_opt")


E3_KW = dict(seed=5, crossover="ox", mutation="inversion", mutation_rate=0.4, elitism=1)


def test_memetic_e3_beats_the_plain_ga():
    """reference_e3(40), population 512, ten generations from the same seed:
    observed on the CPU backend 481 with Or-opt (ls_moves 8, everyone) against
    8790 for the plain GA; the planted path has length 390."""
    p = M.TSP.reference_e3(40)
    on = pga.GeneticAlgorithm(p, 512, device="cpu", local_search="or_opt", ls_moves=8, ls_prob=1.0, **E3_KW)
    off = pga.GeneticAlgorithm(p, 512, device="cpu", **E3_KW)
    on.run(10)
    off.run(10)
    print("memetic E3:", -on.best_score(), "plain:", -off.best_score())
    assert -on.best_score() < 0.5 * -off.best_score()
    assert -on.best_score() >= 390


# -------------------------------------------------------------- invariants ---
def asym_float(n, seed=2):
    g = torch.Generator().manual_seed(seed)
    d = torch.rand(n, n, generator=g) * 1000.0
    d.fill_diagonal_(0.0)
    return M.TSP(d)


def problem(kind, n, seed=2):
    return {"matrix": lambda: M.TSP.random_euclidean(n, seed=seed), "euc": lambda: M.TSPEuclidean.random(n, seed=seed),
            "open": lambda: M.TSP.random_euclidean(n, seed=seed, open_path=True),
            "asym": lambda: asym_float(n, seed=seed)}[kind]()


KINDS = ["matrix", "euc", "open", "asym"]


@pytest.mark.parametrize("kind", KINDS)
def test_invariants_float_instance(kind):
    ga = pga.GeneticAlgorithm(problem(kind, 50), 200, seed=3, device="cpu")
    r0, s0 = ga.rows.clone(), ga.scores.clone()
    ls(ga, 2, 0.5)
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


# ------------------------------------------------ selection, loop, errors ---
def changed_rows(ga, moves, prob):
    r0 = ga.rows.clone()
    ls(ga, moves, prob)
    return (ga.rows != r0).any(dim=1)


def test_selection():
    p = M.TSPEuclidean.random(16, seed=1)
    new = lambda: pga.GeneticAlgorithm(p, 4096, seed=9, device="cpu")  # noqa: E731
    ga = new()
    r0, s0 = ga.rows.clone(), ga.scores.clone()
    ls(ga, 1, 0.0)
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
LS_KW = dict(local_search="or_opt", ls_moves=2, ls_prob=0.5)


def test_loop_equals_manual_stages():
    p = M.TSP.reference_e3(40)
    a = pga.GeneticAlgorithm(p, 256, device="cpu", **LS_KW, **LOOP_KW)
    b = pga.GeneticAlgorithm(p, 256, device="cpu", **LOOP_KW)
    assert a.run(3) == 3
    for _ in range(3):
        b.run(1)
        ls(b, 2, 0.5)
    assert a.generation == b.generation == 3
    assert torch.equal(a.rows, b.rows) and torch.equal(a.scores, b.scores)
    # set_operators switches the option on as well, and the stage defaults to the operators' values and kind
    b.set_operators(**LS_KW)
    a.run(1)
    b.run(1)
    assert torch.equal(a.rows, b.rows) and torch.equal(a.scores, b.scores)
    a.local_search()
    ls(b, 2, 0.5)
    assert torch.equal(a.rows, b.rows) and torch.equal(a.scores, b.scores)


def test_loop_history_describes_the_population_after_the_stage():
    p = M.TSP.reference_e3(40)
    ga = pga.GeneticAlgorithm(p, 256, device="cpu", **LS_KW, **LOOP_KW)
    ga.record_history()
    bests = []
    for _ in range(3):
        ga.run(1)
        bests.append(ga.best_score())
    h = ga.history()
    assert h.shape[0] == 3 and h[:, 1].tolist() == bests


def test_loop_checkpoint_resume(tmp_path):
    p = M.TSP.reference_e3(40)
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


class TorchTSP(M.TSP):
    def __init__(self, dist):
        super().__init__(dist)
        self.torch_objective = lambda g: -self.tour_length(g)


JIT_TOUR = """
__device__ float tour(const unsigned short *row, unsigned int n, const float *d) {
  float s = 0.f;
  for (unsigned int i = 0; i < n; ++i) s += d[row[i] * n + row[(i + 1) % n]];
  return -s;
}
"""


def test_errors():
    with pytest.raises(Exception, match="PERMUTATION"):
        pga.GeneticAlgorithm(M.OneMax(64), 64, device="cpu").local_search(1, 1.0, kind="or_opt")
    with pytest.raises(Exception, match="PERMUTATION"):
        pga.GeneticAlgorithm(M.OneMax(64), 64, device="cpu", local_search="or_opt")
    tt = TorchTSP(M.TSP.reference_e3(12).dist)
    with pytest.raises(Exception, match="torch objective"):
        pga.GeneticAlgorithm(tt, 64, device="cpu").local_search(1, 1.0, kind="or_opt")
    with pytest.raises(Exception, match="torch objective"):
        pga.GeneticAlgorithm(tt, 64, device="cpu", local_search="or_opt")
    with pytest.raises(Exception, match="LocalIslands"):
        pga.parallel.LocalIslands(M.TSP.reference_e3(12), 2, 64, device="cpu", local_search="or_opt")


@pytest.mark.gpu
def test_jit_objective_is_refused():
    p = M.JitObjective("permutation", 12, JIT_TOUR, name="tour", data=M.TSP.reference_e3(12).dist.reshape(-1))
    ga = pga.GeneticAlgorithm(p, 64, device="cuda:0")
    with pytest.raises(Exception, match="not a JIT objective"):
        ga.local_search(1, 1.0, kind="or_opt")
    with pytest.raises(Exception, match="built-in TSP objective"):
        pga.GeneticAlgorithm(p, 64, device="cuda:0", local_search="or_opt")


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


def capi_state(lib, p, pop, S):
    sc = (C.c_float * S)()
    assert lib.pga_get_scores(p, pop, sc) == 0
    rb = lib.pga_row_bytes(pop)
    rows = torch.empty(S, rb // 4, dtype=torch.int32)
    for i in range(S):
        assert lib.pga_get_genome(p, pop, i, C.c_void_p(rows[i].data_ptr())) == 0
    return rows, torch.tensor(list(sc))


def test_capi_matches_python(lib):
    prob = M.TSP.reference_e3(40)
    p = lib.pga_init_device(-1)
    assert p
    lib.pga_set_seed(p, 5)
    lib.pga_set_quiet(p, 1)
    lib.pga_set_abort_on_error(p, 0)
    pop = lib.pga_create_population_ext(p, 256, 40, 2)  # PGA_PERMUTATION
    flat = prob.dist.reshape(-1).tolist()
    arr = (C.c_float * len(flat))(*flat)
    assert lib.pga_set_objective_builtin(p, pop, 33, arr, len(flat), None, 0, 0, 0.0, 0.0) == 0  # PGA_OBJ_TSP_OPEN
    # tournament-4, OX, inversion at 0.4, one elite: LOOP_KW
    assert lib.pga_set_operators(p, pop, 0, 4, 6, 1.0, 5, 0.4, 0.1, 1) == 0
    ga = pga.GeneticAlgorithm(prob, 256, device="cpu", **LS_KW, **LOOP_KW)
    assert lib.pga_set_local_search(p, pop, 3, 2, 0.5) == 0  # PGA_LS_OR_OPT
    lib.pga_run(p, 2)
    ga.run(2)
    assert lib.pga_generation(pop) == 2
    rows, sc = capi_state(lib, p, pop, 256)
    assert torch.equal(rows, ga.rows) and torch.equal(sc, ga.scores)
    assert lib.pga_local_search(p, pop) == 0  # the kind and values set above
    ga.local_search()
    rows, sc = capi_state(lib, p, pop, 256)
    assert torch.equal(rows, ga.rows) and torch.equal(sc, ga.scores)
    assert lib.pga_generation(pop) == 2
    lib.pga_deinit(p)


def test_cpu_has_no_length_limit():
    p = M.TSPEuclidean.random(4097, seed=3)
    c = pga.GeneticAlgorithm(p, 4, seed=2, device="cpu")
    s0 = c.scores.clone()
    ls(c, 1)
    assert (c.scores > s0).all() and is_perm(c.genomes())


# --------------------------------------------------------------------- GPU ---
def assert_same(g, c):
    torch.cuda.synchronize()
    assert torch.equal(g.rows.cpu(), c.rows)
    assert torch.equal(g.scores.cpu(), c.scores)
    assert g.best_score() == c.best_score() and g.best_index() == c.best_index()


GPU_CASES = [(n, S, moves, 1.0)
             for n, S in [(4, 64), (5, 64), (9, 333), (64, 1000), (65, 500), (100, 500), (257, 300), (1000, 32)]
             for moves in (1, 5)] + [(64, 1000, 5, 0.3)]


@functools.lru_cache(maxsize=None)
def cpu_result(kind, n, S, moves, prob):
    """The CPU backend's population before and after the stage (computed once, read only)."""
    c = pga.GeneticAlgorithm(problem(kind, n), S, seed=5, device="cpu")
    r0 = c.rows.clone()
    ls(c, moves, prob)
    return c, r0


@pytest.mark.gpu
@pytest.mark.parametrize("n,S,moves,prob", GPU_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_bitexact(kind, n, S, moves, prob):
    c, r0 = cpu_result(kind, n, S, moves, prob)
    g = pga.GeneticAlgorithm(c.problem, S, seed=5, device="cuda:0")
    assert torch.equal(g.rows.cpu(), r0)
    ls(g, moves, prob)
    assert_same(g, c)
    assert (c.rows != r0).any()
    assert is_perm(g.genomes().cpu())


SOURCES = {"u16_triangle_256": lambda: M.TSP.random_integer_euclidean(256, seed=2),
           "u16_full_e3_100": lambda: M.TSP.reference_e3(100),
           "u16_full_asym_128": lambda: asym_int(128),
           "f32_triangle_256": lambda: M.TSP.random_euclidean(256, seed=2),
           "f32_asym_l2_128": lambda: asym_float(128)}


@pytest.mark.gpu
@pytest.mark.parametrize("inst", list(SOURCES))
def test_gpu_distance_sources(inst, monkeypatch):
    """The u16 triangle, the full u16 matrix, the f32 triangle (all three in
    LDS, 16-wave blocks) and the f32 matrix through L2 give the CPU backend's
    rows and scores; so does each table instance with the tables switched off."""
    p = SOURCES[inst]()
    g = pga.GeneticAlgorithm(p, 1000, seed=8, device="cuda:0")
    c = pga.GeneticAlgorithm(p, 1000, seed=8, device="cpu")
    monkeypatch.setenv("PGA_TSP_NO_LDS", "1")
    f = pga.GeneticAlgorithm(p, 1000, seed=8, device="cuda:0")
    monkeypatch.delenv("PGA_TSP_NO_LDS")
    for ga in (g, c, f):
        ls(ga, 3)
    assert_same(g, c)
    assert_same(f, c)


@pytest.mark.gpu
def test_gpu_longest_genome():
    """kPermMaxL cities, the stage's limit on the GPU (the candidate number
    still fits 32 bits).  The GPU population is a copy of the CPU one, as in
    the 2-opt test: the 4-per-block init / eval kernel does not launch for 4096
    cities given as coordinates, and the stage rewrites every score here."""
    p = M.TSPEuclidean.random(4096, seed=3)
    c = pga.GeneticAlgorithm(p, 4, seed=2, device="cpu")
    g = pga.GeneticAlgorithm(p, 4, seed=2, device="cuda:0", initialize=False)
    g.rows.copy_(c.rows)
    g.scores.copy_(c.scores)
    s0 = c.scores.clone()
    ls(g, 1)
    ls(c, 1)
    assert (c.scores > s0).all()
    assert_same(g, c)


@pytest.mark.gpu
def test_gpu_too_long_raises():
    p = M.TSPEuclidean.random(4097, seed=3)
    g = pga.GeneticAlgorithm(p, 4, seed=2, device="cuda:0")
    with pytest.raises(Exception, match="too long"):
        ls(g, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("xo", ["ox", "pmx"])
@pytest.mark.parametrize("elitism", [1, 2])
def test_gpu_loop_bitexact(xo, elitism):
    p = M.TSP.reference_e3(64)
    kw = dict(seed=5, crossover=xo, mutation="inversion", mutation_rate=0.4, elitism=elitism, **LS_KW)
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
@pytest.mark.parametrize("fam", ["sym", "e3"])
def test_gpu_oracle_to_convergence(fam):
    p, D, t0, snaps, made, stopped, _ = oracle_case(fam, 64)
    g = pga.GeneticAlgorithm(p, 64, seed=4, device="cuda:0")
    ls(g, 4 * 64)
    torch.cuda.synchronize()
    want = snaps[4 * 64]
    assert np.array_equal(g.genomes().cpu().numpy(), want)
    assert np.array_equal(g.scores.cpu().numpy(), (-length(D, want, p.open_path)).astype(np.float32))


@pytest.mark.gpu
def test_gpu_forged_tours():
    """The forged E3 tours (shifts of more than 64 positions in both directions) on the GPU."""
    p, D, t0, final, snaps, _ = forged_case()
    for m, want in ((1, snaps[1]), (400, final)):
        g = pga.GeneticAlgorithm(p, 3, seed=4, device="cuda:0")
        set_rows(g, t0)
        ls(g, m)
        torch.cuda.synchronize()
        assert np.array_equal(g.genomes().cpu().numpy(), want)
        assert np.array_equal(g.scores.cpu().numpy(), (-length(D, want, True)).astype(np.float32))
