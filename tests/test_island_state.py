"""What an Island knows about a population besides its rows and scores (valid
best partials, fused statistics partials and their block partition, tournament
keys, the fused key histogram, the rank sort's tile counts) is a by-product of
the kernel that wrote the scores, and stays usable only until something else
rewrites them.  Each script below drives a GPU island and a CPU-backend island
through the same sequence of public operations, chosen to cross every edge at
which such a by-product must be dropped or may be kept, and compares rows,
scores, best() and stats() after every step.  A by-product kept one step too
long shows as a top-k, a rank sort, a roulette prefix or a tournament computed
from another population.

Exactness follows the per-encoding backend tests: integer objectives (BINARY
OneMax, integer TSP) and polynomial REAL objectives bit for bit
(test_gpu_binary.py, test_perm.py, test_real.py EXACT); Rastrigin as
test_real.py::test_gpu_matches_cpu compares transcendental objectives.  The
statistics compare min, max and count exactly and the sum as
test_gpu_unit_loop.py::check does (exactly while it is an integer below 2^24,
else to 66 * 2^-24 relative).

S = 50 000 for the BINARY scripts (the size test_fused_hist.py takes against
the CPU backend): the two-phase kernel with the histogram, asserted after the
first run.
"""
import pytest
import torch

import libpga_amd as pga
from libpga_amd._ext import C

M = pga.models
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def pair(problem, S, **kw):
    g = pga.GeneticAlgorithm(problem, S, device=DEV, **kw)
    c = pga.GeneticAlgorithm(problem, S, device="cpu", **kw)
    return g, c


def same_stats(g, c):
    gs, cs = g.island.stats(), c.island.stats()  # (min, max, sum, count)
    assert gs[0] == cs[0] and gs[1] == cs[1] and gs[3] == cs[3], f"stats differ: gpu {gs} cpu {cs}"
    sc = c.scores.cpu()
    if bool((sc == sc.round()).all()) and abs(float(sc.double().sum())) < 2 ** 24:
        assert gs[2] == cs[2], f"sums differ: gpu {gs[2]!r} cpu {cs[2]!r}"
    else:
        assert abs(gs[2] - cs[2]) <= 66 * 2.0 ** -24 * abs(cs[2]), f"sums differ: gpu {gs[2]!r} cpu {cs[2]!r}"


def same(g, c, step):
    torch.cuda.synchronize()
    assert torch.equal(g.rows.cpu(), c.rows), f"rows differ after {step}"
    assert torch.equal(g.scores.cpu(), c.scores), f"scores differ after {step}"
    assert g.island.best() == c.island.best(), f"best differs after {step}"
    same_stats(g, c)


def both(g, c, fn):
    for ga in (g, c):
        fn(ga)


def staging(ga, k):
    rw = int(ga.island.row_words)
    return (torch.empty(k * rw, dtype=torch.int32, device=ga.device),
            torch.empty(k, dtype=torch.float32, device=ga.device))


def migration_epoch(g, c, k, policy, check, hist=False):
    """IslandModel's epoch on both islands: emigrate, a generation, re-score the
    migrants, immigrate them over the island's own bottom-k."""
    bufs = {}
    for ga in (g, c):
        ga.island.migration_policy = policy
        bufs[ga] = staging(ga, k)
        ga.island.emigrate(k, *bufs[ga])
    torch.cuda.synchronize()
    assert torch.equal(bufs[g][0].cpu(), bufs[c][0]) and torch.equal(bufs[g][1].cpu(), bufs[c][1]), "emigrants differ"
    both(g, c, lambda ga: ga.run(1))
    check(g, c, f"emigrate({k}) policy {policy}, run(1)")
    for ga in (g, c):
        assert ga.island.evaluate_rows(*bufs[ga])
    torch.cuda.synchronize()
    assert torch.equal(bufs[g][1].cpu(), bufs[c][1]), "re-scored emigrants differ"
    for ga in (g, c):
        ga.island.immigrate(k, *bufs[ga])
    if hist:
        assert not g.island.fused_histogram_ready  # the victims' keys changed
    check(g, c, f"immigrate policy {policy}")


# tail units of the two-phase launch (Island.tp_tail) after every step of the
# BINARY script that runs a generation (eleven of them), recorded on the
# MI355X: only the 16-wave blocks of populations of 2^18 and more take tail
# steps (as many as the CU's LDS admits), the 4-wave blocks here take none
TP_TAIL = {
    "tournament_e3": [0] * 11,
    "rank": [0] * 11,
    "roulette": [0] * 11,
}

BINARY_KW = {
    "tournament_e3": dict(elitism=3),
    "rank": dict(selection="rank"),
    "roulette": dict(selection="roulette"),
}


def binary_script(name, tmp_path, trace):
    S, L = 50000, 1024
    g, c = pair(M.OneMax(L), S, seed=7, **BINARY_KW[name])
    both(g, c, lambda ga: setattr(ga.island, "fused_histogram", True))

    def run(n, step):
        both(g, c, lambda ga: ga.run(n))
        same(g, c, step)
        trace.append(int(g.island.tp_tail))

    same(g, c, "initialize")
    assert not g.island.fused_histogram_ready
    run(3, "run(3)")
    assert g.island.fused_histogram_ready  # the two-phase kernel took the histogram
    for rep in range(2):  # the second selection re-zeroes the status words
        for largest in (True, False):
            assert torch.equal(g.island.topk(777, largest, False).cpu(), c.island.topk(777, largest, False)), \
                f"unsorted topk {rep} differs"
    run(1, "topk, run(1)")
    for policy in (C.MIG_TOPK, C.MIG_STRIPE):
        migration_epoch(g, c, 500, policy, same, hist=True)
        trace.append(int(g.island.tp_tail))
        run(2, "immigrate, run(2)")
    # scores rewritten behind the island's back (what _custom_eval does), then rebest()
    forged = ((torch.arange(300) * 7) % (L + 1)).to(torch.float32)
    both(g, c, lambda ga: ga.scores[1000:1300].copy_(forged.to(ga.device)))
    both(g, c, lambda ga: ga.island.rebest())
    assert not g.island.fused_histogram_ready
    same(g, c, "rebest")
    run(2, "rebest, run(2)")
    both(g, c, lambda ga: ga.set_operators(mutation_rate=0.002))
    assert not g.island.fused_histogram_ready
    run(2, "set_operators, run(2)")
    for ga, f in ((g, "g.ckpt"), (c, "c.ckpt")):
        ga.save(str(tmp_path / f))
    run(1, "save, run(1)")
    for ga, f in ((g, "g.ckpt"), (c, "c.ckpt")):
        ga.load(str(tmp_path / f))
    assert not g.island.fused_histogram_ready
    same(g, c, "load")
    run(2, "load, run(2)")

    def staged(ga):
        isl = ga.island
        isl.crossover_stage()
        isl.mutate_stage()
        isl.swap()
        isl.evaluate()

    both(g, c, staged)
    assert not g.island.fused_histogram_ready
    same(g, c, "staged generation")
    run(2, "staged generation, run(2)")


@pytest.mark.parametrize("name", list(BINARY_KW))
def test_binary_by_products_follow_the_scores(name, tmp_path):
    trace = []
    binary_script(name, tmp_path, trace)
    assert trace == TP_TAIL[name]


# ---------------------------------------------------------------- REAL ---
def close(a, b, rel=2e-4, abs_=2e-3):  # test_real.py
    return torch.allclose(a, b, rtol=rel, atol=abs_)


def same_transcendental(g, c, step):
    """test_real.py::test_gpu_matches_cpu for the objectives whose device cosine
    differs from the host's by ulps: the selection is identical unless two
    contestants' scores lie within an ulp."""
    torch.cuda.synchronize()
    same_rows = (g.rows.cpu() == c.rows).all(-1).float().mean().item()
    assert same_rows > 0.995, f"rows differ after {step}: {same_rows}"
    assert close(g.scores.cpu(), c.scores) or same_rows < 1.0, f"scores differ after {step}"
    gb, cb = g.island.best(), c.island.best()
    assert (abs(gb[0] - cb[0]) <= 2e-3 + 2e-4 * abs(cb[0]) and gb[1] == cb[1]) or same_rows < 1.0, f"best differs after {step}"
    gs, cs = g.island.stats(), c.island.stats()
    assert gs[3] == cs[3]
    assert all(abs(x - y) <= 2e-3 + 2e-4 * abs(y) for x, y in zip(gs[:3], cs[:3])) or same_rows < 1.0, \
        f"stats differ after {step}: gpu {gs} cpu {cs}"


def foreign_rows(problem, S, k):
    src = pga.GeneticAlgorithm(problem, S, seed=99, device="cpu", elitism=1)
    src.run(5)
    rows, sc = staging(src, k)
    src.island.emigrate(k, rows, sc)
    return rows, sc


# qkeys(0) is not None after each step of the script below (the parent's
# pattern): a generation leaves the keys it wrote, a rewrite of the scores
# drops them, the next generation re-keys
QKEYS = [False, True, False, True, False, True]  # initialize, run(34), immigrate, run(2), rebest, run(2)


def real_qkey_script(trace):
    p, S = M.Rastrigin(30), 3000
    g, c = pair(p, S, seed=21, elitism=1)

    def step(fn, what):
        both(g, c, fn)
        same_transcendental(g, c, what)
        trace.append(g.island.qkeys(0) is not None)

    trace.append(g.island.qkeys(0) is not None)
    step(lambda ga: ga.run(34), "run(34)")  # the range refresh at generation 32 is crossed
    rows, sc = foreign_rows(p, S, 64)
    step(lambda ga: ga.island.immigrate(64, rows.to(ga.device), sc.to(ga.device)), "immigrate")
    step(lambda ga: ga.run(2), "immigrate, run(2)")
    step(lambda ga: ga.island.rebest(), "rebest")
    step(lambda ga: ga.run(2), "rebest, run(2)")


def test_real_quantized_keys_follow_the_scores(monkeypatch):
    monkeypatch.setenv("PGA_TP_MIN_S", "0")  # the two-phase kernel (and the quantized keys) at this size
    trace = []
    real_qkey_script(trace)
    assert trace == QKEYS


def test_real_tiny_multi_generation_launch(monkeypatch):
    """S = 256: run(n >= 2) is one launch that leaves the other parity without
    valid partials or keys; run(1) after it is a plain generation."""
    monkeypatch.delenv("PGA_TP_MIN_S", raising=False)
    p, S = M.Sphere(3), 256
    g, c = pair(p, S, seed=5, elitism=1)
    both(g, c, lambda ga: ga.run(5))
    same(g, c, "run(5)")
    assert g.island.qkeys(0) is None and g.island.qkeys(1) is None
    rows, sc = foreign_rows(p, S, 8)
    both(g, c, lambda ga: ga.island.immigrate(8, rows.to(ga.device), sc.to(ga.device)))
    same(g, c, "immigrate")
    both(g, c, lambda ga: ga.run(1))
    same(g, c, "immigrate, run(1)")
    both(g, c, lambda ga: ga.run(4))
    same(g, c, "run(4)")


# --------------------------------------------------------- PERMUTATION ---
def test_tsp_local_search_and_migration():
    p = M.TSP.random_integer_euclidean(64, seed=1)
    assert torch.equal(p.dist, p.dist.T) and torch.equal(p.dist, p.dist.round())
    g, c = pair(p, 4096, seed=8, elitism=1, local_search="two_opt")
    both(g, c, lambda ga: ga.run(3))
    same(g, c, "run(3)")
    both(g, c, lambda ga: ga.local_search())
    same(g, c, "local_search()")
    for policy in (C.MIG_TOPK, C.MIG_STRIPE):
        migration_epoch(g, c, 100, policy, same)
        both(g, c, lambda ga: ga.run(2))
        same(g, c, "immigrate, run(2)")


# --------------------------------------------------------------- graph ---
def test_graph_replay_across_set_operators():
    """test_graph.py's onemax_e4_roulette (elitism > 1: the fused histogram is
    on, replays produce none): replay, a configuration change, replay, against
    plain launches."""
    kw = dict(seed=3, device=DEV, elitism=4, selection="roulette")
    a = pga.GeneticAlgorithm(M.OneMax(200), 3000, **kw)
    b = pga.GeneticAlgorithm(M.OneMax(200), 3000, **kw)
    a.island.graph_generations = 0
    b.island.graph_generations = 8
    replays = 0
    for step in ("replay", "set_operators, replay"):
        a.run(21)
        b.run(21)
        torch.cuda.synchronize()
        assert torch.equal(a.rows, b.rows) and torch.equal(a.scores, b.scores), f"differ after {step}"
        assert a.island.best() == b.island.best()
        same_stats(a, b)
        assert b.island.graph_replays > replays, f"no replay in {step}"
        replays = b.island.graph_replays
        for ga in (a, b):
            ga.set_operators(mutation_rate=0.01)
    assert a.generation == b.generation == 42
