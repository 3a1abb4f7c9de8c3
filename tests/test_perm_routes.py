"""Every boundary of the PERMUTATION launchers (the end of perm.hip), each
pinned by Island.route() first -- the kernel, group size, FULL variant, LDS
table kind, block and unit the generation really took -- and then bit for bit
against the CPU backend after two generations.  The three launcher switches
that are cached per process (PGA_FORCE_GENERIC, PGA_PERM_NO_FULL,
PGA_PERM_PMX_TBL) run in fresh processes (perm_switch_worker.py)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import libpga_amd as pga
from libpga_amd.parallel import LocalIslands

import perm_switch_worker as worker

M = pga.models
GENS = 2
HERE = os.path.dirname(os.path.abspath(__file__))


def group_size(L):
    """Lanes per individual: the smallest power of two >= the 8-gene chunks, at most 64."""
    chunks, g = (L + 7) // 8, 1
    while g < chunks and g < 64:
        g <<= 1
    return g


def run_pair(problem, S, gens=GENS, **ops):
    """The same island on the GPU and on the CPU backend through `gens`
    generations: (the GPU island's route, the two GeneticAlgorithms)."""
    g = pga.GeneticAlgorithm(problem, S, device="cuda:0", **ops)
    assert g.island.route() is None  # no generation yet
    c = pga.GeneticAlgorithm(problem, S, device="cpu", **ops)
    g.run(gens)
    c.run(gens)
    torch.cuda.synchronize()
    assert c.island.route() is None  # the CPU backend launches nothing
    return g.island.route(), g, c


def assert_equal_to_cpu(g, c):
    assert torch.equal(g.rows.cpu(), c.rows), "rows differ from the CPU backend"
    assert torch.equal(g.scores.cpu().view(torch.int32), c.scores.view(torch.int32)), "scores differ from the CPU backend"


def test_route_is_none_without_a_gpu_generation():
    ga = pga.GeneticAlgorithm(M.TSP.random_euclidean(9, seed=1), 64, seed=1, device="cpu")
    assert ga.island.route() is None
    ga.run(1)
    assert ga.island.route() is None
    other = pga.GeneticAlgorithm(M.OneMax(64), 64, seed=1, device="cpu")
    other.run(1)
    assert other.island.route() is None


@pytest.mark.gpu
def test_route_is_none_for_other_encodings():
    ga = pga.GeneticAlgorithm(M.OneMax(64), 256, seed=1, device="cuda:0")
    ga.run(1)
    assert ga.island.route() is None


# ---------------------------------------------------------- GS and FULL -----
@pytest.mark.gpu
@pytest.mark.parametrize("xo", ["ox", "pmx"])
@pytest.mark.parametrize("L", [2, 8, 9, 24, 32, 33, 64, 65, 128, 129, 256, 257, 511, 512])
def test_group_sizes_and_full(L, xo):
    r, g, c = run_pair(M.TSPEuclidean.random(L, seed=L), 1000, seed=5, crossover=xo, mutation="inversion",
                       mutation_rate=0.4, elitism=1)
    assert r["kernel"] == "fast" and r["GS"] == group_size(L) and r["block"] == 256 and r["tbl"] == 0
    assert r["full"] == (L in (64, 128, 256, 512))
    assert r["unit"] == 64 // r["GS"]  # 1000 children: the smallest unit
    assert_equal_to_cpu(g, c)


@pytest.mark.gpu
@pytest.mark.parametrize("xo", ["ox", "pmx"])
@pytest.mark.parametrize("L,S,prob,kernel,block", [(513, 1000, "euc", "generic", 256), (4064, 64, "euc", "generic", 256),
                                                   (4088, 64, "euc", "long", 64), (4096, 64, "euc", "long", 64),
                                                   (4096, 64, "matrix", "generic", 256), (4104, 64, "euc", "long", 64)])
def test_generic_and_long(L, S, prob, kernel, block, xo):
    """65 chunks and more leave the fast kernel; beyond 4096 genes one 64-lane
    block per individual.  With Euclidean coordinates in LDS as well the four
    individuals of a 256-thread block need 576 + 320 bytes per 8-gene chunk:
    508 chunks (4064 cities) fit the 160 KiB, 511 (4088) cannot, and there
    the launcher takes the long kernel (the launch used to fail)."""
    p = M.TSPEuclidean.random(L, seed=L) if prob == "euc" else M.TSP.random_euclidean(L, seed=L)
    r, g, c = run_pair(p, S, seed=5, crossover=xo, mutation="inversion", mutation_rate=0.4, elitism=1)
    assert r["kernel"] == kernel and r["GS"] == 64 and r["block"] == block and not r["full"] and r["tbl"] == 0
    assert_equal_to_cpu(g, c)


# ---------------------------------------------------------------- tables -----
def table_problem(tbl, L):
    gen = torch.Generator().manual_seed(L + tbl)
    if tbl == 1:    # integer, symmetric: the u16 triangle
        return M.TSP.random_integer_euclidean(L, seed=L)
    if tbl == 2:    # integer, asymmetric: the full u16 matrix
        return M.TSP(torch.randint(1, 1000, (L, L), generator=gen).float())
    if tbl == 3:    # f32, symmetric: the f32 triangle
        return M.TSP.random_euclidean(L, seed=L)
    d = torch.rand(L, L, generator=gen) * 10  # f32, asymmetric: no table
    d.fill_diagonal_(0)
    return M.TSP(d)


@pytest.mark.gpu
@pytest.mark.parametrize("xo", ["ox", "pmx"])
@pytest.mark.parametrize("L", [100, 256])
@pytest.mark.parametrize("tbl", [1, 2, 3, 0])
def test_tables(tbl, L, xo):
    p = table_problem(tbl, L)
    sym, ints = torch.equal(p.dist, p.dist.T), torch.equal(p.dist, p.dist.round())
    assert (sym, ints) == {1: (True, True), 2: (False, True), 3: (True, False), 0: (False, False)}[tbl]
    r, g, c = run_pair(p, 1000, seed=8, crossover=xo, mutation="swap", mutation_rate=0.4, elitism=1)
    assert r["kernel"] == "fast" and r["tbl"] == tbl and r["block"] == 256 and r["full"] == (L == 256)
    assert_equal_to_cpu(g, c)


# ------------------------------------------------- the benchmark's route -----
@pytest.mark.gpu
@pytest.mark.parametrize("xo", ["ox", "pmx"])
def test_benchmark_route(xo):
    """TSP-256 on a symmetric f32 matrix at the smallest population the
    launcher calls big (1024 children per CU): 16-wave blocks, 64-child units,
    FULL, the f32 triangle in LDS -- the route bench.py measures, bit for bit."""
    S = 1024 * torch.cuda.get_device_properties(0).multi_processor_count
    r, g, c = run_pair(M.TSP.random_euclidean(256, seed=2), S, seed=1, crossover=xo, mutation="inversion",
                       mutation_rate=0.3, elitism=1)
    print("benchmark route:", r)
    assert r["kernel"] == "fast" and r["GS"] == 32
    assert r["block"] == 1024 and r["unit"] == 64 and r["full"] and r["tbl"] != 0
    assert_equal_to_cpu(g, c)


# ------------------------------------------------------------- unit sizes -----
UNIT_S = [4096, 3 << 15, 3 << 16, 3 << 17]


@pytest.mark.gpu
def test_unit_sizes():
    """TSP-64 from coordinates (GS 8, 256-thread blocks): the children per
    wave batch halve from 64 down to 64 / GS while the batches would leave
    waves idle.  Every power of two in between is taken by one of these S."""
    seen = {}
    for S in UNIT_S:
        r, g, c = run_pair(M.TSPEuclidean.random(64, seed=4), S, seed=3, crossover="pmx", mutation="swap",
                           mutation_rate=0.4, elitism=1)
        assert r["kernel"] == "fast" and r["GS"] == 8 and r["full"] and r["block"] == 256
        assert_equal_to_cpu(g, c)
        seen[S] = r["unit"]
    print("units:", seen)
    assert set(seen.values()) == {8, 16, 32, 64}, seen


# ------------------------------------------- branches without a crossover -----
@pytest.mark.gpu
@pytest.mark.parametrize("ops", [dict(crossover="ox", crossover_prob=0.5), dict(crossover="pmx", crossover_prob=0.5),
                                 dict(crossover="none"), dict(crossover="ox", mutation="none"),
                                 dict(crossover="none", mutation="none")],
                         ids=["ox_p0.5", "pmx_p0.5", "xo_none", "mut_none", "copy"])
@pytest.mark.parametrize("L", [64, 100])
def test_no_crossover_branches(L, ops):
    kw = dict(seed=6, mutation="inversion", mutation_rate=0.4, elitism=1)
    kw.update(ops)
    r, g, c = run_pair(M.TSP.random_euclidean(L, seed=3), 1000, **kw)
    assert r["kernel"] == "fast" and r["full"] == (L == 64) and r["tbl"] == 3
    assert_equal_to_cpu(g, c)


# -------------------------------------------------------- batched islands -----
@pytest.mark.gpu
@pytest.mark.parametrize("xo", ["ox", "pmx"])
@pytest.mark.parametrize("L", [8, 256, 257])
def test_batched_islands(L, xo):
    """LocalIslands TSP in one launch per generation against the same islands on their streams."""
    common = dict(seed=7, device="cuda:0", migrate_every=0, elitism=1, crossover=xo)
    a = LocalIslands(M.TSP.random_euclidean(L, seed=3), 4, 1024, **common)
    b = LocalIslands(M.TSP.random_euclidean(L, seed=3), 4, 1024, batched=False, **common)
    a.run(GENS)
    b.run(GENS)
    torch.cuda.synchronize()
    assert a.batched_generations == GENS and b.batched_generations == 0
    for x, y in zip(a.islands, b.islands):
        rx, ry = x.island.route(), y.island.route()
        assert rx["kernel"] == "batch" and rx["GS"] == group_size(L) and rx["block"] == 256 and not rx["full"]
        assert ry["kernel"] == "fast" and ry["full"] == (L == 256)
        assert rx["tbl"] == ry["tbl"] == 3
        assert torch.equal(x.rows, y.rows) and torch.equal(x.scores, y.scores)


# ------------------------------------- the cached switches, fresh processes -----
SWITCH_CASES = [dict(L=L, xo=xo, S=1000) for L in (9, 64, 100, 256) for xo in ("ox", "pmx")]


@functools.lru_cache(maxsize=None)
def _switch_cpu():
    return worker.run_cases(SWITCH_CASES, "cpu")


def _run_worker(tmp_path, name, value):
    cases, out = tmp_path / "cases.json", tmp_path / f"{name}.npz"
    cases.write_text(json.dumps(SWITCH_CASES))
    env = dict(os.environ)
    for k in ("PGA_FORCE_GENERIC", "PGA_PERM_NO_FULL", "PGA_PERM_PMX_TBL"):
        env.pop(k, None)
    env[name] = value
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "perm_switch_worker.py"), str(cases), str(out)], env=env,
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"{name}={value}: the worker timed out; stderr:\n{e.stderr}")
    assert p.returncode == 0, f"{name}={value}: the worker exited with {p.returncode}; stderr:\n{p.stderr}"
    return np.load(out, allow_pickle=False)


def _assert_worker_equals_cpu(got):
    cpu = _switch_cpu()
    for i in range(len(SWITCH_CASES)):
        assert np.array_equal(got[f"rows{i}"], cpu[f"rows{i}"]), f"case {SWITCH_CASES[i]}: rows differ from the CPU backend"
        assert np.array_equal(got[f"scores{i}"].view(np.int32), cpu[f"scores{i}"].view(np.int32)), \
            f"case {SWITCH_CASES[i]}: scores differ from the CPU backend"
    return [json.loads(str(got[f"route{i}"])) for i in range(len(SWITCH_CASES))]


@pytest.mark.gpu
def test_switch_force_generic(tmp_path):
    routes = _assert_worker_equals_cpu(_run_worker(tmp_path, "PGA_FORCE_GENERIC", "1"))
    for case, r in zip(SWITCH_CASES, routes):
        assert r["kernel"] == "generic" and r["GS"] == group_size(case["L"]), (case, r)


@pytest.mark.gpu
def test_switch_no_full(tmp_path):
    routes = _assert_worker_equals_cpu(_run_worker(tmp_path, "PGA_PERM_NO_FULL", "1"))
    for case, r in zip(SWITCH_CASES, routes):
        assert r["kernel"] == "fast" and not r["full"] and r["tbl"] == 3, (case, r)


@pytest.mark.gpu
def test_switch_pmx_table_off(tmp_path):
    routes = _assert_worker_equals_cpu(_run_worker(tmp_path, "PGA_PERM_PMX_TBL", "0"))
    for case, r in zip(SWITCH_CASES, routes):
        assert r["kernel"] == "fast" and r["full"] == (case["L"] in (64, 256)), (case, r)
        assert r["tbl"] == (0 if case["xo"] == "pmx" else 3) and (case["xo"] != "pmx" or r["block"] == 256), (case, r)
