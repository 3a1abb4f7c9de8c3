"""The tail steps of binary_gen_tp's unit loop (binary_dev.hpp, TAIL: the last
units of a 16-wave block's round are resolved into block-shared records by
whoever draws their ticket and bred step by step by whichever wave is free)
against the CPU backend after 3 generations: rows, scores, the best, the
{min, max, mean} statistics and the u16 keys through the key top-k.

Which wave breeds which step differs from run to run; the RNG is keyed per
child, so every output must equal the CPU backend's whatever the assignment.
The shapes are the smallest of the 16-wave launch (S0 = 16 x 64 x CUs: one
unit per wave) and just above it, where a block's round is all tail, part
tail, or owned units followed by the tail.

Statistics as in test_gpu_unit_loop.py: min and max for equality; the mean
for equality with the f32 reduction of the exact per-block totals (every
partial sum inside a block is an integer below 2^24, asserted), replayed on
the host from the scores and the launch's partition by device_sum()."""
import os

import numpy as np
import pytest
import torch

import libpga_amd as pga
from libpga_amd.parallel import LocalIslands

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = pga.models


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def s0():
    return 16 * 64 * cus()


def pair(problem, S, **kw):
    kw = dict(dict(seed=23, elitism=1), **kw)
    return (pga.GeneticAlgorithm(problem, S, device=DEV, **kw), pga.GeneticAlgorithm(problem, S, device="cpu", **kw))


def device_sum(scores, selection, grid=None, skew=None):
    """The f32 sum the device reports for integer scores from the 16-wave
    launch (one block per CU; batched islands: grid = their share of the CUs,
    no skew): exact block totals over the blocks' shares (tp.hpp tp_share,
    util.hip tp_skew_units), reduced as stats_from_parts_kernel does (256
    threads: strided adds, a 64-lane xor butterfly per wave, then the 4 wave
    values in order)."""
    S = scores.numel()
    grid = cus() if grid is None else grid
    assert (S + 63) // 64 >= 16 * grid, "not the 16-wave launch"
    per = -(-S // grid)
    per = -(-per // 64) * 64
    skew = int(os.environ.get("PGA_TP_SKEW", "2")) if skew is None else skew
    if skew * 4 >= per // 64 or grid < 2:
        skew = 0
    if selection == "rank" and -(-S // grid) == 4096 and grid == -(-S // 4096):
        skew = 0  # block b breeds sort tile b
    d = skew * 64
    sc = scores.double().numpy()
    parts = np.zeros(-(-grid // 256) * 256, dtype=np.float32)
    for b in range(grid):
        dd = d if (b | 1) < grid else 0
        lo = b * per + (dd if b & 1 else 0)
        n = per - dd if b & 1 else per + dd
        lo = min(lo, S)
        hi = min(lo + n, S)
        tot = sc[lo:hi].sum()
        assert tot < 2 ** 24, "block total not exact in f32"
        parts[b] = np.float32(tot)
    v = np.zeros(256, dtype=np.float32)
    for k in range(0, parts.size, 256):
        v = v + parts[k:k + 256]
    w = v.reshape(4, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lanes ^ o]
    r = w[0, 0]
    for i in (1, 2, 3):
        r = np.float32(r + w[i, 0])
    return float(r)


def assert_tail(island, L):
    """That the launch really asked for tail units: the outputs do not show it
    (they equal the CPU's either way).  Island.tp_tail is the launcher's
    GenArgs::tp_tail after its gates and its LDS clamp.  GS 8 (L above 512):
    PGA_TP_TAIL (default 16) units; up to 17 fit beside the records, the
    parents and the L + 1 <= 1025 histogram bins of these shapes.  GS 4: none."""
    want = int(os.environ.get("PGA_TP_TAIL", "16"))
    if L <= 512:
        assert island.tp_tail == 0
    elif want <= 16:
        assert island.tp_tail == want
    else:
        assert 17 <= island.tp_tail <= min(want, 32)


def check(g, c, selection="tournament"):
    torch.cuda.synchronize()
    assert_tail(g.island, g.problem.length)
    assert torch.equal(g.rows.cpu(), c.rows), "rows differ"
    assert torch.equal(g.scores.cpu(), c.scores), "scores differ"
    assert g.island.best() == c.island.best()
    gs, cs = g.stats(), c.stats()
    S = c.scores.numel()
    total = float(c.scores.double().sum())
    assert bool((c.scores == c.scores.round()).all())
    print(f"stats gpu {gs} cpu {cs} total {total}")
    assert gs["min"] == cs["min"] and gs["max"] == cs["max"]
    if abs(total) < 2 ** 24:
        assert gs["mean"] == cs["mean"]
    else:
        want = device_sum(c.scores, selection) / float(np.float32(S))
        print(f"mean gpu {gs['mean']!r} replayed {want!r}")
        assert gs["mean"] == want
    for largest in (True, False):  # the selection reads the u16 keys the generation wrote
        assert torch.equal(g.island.topk(777, largest, False).cpu(), c.island.topk(777, largest, False))


def run(g, c, n=3):
    g.run(n)
    c.run(n)


@pytest.mark.parametrize("extra", ["0", "+37", "+3x64", "x2+64"])
def test_tail_steps_onemax(extra):
    """S0: one unit per wave, so the whole round is tail and no owned unit
    precedes the tail loop; S0 + 37: a partial last unit inside the tail
    (padding rows; c < S in best, statistics and histogram); S0 + 3 x 64: most
    blocks all tail, one block with an extra unit, a last share smaller than
    the tail; 2 S0 + 64: owned units, then the tail, with uneven ticket counts
    (the hand-over from a wave's last owned unit to its first tail steps)."""
    S = {"0": s0(), "+37": s0() + 37, "+3x64": s0() + 3 * 64, "x2+64": 2 * s0() + 64}[extra]
    g, c = pair(M.OneMax(1024), S)
    run(g, c)
    check(g, c)


@pytest.mark.parametrize("L", [512, 1000])
def test_tail_steps_gs4_and_partial_group(L):
    """L = 512: GS = 4, whose kernels are built without the tail (it measured
    slower there, profiles/tail_steps_ab.txt): the launcher must ask for none
    and the unit loop alone must serve the shape; L = 1000: a partial group
    (have, last_mask) in the tail step."""
    g, c = pair(M.OneMax(L), s0() + 37)
    run(g, c)
    check(g, c)


@pytest.mark.parametrize("prob", ["leading", "trap"])
def test_tail_steps_key_objectives(prob):
    p = M.LeadingOnes(1024) if prob == "leading" else M.Trap(1024, 8)
    g, c = pair(p, s0() + 37)
    run(g, c)
    check(g, c)


def test_tail_steps_rank_counts():
    """Rank selection, elitism 3, a block's share one sort tile: the tile
    counts (rank_counts) the next generation's rank sort reads must include
    the children bred in the tail."""
    S = 4096 * cus()
    g, c = pair(M.OneMax(1024), S, selection="rank", rank_pressure=1.7, elitism=3)
    run(g, c)
    check(g, c, selection="rank")


def test_tail_steps_fused_key_histogram():
    """The fused key histogram takes the tail's per-step atomics: the top-k
    and bottom-k selections that read it equal the CPU's."""
    g, c = pair(M.OneMax(1024), s0() + 37)
    g.island.fused_histogram = True
    run(g, c)
    assert g.island.fused_histogram_ready
    check(g, c)
    assert g.island.fused_histogram_ready


@pytest.mark.parametrize("L", [512, 1024])
def test_tail_steps_two_rounds(L):
    """7168 children per round at 16 waves: a block's share of 7168 + 1024 + a
    few children takes two rounds.  L = 1024 (GS 8): each round has its own
    tail, so the step counter and the unit flags are re-armed at the first
    round's last barrier; L = 512 (GS 4, no tail): the counters of the unit
    loop alone."""
    S = 7168 * cus() + s0() + 37
    g, c = pair(M.OneMax(L), S)
    run(g, c, 2)
    check(g, c)


def test_tail_steps_batched_islands():
    """Two same-shape islands in one launch (binary_gen_tp_batch), each on
    half the device at the smallest population of its 16-wave launch + 37."""
    S = s0() // 2 + 37
    kw = dict(seed=29, migrate_every=100, elitism=1)
    a = LocalIslands(M.OneMax(1024), 2, S, device=DEV, **kw)
    b = LocalIslands(M.OneMax(1024), 2, S, device="cpu", **kw)
    a.run(3)
    b.run(3)
    torch.cuda.synchronize()
    assert a.batched_generations == 3
    for x, y in zip(a.islands, b.islands):
        assert torch.equal(x.rows.cpu(), y.rows) and torch.equal(x.scores.cpu(), y.scores)
        assert x.island.best() == y.island.best()
        assert_tail(x.island, 1024)
        xs, ys = x.stats(), y.stats()
        assert xs["min"] == ys["min"] and xs["max"] == ys["max"]
        want = device_sum(y.scores, "tournament", grid=cus() // 2, skew=0) / float(np.float32(S))
        print(f"mean gpu {xs['mean']!r} cpu {ys['mean']!r} replayed {want!r}")
        assert xs["mean"] == want
        for largest in (True, False):
            assert torch.equal(x.island.topk(777, largest, False).cpu(), y.island.topk(777, largest, False))
