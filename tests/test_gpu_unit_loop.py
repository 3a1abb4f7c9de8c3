"""The unit-unrolled breed loop of binary_gen_tp (binary_dev.hpp: full
64-child units, the 16-wave launch) and its per-unit transposed epilogue (one
score / key store, one best, one statistics add and one histogram atomic per
child) against the CPU backend after 3 generations: rows, scores, the best,
the u16 keys (through the key top-k, the only reader besides the next
generation's tournaments) and the {min, mean} statistics.

The 16-wave launch needs ceil(S / 64) >= 16 x CUs; S0 below is the smallest
such population on the device the test runs on.

Statistics.  min and max are compared for equality with the CPU backend.  The
mean is compared for equality too, with what it must be: the device builds
the sum in f32 -- per lane, per wave and per block in the generation kernel,
then one pass over the block partials (stats_from_parts_kernel) -- while the
CPU backend sums in f64 and rounds once, so above a total of 2^24 the two
differ by design in the last bits.  For the integer objectives every partial
sum inside a block is an exact integer below 2^24 whatever the grouping (the
block totals are asserted to be), so the device's sum is exactly the f32
reduction of the exact block totals in the final pass's order, which
device_sum() replays on the host from the score array and the launch's
partition (tp.hpp tp_share, util.hip tp_skew_units).  A wrong, missing or
doubled add in the per-unit epilogue changes a block total and fails it.
The float knapsack's block partials are themselves rounded sums in lane
order, which only the device can produce: its mean is held to the rounding
bound instead, 2^-24 relative per f32 add on the longest chain of adds behind
one child (8 steps x 4 units per lane + 6 butterfly levels + 16 wave partials
+ 1 + 6 + 4 in the final pass = 65) plus the CPU's one."""
import os

import numpy as np
import pytest
import torch

import libpga_amd as pga

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = pga.models


def s0():
    return 16 * 64 * torch.cuda.get_device_properties(0).multi_processor_count


def pair(problem, S, **kw):
    kw = dict(dict(seed=17, elitism=1), **kw)
    return (pga.GeneticAlgorithm(problem, S, device=DEV, **kw), pga.GeneticAlgorithm(problem, S, device="cpu", **kw))


def device_sum(scores, selection):
    """The f32 sum the device reports for integer scores from the 16-wave
    launch (one block per CU): exact block totals over the blocks' shares,
    reduced as stats_from_parts_kernel does (256 threads: strided adds, a
    64-lane xor butterfly per wave, then the 4 wave values in order)."""
    S = scores.numel()
    grid = torch.cuda.get_device_properties(0).multi_processor_count
    assert (S + 63) // 64 >= 16 * grid, "not the 16-wave launch"
    per = -(-S // grid)
    per = -(-per // 64) * 64
    skew = int(os.environ.get("PGA_TP_SKEW", "2"))
    if skew * 4 >= per // 64 or grid < 2:
        skew = 0
    if selection == "rank" and -(-S // grid) == 4096 and grid == -(-S // 4096):
        skew = 0  # block b breeds sort tile b (binary_gs.hip go_tp)
    d = skew * 64
    sc = scores.double().numpy()
    parts = np.zeros(-(-grid // 256) * 256, dtype=np.float32)
    for b in range(grid):
        pair_ok = (b | 1) < grid
        dd = d if pair_ok else 0
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


def check(g, c, keys=True, selection="tournament"):
    torch.cuda.synchronize()
    assert torch.equal(g.rows.cpu(), c.rows), "rows differ"
    assert torch.equal(g.scores.cpu(), c.scores), "scores differ"
    assert g.island.best() == c.island.best()
    gs, cs = g.stats(), c.stats()
    S = c.scores.numel()
    total = float(c.scores.double().sum())
    integer = bool((c.scores == c.scores.round()).all())
    print(f"stats gpu {gs} cpu {cs} total {total}")
    assert gs["min"] == cs["min"] and gs["max"] == cs["max"]
    if integer and abs(total) < 2 ** 24:
        assert gs["mean"] == cs["mean"]
    elif integer:
        want = device_sum(c.scores, selection) / float(np.float32(S))
        print(f"mean gpu {gs['mean']!r} replayed {want!r}")
        assert gs["mean"] == want
    else:
        assert abs(gs["mean"] - cs["mean"]) <= 66 * 2.0 ** -24 * abs(cs["mean"])
    if keys:  # the selection reads the u16 keys the generation wrote
        for largest in (True, False):
            assert torch.equal(g.island.topk(777, largest, False).cpu(), c.island.topk(777, largest, False))


def run3(g, c):
    g.run(3)
    c.run(3)


@pytest.mark.parametrize("extra", ["0", "+37", "x2+64"])
def test_unit_loop_onemax(extra):
    """S0: one unit per wave (the first unit's RESOLVE and nothing after it);
    S0 + 37: a partial last unit (padding rows, scores and keys past S; c < S
    in best, statistics and histogram); 2 S0 + 64: several units per wave with
    uneven ticket counts (the load cursor's hand-over into the next unit, and
    a last unit without a successor)."""
    S = {"0": s0(), "+37": s0() + 37, "x2+64": 2 * s0() + 64}[extra]
    g, c = pair(M.OneMax(1024), S)
    run3(g, c)
    check(g, c)


@pytest.mark.parametrize("L", [1000, 512])
def test_unit_loop_partial_group_and_gs4(L):
    """L = 1000: FULL == false at GS = 8 (have, last_mask); L = 512: GS = 4,
    four register sets over a unit of four steps."""
    g, c = pair(M.OneMax(L), s0() + 37)
    run3(g, c)
    check(g, c)


@pytest.mark.parametrize("prob", ["leading", "trap"])
def test_unit_loop_key_objectives(prob):
    """The other exact-key objectives through the transposed epilogue."""
    p = M.LeadingOnes(1024) if prob == "leading" else M.Trap(1024, 8)
    g, c = pair(p, s0() + 37)
    run3(g, c)
    check(g, c)


def test_unit_loop_float_objective_keeps_per_step_epilogue():
    """A non-integer knapsack (f32 scores, no keys) takes the per-step score
    stores and statistics (the rotating loop), whose f32 sums depend on the
    order in which a lane adds."""
    gen = torch.Generator().manual_seed(3)
    p = M.Knapsack01(torch.rand(1024, generator=gen) * 10, torch.rand(1024, generator=gen) * 10, 2500.0)
    g, c = pair(p, s0() + 37)
    run3(g, c)
    assert g.island.knapsack_digits == 0  # the scalar evaluation, not the matrix cores
    check(g, c, keys=False)


def test_unit_loop_rank_counts():
    """Rank selection, elitism 3: the rank sort's tile counts (rank_counts)
    come from the per-unit histogram atomics when a block's share is one sort
    tile (S = 4096 x CUs)."""
    S = 4096 * torch.cuda.get_device_properties(0).multi_processor_count
    g, c = pair(M.OneMax(1024), S, selection="rank", rank_pressure=1.7, elitism=3)
    run3(g, c)
    check(g, c, selection="rank")


def test_unit_loop_fused_key_histogram():
    """The fused key histogram (key_hist) filled per unit: the top-k and
    bottom-k selections that read it equal the CPU's."""
    g, c = pair(M.OneMax(1024), s0() + 37)
    g.island.fused_histogram = True
    run3(g, c)
    assert g.island.fused_histogram_ready
    check(g, c)
    assert g.island.fused_histogram_ready


def test_small_population_keeps_rotating_loop():
    """S = 4096: units below 64 children on the 4-wave grid, the rotating
    loop."""
    g, c = pair(M.OneMax(1024), 4096)
    run3(g, c)
    check(g, c)
