"""REAL tournaments on quantized 16-bit keys (core.hpp qkey, tp.hpp
tp_select_segment<TP_QKEY16>) at adversarial scores and ranges.

The oracle here shares no code with either backend: Philox4x32-10, the ST_SEL
word layout, the tournament, linear ranking and the key quantization are
written out in numpy.  With crossover "none", mutation "none" and no elitism a
child is a copy of its parent A, and every individual's row names it, so the
children of one generation ARE the selection.  Scores are forged independently
of the rows (scores(0) written, then rebest()).

Without a GPU the oracle is proved against the CPU backend; on the GPU the
children of the key path must equal the oracle's and the CPU backend's bit for
bit, the keys must be live, monotone and equal to the numpy quantization, and
every path that rewrites scores must re-key.
"""
import functools
import os
import re
import zlib

import numpy as np
import pytest
import torch

import libpga_amd as pga
from libpga_amd._ext import C
from libpga_amd.parallel import LocalIslands
from philox_np import MASK, U64, philox  # Philox4x32-10 in plain numpy

M = pga.models
F32 = np.float32
U32 = np.uint32
QK_NAN = 0xFFFF


@pytest.fixture(autouse=True)
def _transposed_kernel_at_every_size(monkeypatch):
    # the two-phase kernel (and with it the quantized keys) at every size
    monkeypatch.setenv("PGA_TP_MIN_S", "0")


def _st_sel():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "csrc", "include", "pga", "core.hpp")
    with open(path) as f:
        return int(re.search(r"\bST_SEL\s*=\s*(\d+)", f.read()).group(1))


ST_SEL = _st_sel()


# ------------------------------------------------------------ plain oracle ---
def sel_words(seed, gen, island, S, n):
    """The first n ST_SEL words of children 0..S-1: word t = register t % 4 of block t // 4."""
    child = np.arange(S, dtype=U64)
    out = []
    for block in range((n + 3) // 4):
        out += philox(np.full(S, block | (ST_SEL << 24), dtype=U64), child & MASK,
                      (child >> U64(32)) | U64(island << 16), np.full(S, gen, dtype=U64),
                      seed & 0xFFFFFFFF, seed >> 32)
    return out[:n]


def idx(w, S):
    return ((w * U64(S)) >> U64(32)).astype(np.int64)


def oracle_tournament(s, seed, gen, island=0):
    """(parent A, parent B) of a binary tournament: the first contestant wins
    unless it is strictly below the second (so it wins on equality and on NaN)."""
    S = len(s)
    x, y, z, w = (idx(v, S) for v in sel_words(seed, gen, island, S, 4))
    with np.errstate(invalid="ignore"):
        return np.where(s[x] < s[y], y, x), np.where(s[z] < s[w], w, z)


def score_key(s):
    u = s.view(U32)
    return np.where(u & U32(0x80000000), ~u, u | U32(0x80000000)).astype(U32)


def rank_thresh_of(sp):
    b = 2.0 - float(min(max(F32(sp), F32(1.0)), F32(2.0)))
    t = b * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def oracle_rank(s, seed, gen, sp, island=0):
    S = len(s)
    order = np.argsort(score_key(s), kind="stable")  # ascending (score_key, index)
    w = sel_words(seed, gen, island, S, 6)
    thresh = U64(rank_thresh_of(sp))

    def pick(wb, w1, w2):
        r1, r2 = idx(w1, S), idx(w2, S)
        return np.where(wb < thresh, r1, np.maximum(r1, r2))

    return order[pick(w[0], w[1], w[2])], order[pick(w[3], w[4], w[5])]


def qkey_params(mn, mx):
    """core.hpp qkey_params in f32: a degenerate range (d not in (0, 3e38), or
    mn not above -3e38, NaN included) gives lo = 0, scale = 0."""
    mn, mx = F32(mn), F32(mx)
    with np.errstate(all="ignore"):
        d = F32(mx - mn)
        ok = bool(d > F32(0.0)) and bool(d < F32(3.0e38)) and bool(mn > F32(-3.0e38))
        return (mn, F32(F32(65534.0) / d)) if ok else (F32(0.0), F32(0.0))


def qkey(s, rng):
    """core.hpp qkey in f32: x = (s - lo) * scale; 0xFFFF where x is NaN (a NaN
    score, or an infinite difference times a zero scale), else x clamped to
    [0, 65534] and truncated."""
    lo, scale = qkey_params(rng[0], rng[1])
    with np.errstate(all="ignore"):
        x = ((s - lo).astype(F32) * scale).astype(F32)
        k = np.where(x <= 0, 0, np.where(x >= 65534, 65534, np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)))
        return np.where(np.isnan(x), QK_NAN, k.astype(np.int64)), np.isnan(x)


# ---------------------------------------------------------- score patterns ---
def _gen(name, S):
    return np.random.default_rng(zlib.crc32(name.encode()) * 7 + S)


def _normal(S):
    return _gen("normal", S).standard_normal(S).astype(F32)


def _outlier(name, S, v):
    g = _gen(name, S)
    s = (g.random(S) * 1e-3).astype(F32)
    s[g.integers(0, S)] = v
    return s


def _ulp_ladder(S):
    g = _gen("ulp_ladder", S)
    ladder = np.empty(64, dtype=F32)
    ladder[0] = 1e6
    for k in range(1, 64):
        ladder[k] = np.nextafter(ladder[k - 1], F32(np.inf))
    s = ladder[g.integers(0, 64, S)]
    a, b = g.choice(S, 2, replace=False)
    s[a], s[b] = -1e6, 3e6
    return s


def _nonfinite(S):
    g = _gen("nonfinite", S)
    s = g.standard_normal(S).astype(F32)
    p, n = g.permutation(S), max(1, S // 100)
    u = s.view(U32)
    for j, bits in enumerate((0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000)):  # +inf, -inf, +NaN, -NaN
        u[p[j * n:(j + 1) * n]] = bits
    return s


def _denormal(S):
    g = _gen("denormal", S)
    u = g.integers(1, 1 << 23, S).astype(U32)  # multiples of 2^-149 below 2^-126
    u[g.random(S) < 0.25] = 0                  # zeros
    u |= (g.integers(0, 2, S).astype(U32) << U32(31))  # either sign, -0.0 included
    return u.view(F32)


PATTERNS = {
    "normal": _normal,
    "all_equal": lambda S: np.full(S, 7.0, dtype=F32),
    "two_values": lambda S: _gen("two_values", S).integers(0, 2, S).astype(F32),
    "outlier_hi": lambda S: _outlier("outlier_hi", S, 3e38),
    "outlier_lo": lambda S: _outlier("outlier_lo", S, -3e38),
    "ulp_ladder": _ulp_ladder,
    "nonfinite": _nonfinite,
    "all_nan": lambda S: np.full(S, np.nan, dtype=F32),
    "denormal": _denormal,
    "span_overflow": lambda S: _gen("span_overflow", S).uniform(-3e38, 3e38, S).astype(F32),
    "span_wide": lambda S: _gen("span_wide", S).uniform(-1.4e38, 1.4e38, S).astype(F32),
    "neg_ints": lambda S: (-(_gen("neg_ints", S).permutation(S) + 1)).astype(F32),
}
PHASES = {"fresh": 0, "stale": 1}  # generations run before the scores are forged
SEED = 12345 | (77 << 32)          # both Philox key words in use


def test_patterns_are_what_they_claim():
    S = 5000
    s = {k: f(S) for k, f in PATTERNS.items()}
    assert all(v.dtype == F32 and v.shape == (S,) for v in s.values())
    assert all(np.array_equal(v.view(U32), PATTERNS[k](S).view(U32)) for k, v in s.items())  # seeded
    nf = s["nonfinite"]
    assert np.isposinf(nf).sum() == np.isneginf(nf).sum() == 50 and np.isnan(nf).sum() == 100
    assert (nf.view(U32)[np.isnan(nf)] >> 31).sum() == 50  # half the NaNs carry the sign bit
    d = s["denormal"]
    assert np.abs(d).max() < 2.0 ** -126 and (d == 0).sum() > 100 and np.signbit(d[d == 0]).any()
    assert len(np.unique(np.abs(d))) > 1000
    assert len(np.unique(s["ulp_ladder"])) == 66
    with np.errstate(over="ignore"):
        assert np.isinf(s["span_overflow"].max() - s["span_overflow"].min())
        assert s["span_wide"].max() - s["span_wide"].min() < F32(3.0e38)
    assert sorted(-s["neg_ints"]) == list(range(1, S + 1))


# --------------------------------------------------------- Philox (no GPU) ---
def test_philox_numpy_known_answer():
    """The three Random123 vectors of test_philox_known_answer."""
    def one(*a):
        return tuple(int(v[0]) for v in philox(*[[x] for x in a[:4]], a[4], a[5]))
    f = 0xFFFFFFFF
    assert one(0, 0, 0, 0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert one(f, f, f, f, f, f) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert one(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0) == (
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_philox_numpy_matches_native():
    g = np.random.default_rng(1)
    c = g.integers(0, 1 << 32, (1000, 4), dtype=U64)
    k0, k1 = 0x9ABCDEF0, 0x12345678
    out = np.stack(philox(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k0, k1), axis=1)
    for i in range(1000):
        assert tuple(int(v) for v in out[i]) == C.philox(*[int(v) for v in c[i]], k0, k1)


def test_st_sel_stream_id():
    assert ST_SEL == 8  # the id test_mutation_rate_statistics spells out


# ------------------------------------------------- forged populations ---------
def _problem():
    return M.Sphere(3)  # bounds +-5.12, one 4-gene chunk, a native objective (keys are kept)


def _named_rows(S):
    """Row i names individual i with exact f32 values inside the bounds:
    gene 0 = (i mod 1024) / 128 - 4, gene 1 = (i div 1024) / 128 - 4."""
    assert S <= 1 << 18
    i = np.arange(S)
    rows = np.zeros((S, 4), dtype=F32)
    rows[:, 0] = (i & 1023) / 128.0 - 4.0
    rows[:, 1] = (i >> 10) / 128.0 - 4.0
    rows[:, 2] = 0.5
    return rows


def _forge(ga, rows, scores):
    isl = ga.island
    isl.rows(0).copy_(torch.from_numpy(rows.view(np.int32)))
    isl.scores(0).copy_(torch.from_numpy(scores))
    isl.rebest()


def _rows_np(ga):
    return ga.rows.cpu().numpy().copy()


COPY = dict(crossover="none", mutation="none", elitism=0)      # a child is its parent A
BREED = dict(crossover="two_point", mutation="gaussian", elitism=3)  # both parents, elites


def _forged_generation(device, pattern, phase, S, **ops):
    ga = pga.GeneticAlgorithm(_problem(), S, seed=SEED, device=device, **ops)
    ga.run(PHASES[phase])
    assert ga.generation == PHASES[phase]
    _forge(ga, _named_rows(S), PATTERNS[pattern](S))
    ga.run(1)
    if device != "cpu":
        torch.cuda.synchronize()
    return ga


def _bits(a):
    return a.view(np.int32) if a.dtype == F32 else a


@functools.lru_cache(maxsize=None)
def _cpu_children(pattern, phase, S, breed=False, **sel):
    return _rows_np(_forged_generation("cpu", pattern, phase, S, **(BREED if breed else COPY), **sel))


@functools.lru_cache(maxsize=None)
def _gpu_case(pattern, phase, S):
    """One GPU generation from the forged population (copy operators): the
    children, their scores, and both parities' keys."""
    ga = _forged_generation("cuda:0", pattern, phase, S, **COPY)
    return dict(rows=_rows_np(ga), child_scores=ga.scores.cpu().numpy().copy(), k1=ga.island.qkeys(1),
                k0=ga.island.qkeys(0))


def _expected_children(pattern, phase, S):
    pa, _ = oracle_tournament(PATTERNS[pattern](S), SEED, PHASES[phase])
    return _named_rows(S)[pa].view(np.int32)


@pytest.mark.parametrize("phase", list(PHASES))
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_cpu_tournament_matches_oracle(pattern, phase):
    S = 5000
    assert np.array_equal(_cpu_children(pattern, phase, S), _expected_children(pattern, phase, S))


@pytest.mark.parametrize("sp", [1.0, 1.5, 2.0])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_cpu_rank_matches_oracle(pattern, sp):
    S = 5000
    got = _cpu_children(pattern, "fresh", S, selection="rank", rank_pressure=sp)
    pa, _ = oracle_rank(PATTERNS[pattern](S), SEED, 0, sp)
    assert np.array_equal(got, _named_rows(S)[pa].view(np.int32))


# ------------------------------------------------------------- GPU tests -----
@pytest.mark.gpu
@pytest.mark.parametrize("S", [5000, 4096])  # 5000: a tail segment and a tail unit
@pytest.mark.parametrize("phase", list(PHASES))
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_forged_tournament_matches_oracle_and_cpu(pattern, phase, S):
    """fresh: the range is refreshed from the forged scores (score_stats);
    stale: it is the initial population's (about [-79, 0]), the forged scores
    lie outside it or inside few bins.  Children == CPU backend == oracle."""
    got = _gpu_case(pattern, phase, S)["rows"]
    exp = _expected_children(pattern, phase, S)
    cpu = _cpu_children(pattern, phase, S)
    bad = np.flatnonzero((got != exp).any(-1))
    assert bad.size == 0, f"{bad.size} children differ from the oracle, first {bad[:8]}"
    assert np.array_equal(got, cpu)
    # both parents, the mutation stream and the elites (NaN / inf bests) against the CPU backend
    g = _forged_generation("cuda:0", pattern, phase, S, **BREED)
    c = _cpu_children(pattern, phase, S, breed=True)
    bad = np.flatnonzero((_rows_np(g) != c).any(-1))
    assert bad.size == 0, f"{bad.size} bred children differ from the CPU backend, first {bad[:8]}"


def _assert_monotone(keys, scores, what):
    ok = ~np.isnan(scores)
    order = np.argsort(score_key(scores[ok]), kind="stable")  # ascending score; -0.0 before +0.0
    s, k = scores[ok][order], keys[ok][order]
    # equal scores (-0.0 == 0.0 too) must share a key: compare runs of equal scores as a whole
    with np.errstate(invalid="ignore"):
        live = k != QK_NAN
        s, k = s[live], k[live]
        assert np.all(np.diff(k) >= 0), f"{what}: keys decrease along ascending scores"
        same = s[1:] == s[:-1]
        assert np.all(k[1:][same] == k[:-1][same]), f"{what}: equal scores, different keys"


def _check_keys(case, scores_forged, pattern, phase):
    assert case["k1"] is not None, "the forged generation was not selected on quantized keys"
    assert case["k0"] is not None, "the generation kernel wrote no keys for its children"
    for which, scores in ((1, scores_forged), (0, case["child_scores"])):
        keys, rng = (t.numpy() for t in case[f"k{which}"])
        assert keys.dtype == np.int32 and keys.shape == scores.shape
        exp, xnan = qkey(scores, rng)
        # 0xFFFF exactly where (s - lo) * scale is NaN: every NaN score, and a
        # non-NaN score only when that product is NaN (+-inf under a degenerate
        # range, scale 0; or an infinite range end)
        assert np.array_equal(keys == QK_NAN, xnan), f"which={which}: 0xFFFF keys misplaced"
        assert np.all(xnan[np.isnan(scores)])
        _assert_monotone(keys, scores, f"which={which}")
        # the re-keying launch (which=1) and the generation kernel's stores
        # (which=0) both are core.hpp qkey over the reported range
        bad = np.flatnonzero(keys != exp)
        assert bad.size == 0, f"which={which}: {bad.size} keys differ from qkey(), first {bad[:8]}"
    keys, rng = (t.numpy() for t in case["k1"])
    if pattern == "normal" and phase == "fresh":
        # the range is exactly the population's; 65534 / d is rounded once (a
        # relative 2^-24, below 0.004 of a key step at 65534), so truncation
        # loses at most one step at the top
        assert rng[0] == scores_forged.min() and rng[1] == scores_forged.max()
        assert keys.min() == 0 and keys.max() >= 65533
    if phase == "fresh" and pattern in ("all_equal", "span_overflow", "all_nan"):
        live = keys[keys != QK_NAN]
        assert live.size == 0 or np.all(live == live[0])
        assert pattern != "all_nan" or live.size == 0


@pytest.mark.gpu
@pytest.mark.parametrize("phase", list(PHASES))
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_keys_are_live_and_monotone(pattern, phase):
    S = 5000
    _check_keys(_gpu_case(pattern, phase, S), PATTERNS[pattern](S), pattern, phase)


@pytest.mark.gpu
@pytest.mark.parametrize("phase", list(PHASES))
@pytest.mark.parametrize("pattern", ["normal", "nonfinite", "neg_ints"])
def test_large_population_default_route(pattern, phase, monkeypatch):
    """S = 2^18 with the default routing: the 8-generation refresh cadence."""
    monkeypatch.delenv("PGA_TP_MIN_S", raising=False)
    S = 1 << 18
    g = _forged_generation("cuda:0", pattern, phase, S, **COPY)
    assert g.island.qkeys(1) is not None and g.island.qkeys(0) is not None
    got = _rows_np(g)
    exp = _expected_children(pattern, phase, S)
    bad = np.flatnonzero((got != exp).any(-1))
    assert bad.size == 0, f"{bad.size} children differ from the oracle, first {bad[:8]}"
    c = _forged_generation("cpu", pattern, phase, S, **COPY)
    assert np.array_equal(got, _rows_np(c))


def _lockstep(g, c, gens, what=""):
    for k in range(gens):
        g.run(1)
        c.run(1)
        torch.cuda.synchronize()
        assert torch.equal(g.rows.cpu(), c.rows), f"{what}rows differ after generation {g.generation} (step {k + 1})"
        assert torch.equal(g.scores.cpu(), c.scores), f"{what}scores differ after generation {g.generation}"
        assert g.island.qkeys(0) is not None, f"{what}no valid keys after generation {g.generation}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere30", "rosen30", "sphere3_256k"])
def test_bitexact_across_refresh(name):
    """Rows and scores against the CPU backend after every generation, across
    the range refreshes (generation 33 below 2^18 children, from the fused
    partials; 9 and 17 at 2^18)."""
    p, S, gens = {"sphere30": (M.Sphere(30), 3000, 40), "rosen30": (M.Rosenbrock(30), 3000, 40),
                  "sphere3_256k": (M.Sphere(3), 1 << 18, 20)}[name]
    kw = dict(seed=21, elitism=1, crossover="blend", mutation="gaussian")
    g = pga.GeneticAlgorithm(p, S, device="cuda:0", **kw)
    c = pga.GeneticAlgorithm(p, S, device="cpu", **kw)
    _lockstep(g, c, gens)


def _rewrite(how, g, c, tmp_path):
    """The same score rewrite on the GPU island g and the CPU island c."""
    S, rw = g.pop_size, int(g.island.row_words)
    rng = np.random.default_rng(5)
    if how == "scatter":
        n = 200
        victims = torch.from_numpy(rng.choice(S, n, replace=False).astype(np.int32))
        rows = rng.uniform(-5, 5, (n, rw)).astype(F32)
        rows[:, g.problem.length:] = 0
        rows = torch.from_numpy(rows.view(np.int32))
        sc = np.where(rng.random(n) < 0.5, 1e6, -1e6).astype(F32)  # far outside the stale range on both sides
        sc[:8] = np.nan
        sc[8:16] = np.inf
        sc = torch.from_numpy(sc)
        for ga in (g, c):
            d = ga.device
            ga.island.scatter(victims.to(d), rows.to(d).contiguous(), sc.to(d))
    elif how == "immigrate":
        k = 64
        src = pga.GeneticAlgorithm(g.problem, S, seed=99, device="cpu", elitism=1)
        src.run(5)
        rows, sc = torch.empty(k * rw, dtype=torch.int32), torch.empty(k, dtype=torch.float32)
        src.island.emigrate(k, rows, sc)
        for ga in (g, c):
            ga.island.immigrate(k, rows.to(ga.device), sc.to(ga.device))
    elif how == "load":
        path = str(tmp_path / "gen5.ckpt")
        g.save(path)
        for ga in (g, c):
            ga.load(path)
    else:
        rows = torch.from_numpy(rng.uniform(-5, 5, (S, rw)).astype(F32))
        rows[:, g.problem.length:] = 0
        for ga in (g, c):
            ga.island.rows(0).copy_(rows.view(torch.int32))
            ga.evaluate()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["scatter", "immigrate", "load", "evaluate"])
def test_rekey_after_score_rewrite(how, tmp_path):
    """A rewrite of the scores at generation 5 (the range is 5 generations
    stale) invalidates the keys; the next generation re-keys and stays bit
    exact against a CPU island given the same treatment."""
    p, S = M.Sphere(30), 3000
    kw = dict(seed=17, elitism=1, crossover="blend", mutation="gaussian")
    g = pga.GeneticAlgorithm(p, S, device="cuda:0", **kw)
    c = pga.GeneticAlgorithm(p, S, device="cpu", **kw)
    _lockstep(g, c, 5)
    _rewrite(how, g, c, tmp_path)
    torch.cuda.synchronize()
    assert g.island.qkeys(0) is None, "keys of rewritten scores still count as valid"
    assert torch.equal(g.rows.cpu(), c.rows) and torch.equal(g.scores.cpu().view(torch.int32), c.scores.view(torch.int32))
    if how == "load":
        # a fresh island resumed from the checkpoint refreshes its range at
        # another phase than the one that ran on: the same children anyway
        r = pga.GeneticAlgorithm(p, S, device="cuda:0", **kw)
        r.load(str(tmp_path / "gen5.ckpt"))
        assert r.generation == 5
    _lockstep(g, c, 5, what=f"after {how}: ")
    if how == "load":
        g.run(5)
        r.run(10)
        torch.cuda.synchronize()
        assert g.generation == r.generation == 15
        assert torch.equal(g.rows, r.rows) and torch.equal(g.scores, r.scores)
    # the keys of the last generation are the quantization of its scores
    keys, rng = (t.numpy() for t in g.island.qkeys(0))
    assert np.array_equal(keys, qkey(g.scores.cpu().numpy(), rng)[0])


@pytest.mark.gpu
def test_batched_islands_across_refresh():
    """Eight REAL islands in one launch per generation against the same
    islands on their own streams, over 40 generations: migration every 5
    (the immigrants re-key) and the refresh of each island's range at 33."""
    common = dict(seed=5, device="cuda:0", migrate_every=5, migrate_pct=0.02, elitism=1)
    a = LocalIslands(M.Sphere(30), 8, 4096, **common)
    b = LocalIslands(M.Sphere(30), 8, 4096, batched=False, **common)
    a.run(40)
    b.run(40)
    torch.cuda.synchronize()
    assert a.batched_generations == 40 and b.batched_generations == 0
    for x, y in zip(a.islands, b.islands):
        assert torch.equal(x.rows, y.rows) and torch.equal(x.scores, y.scores)
        assert x.best_score() == y.best_score()
    assert a.migrations == b.migrations == 8
