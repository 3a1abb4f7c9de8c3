#!/usr/bin/env python3
"""Cost and effect of the 2-opt local search stage (Island::local_search).

Instance: bench_configs' tsp256_ox (256 cities, symmetric f32 matrix,
population 256K, OX, elitism 1).  Measures, each over `--reps` windows after a
warm-up, with a device synchronise closing every window:

  generation   ms per generation with the option off, on this tree and (with
               --parent ROOT, a built checkout of the parent commit) on the
               parent, in fresh processes that alternate between the two
  stage        ms per local_search(moves, prob) on a freshly initialised
               population, at (1, 1.0), (1, 0.05), (8, 0.05)
  loop         ms per generation of run() with local_search="two_opt" at (1, 0.05)
  quality      best tour length after --quality-gens generations with and
               without the option at (8, 0.05)

Prints one JSON line and writes the report to --out (markdown).

    python bench/bench_two_opt.py --parent ../parent-checkout --out profiles/two_opt.md
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def instance():
    import torch
    from libpga_amd import models as M

    g = torch.Generator().manual_seed(7)
    xy = torch.rand(256, 2, generator=g)
    return M.TSP(torch.cdist(xy, xy, compute_mode="donot_use_mm_for_euclid_dist"))


def windows(fn, reps, sync):
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        n = fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / n)
    return out


def child_generation(a):
    """ms per generation, option off, with whichever libpga_amd is first on sys.path."""
    import torch
    import libpga_amd as pga

    ga = pga.GeneticAlgorithm(instance(), a.pop, seed=1, device=a.device, elitism=1, crossover="ox")
    ga.run(a.warmup)

    def gens():
        ga.run(a.gens)
        return a.gens

    print(json.dumps({"ms": windows(gens, a.reps, ga.synchronize), "root": os.path.dirname(pga.__path__[0])}))


def run_child(root, a):
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--pop", str(a.pop), "--gens", str(a.gens),
           "--reps", str(a.reps), "--warmup", str(a.warmup), "--device", a.device]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"generation child failed in {root}:\n{r.stderr[-2000:]}")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.samefile(res["root"], root), (res["root"], root)
    return res["ms"]


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=1 << 18)
    ap.add_argument("--gens", type=int, default=50, help="generations per timed window")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the generation processes")
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--quality-gens", type=int, default=50)
    ap.add_argument("--parent", default=None, help="root of a built checkout of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0", help="cpu: a rehearsal of the script, not a measurement")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child_generation(a)

    sys.path.insert(0, ROOT)
    import torch
    import libpga_amd as pga

    if a.device != "cpu" and not torch.cuda.is_available():
        raise SystemExit("bench_two_opt needs a GPU")
    res = {"pop": a.pop, "cities": 256, "gens_per_window": a.gens, "reps": a.reps}

    # ---- the generation alone, this tree and the parent alternating ----
    this_ms, parent_ms = [], []
    for _ in range(a.rounds):
        this_ms += run_child(ROOT, a)
        if a.parent:
            parent_ms += run_child(os.path.abspath(a.parent), a)
    res["generation_ms"] = spread(this_ms)
    if parent_ms:
        res["generation_parent_ms"] = spread(parent_ms)

    # ---- the stage alone ----
    p = instance()
    kw = dict(seed=1, device=a.device, elitism=1, crossover="ox")
    sync = torch.cuda.synchronize if a.device != "cpu" else (lambda: None)
    res["stage_ms"] = {}
    for moves, prob in [(1, 1.0), (1, 0.05), (8, 0.05)]:
        ms = []
        for rep in range(a.stage_reps + 1):  # fresh random tours each time; the first is the warm-up
            ga = pga.GeneticAlgorithm(p, a.pop, **dict(kw, seed=100 + rep))
            one = windows(lambda: ga.local_search(moves, prob) or 1, 1, sync)
            if rep:
                ms += one
        res["stage_ms"][f"{moves},{prob}"] = spread(ms)

    # ---- the loop with the option ----
    ga = pga.GeneticAlgorithm(p, a.pop, local_search="two_opt", ls_moves=1, ls_prob=0.05, **kw)
    ga.run(a.warmup)
    res["loop_ms"] = spread(windows(lambda: ga.run(a.gens) or a.gens, a.reps, sync))

    # ---- quality ----
    off = pga.GeneticAlgorithm(p, a.pop, **kw)
    on = pga.GeneticAlgorithm(p, a.pop, local_search="two_opt", ls_moves=8, ls_prob=0.05, **kw)
    first = -off.best_score()
    off.run(a.quality_gens)
    on.run(a.quality_gens)
    res["quality"] = {"generations": a.quality_gens, "initial_best": first, "ga": -off.best_score(),
                      "ga_two_opt_8_0.05": -on.best_score()}
    print(json.dumps(res))

    if a.out:
        g, st, q = res["generation_ms"], res["stage_ms"], res["quality"]
        f3 = lambda d: f"{d['median']:.3f} ({d['min']:.3f} .. {d['max']:.3f})"  # noqa: E731
        L = ["# 2-opt local search stage: cost and effect", "",
             f"`python bench/bench_two_opt.py` on one MI355X: TSP-256 (symmetric f32 matrix), population {a.pop}, OX,",
             f"elitism 1.  Times are host clock around work closed by a device synchronise, median (min .. max)",
             f"in ms; generation windows are {a.gens} generations after {a.warmup} warm-up generations.", "",
             "## The generation alone (option off)", "",
             f"| Tree | ms per generation, {len(this_ms)} windows in {a.rounds} fresh processes |", "|---|---|",
             f"| this commit | {f3(g)} |"]
        if parent_ms:
            gp = res["generation_parent_ms"]
            noise = gp["max"] - gp["min"]
            L += [f"| parent commit | {f3(gp)} |", "",
                  f"The parent's own windows spread over {noise:.3f} ms ({100 * noise / gp['median']:.1f} % of its median);",
                  f"the medians differ by {g['median'] - gp['median']:+.3f} ms "
                  f"({100 * (g['median'] - gp['median']) / gp['median']:+.2f} %).  The processes alternated (this, parent, ...)."]
        else:
            L += ["", "The parent commit was not measured in this run (no --parent)."]
        L += ["", "## The stage alone", "",
              "One `local_search(moves, prob)` on a freshly initialised (random) population, "
              f"{a.stage_reps} populations each.", "",
              "| moves, prob | ms per stage | generations' worth |", "|---|---|---|"]
        for k, v in st.items():
            L.append(f"| {k} | {f3(v)} | {v['median'] / g['median']:.1f} |")
        L += ["", "An all-pairs best-improvement move is ~32K gains per tour at 256 cities.", "",
              "## The loop with the option", "",
              f"`run()` with `local_search=\"two_opt\", ls_moves=1, ls_prob=0.05`: {f3(res['loop_ms'])} ms per generation "
              f"({res['loop_ms']['median'] / g['median']:.2f} x the plain generation).", "",
              "## Quality", "",
              f"Best tour length after {q['generations']} generations from the same initial population "
              f"(initial best {q['initial_best']:.3f}):", "",
              "| | best tour length |", "|---|---|",
              f"| GA | {q['ga']:.3f} |", f"| GA + 2-opt (8 moves, prob 0.05) | {q['ga_two_opt_8_0.05']:.3f} |", ""]
        with open(a.out, "w") as f:
            f.write("\n".join(L))


if __name__ == "__main__":
    main()
