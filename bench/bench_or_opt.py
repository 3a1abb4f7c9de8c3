#!/usr/bin/env python3
"""Cost and effect of the Or-opt local search stage (Island::local_search with
LS_OR_OPT, csrc/kernels/perm_ls.hip perm_oropt_kernel).

Instances: bench_two_opt's TSP-256 (symmetric f32 matrix, population 256K, OX,
elitism 1) and the reference's E3 family at 100 cities (asymmetric integer
matrix, open path, planted path of length 990; population 40,000).  Measures,
each over `--reps` windows after a warm-up, with a device synchronise closing
every window:

  generation   ms per TSP-256 generation with the option off, on this tree and
               (with --parent ROOT, a built checkout of the parent commit) on
               the parent, in fresh processes that alternate between the two
  stage        ms per local_search(moves, prob, kind="or_opt") on a freshly
               initialised population, at (1, 1.0), (1, 0.05), (8, 0.05), on
               both instances (and 2-opt at (1, 1.0) on TSP-256 beside it)
  loop         ms per generation of run() with local_search="or_opt" at (1, 0.05)
  quality      best length after --quality-gens generations: the GA, GA + 2-opt
               and GA + Or-opt at (8, 0.05) on TSP-256; the GA and GA + Or-opt
               on E3-100

Prints one JSON line and writes the report to --out (markdown).

    python bench/bench_or_opt.py --parent ../parent-checkout --out profiles/or_opt.md
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_two_opt import instance, run_child, spread, windows  # noqa: E402  (its generation child serves both)

GRID = [(1, 1.0), (1, 0.05), (8, 0.05)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=1 << 18)
    ap.add_argument("--e3-pop", type=int, default=40000)
    ap.add_argument("--gens", type=int, default=50, help="generations per timed window")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the generation processes")
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--quality-gens", type=int, default=50)
    ap.add_argument("--parent", default=None, help="root of a built checkout of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0", help="cpu: a rehearsal of the script, not a measurement")
    a = ap.parse_args()

    sys.path.insert(0, ROOT)
    import torch
    import libpga_amd as pga
    from libpga_amd import models as M

    if a.device != "cpu" and not torch.cuda.is_available():
        raise SystemExit("bench_or_opt needs a GPU")
    res = {"pop": a.pop, "e3_pop": a.e3_pop, "gens_per_window": a.gens, "reps": a.reps}

    # ---- the generation alone, this tree and the parent alternating ----
    this_ms, parent_ms = [], []
    for _ in range(a.rounds):
        this_ms += run_child(ROOT, a)
        if a.parent:
            parent_ms += run_child(os.path.abspath(a.parent), a)
    res["generation_ms"] = spread(this_ms)
    if parent_ms:
        res["generation_parent_ms"] = spread(parent_ms)

    sync = torch.cuda.synchronize if a.device != "cpu" else (lambda: None)
    kw = dict(seed=1, device=a.device, elitism=1, crossover="ox")
    cases = {"tsp256": (instance(), a.pop), "e3_100": (M.TSP.reference_e3(100), a.e3_pop)}
    for name, (p, pop) in cases.items():
        r = res[name] = {}
        # the plain generation in this process: what the stage is measured in
        ga = pga.GeneticAlgorithm(p, pop, **kw)
        ga.run(a.warmup)
        r["generation_ms"] = spread(windows(lambda: ga.run(a.gens) or a.gens, a.reps, sync))

        # ---- the stage alone ----
        r["stage_ms"] = {}
        grid = [("or_opt", m, pr) for m, pr in GRID] + ([("two_opt", 1, 1.0)] if name == "tsp256" else [])
        for kind, moves, prob in grid:
            ms = []
            for rep in range(a.stage_reps + 1):  # fresh random tours each time; the first is the warm-up
                ga = pga.GeneticAlgorithm(p, pop, **dict(kw, seed=100 + rep))
                one = windows(lambda: ga.local_search(moves, prob, kind=kind) or 1, 1, sync)
                if rep:
                    ms += one
            r["stage_ms"][f"{kind},{moves},{prob}"] = spread(ms)

        # ---- the loop with the option ----
        ga = pga.GeneticAlgorithm(p, pop, local_search="or_opt", ls_moves=1, ls_prob=0.05, **kw)
        ga.run(a.warmup)
        r["loop_ms"] = spread(windows(lambda: ga.run(a.gens) or a.gens, a.reps, sync))

        # ---- quality ----
        off = pga.GeneticAlgorithm(p, pop, **kw)
        q = r["quality"] = {"generations": a.quality_gens, "initial_best": -off.best_score()}
        off.run(a.quality_gens)
        q["ga"] = -off.best_score()
        for kind in (["two_opt"] if name == "tsp256" else []) + ["or_opt"]:
            on = pga.GeneticAlgorithm(p, pop, local_search=kind, ls_moves=8, ls_prob=0.05, **kw)
            on.run(a.quality_gens)
            q[f"ga_{kind}_8_0.05"] = -on.best_score()
    res["e3_100"]["quality"]["planted"] = 990.0
    print(json.dumps(res))

    if a.out:
        g = res["generation_ms"]
        f3 = lambda d: f"{d['median']:.3f} ({d['min']:.3f} .. {d['max']:.3f})"  # noqa: E731
        L = ["# Or-opt local search stage: cost and effect", "",
             f"`python bench/bench_or_opt.py` on one MI355X.  TSP-256: symmetric f32 matrix, population {a.pop}; E3-100:",
             f"`TSP.reference_e3(100)`, asymmetric integer matrix, open path, population {a.e3_pop}; both OX, elitism 1.",
             "Times are host clock around work closed by a device synchronise, median (min .. max) in ms;",
             f"generation windows are {a.gens} generations after {a.warmup} warm-up generations.", "",
             "## The generation alone (option off, TSP-256)", "",
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
        titles = {"tsp256": f"TSP-256, population {a.pop}", "e3_100": f"E3-100, population {a.e3_pop}"}
        for name, title in titles.items():
            r = res[name]
            gm = r["generation_ms"]["median"]
            L += ["", f"## The stage alone: {title}", "",
                  "One `local_search(moves, prob, kind)` on a freshly initialised (random) population, "
                  f"{a.stage_reps} populations each; the plain generation in the same process took {f3(r['generation_ms'])} ms.", "",
                  "| kind, moves, prob | ms per stage | generations' worth |", "|---|---|---|"]
            for k, v in r["stage_ms"].items():
                L.append(f"| {k} | {f3(v)} | {v['median'] / gm:.1f} |")
            L += ["", f"`run()` with `local_search=\"or_opt\", ls_moves=1, ls_prob=0.05`: {f3(r['loop_ms'])} ms per generation "
                  f"({r['loop_ms']['median'] / gm:.2f} x the plain generation)."]
        n = 256
        L += ["", f"A best-improvement Or-opt move scans {n * n // 1000}K (p, q) pairs per tour at {n} cities, six distance lookups and",
              "up to five gains each; a 2-opt move half as many pairs with two lookups and one gain."]
        q, e = res["tsp256"]["quality"], res["e3_100"]["quality"]
        L += ["", "## Quality", "",
              f"Best length after {q['generations']} generations from the same initial population, the stage at 8 moves, "
              "prob 0.05:", "",
              "| | TSP-256 best tour | E3-100 best path |", "|---|---|---|",
              f"| initial population | {q['initial_best']:.3f} | {e['initial_best']:.0f} |",
              f"| GA | {q['ga']:.3f} | {e['ga']:.0f} |",
              f"| GA + 2-opt | {q['ga_two_opt_8_0.05']:.3f} | refused (asymmetric matrix) |",
              f"| GA + Or-opt | {q['ga_or_opt_8_0.05']:.3f} | {e['ga_or_opt_8_0.05']:.0f} |",
              f"| planted path | | {e['planted']:.0f} |", ""]
        with open(a.out, "w") as f:
            f.write("\n".join(L))


if __name__ == "__main__":
    main()
