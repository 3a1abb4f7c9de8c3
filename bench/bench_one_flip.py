#!/usr/bin/env python3
"""Cost and effect of the one-flip local search stage of the QUBO objective
(Island::local_search on BINARY / OBJ_QUBO, csrc/kernels/qubo_ls.hip).

Instances: bench_configs' maxcut512_qubo (population 1M) and qubo1024
(population 256K), elitism 1.  Measures per instance, each over `--reps`
windows after a warm-up, with a device synchronise closing every window:

  generation   ms per generation with the option off, on this tree and (with
               --parent ROOT, a built checkout of the parent commit) on the
               parent, in fresh processes that alternate between the two
  stage        ms per local_search(moves, prob) on a freshly initialised
               population, at (1, 1.0), (8, 1.0), (1, 0.05), (8, 0.05), also in
               multiples of the plain generation measured in the same process
  loop         ms per generation of run() with local_search="one_flip" at (8, 0.05)
  quality      best score after --quality-gens generations with and without
               the option at (8, 0.05), same seed

Prints one JSON line and writes the report to --out (markdown).

    python bench/bench_one_flip.py --parent ../parent-checkout --out profiles/one_flip.md
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
STAGES = [(1, 1.0), (8, 1.0), (1, 0.05), (8, 0.05)]


def instance(name):
    from libpga_amd import models as M

    if name == "maxcut512_qubo":
        return M.MaxCut.random_graph(512, degree=16, seed=1), 1 << 20, 50
    if name == "qubo1024":
        return M.QUBO.random(1024, seed=1, lo=-128, hi=127), 1 << 18, 20
    raise KeyError(name)


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
    import libpga_amd as pga

    out = {}
    for name in a.configs:
        p, pop, gens = instance(name)
        pop = min(pop, a.max_pop)
        ga = pga.GeneticAlgorithm(p, pop, seed=1, device=a.device, elitism=1)
        ga.run(a.warmup)
        out[name] = windows(lambda: ga.run(gens) or gens, a.reps, ga.synchronize)
    print(json.dumps({"ms": out, "root": os.path.dirname(pga.__path__[0])}))


def run_child(root, a):
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup),
           "--device", a.device, "--max-pop", str(a.max_pop), "--configs", *a.configs]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"generation child failed in {root}:\n{r.stderr[-2000:]}")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.samefile(res["root"], root), (res["root"], root)
    return res["ms"]


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["maxcut512_qubo", "qubo1024"])
    ap.add_argument("--max-pop", type=int, default=1 << 30, help="cap on the populations (rehearsals)")
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
        raise SystemExit("bench_one_flip needs a GPU")
    sync = torch.cuda.synchronize if a.device != "cpu" else (lambda: None)
    res = {"reps": a.reps, "warmup": a.warmup, "configs": {}}

    # ---- the generation alone, this tree and the parent alternating ----
    this_ms = {n: [] for n in a.configs}
    parent_ms = {n: [] for n in a.configs}
    for _ in range(a.rounds):
        for n, v in run_child(ROOT, a).items():
            this_ms[n] += v
        if a.parent:
            for n, v in run_child(os.path.abspath(a.parent), a).items():
                parent_ms[n] += v

    for name in a.configs:
        p, pop, gens = instance(name)
        pop = min(pop, a.max_pop)
        kw = dict(seed=1, device=a.device, elitism=1)
        r = {"pop": pop, "bits": p.length, "gens_per_window": gens, "generation_ms": spread(this_ms[name])}
        if parent_ms[name]:
            r["generation_parent_ms"] = spread(parent_ms[name])

        # ---- the plain generation in this process: the unit of the stage's cost ----
        ga = pga.GeneticAlgorithm(p, pop, **kw)
        ga.run(a.warmup)
        r["generation_here_ms"] = spread(windows(lambda: ga.run(gens) or gens, a.reps, sync))
        del ga

        # ---- the stage alone ----
        r["stage_ms"] = {}
        for moves, prob in STAGES:
            ms = []
            for rep in range(a.stage_reps + 1):  # fresh random rows each time; the first is the warm-up
                ga = pga.GeneticAlgorithm(p, pop, **dict(kw, seed=100 + rep))
                one = windows(lambda: ga.local_search(moves, prob) or 1, 1, sync)
                if rep:
                    ms += one
            r["stage_ms"][f"{moves},{prob}"] = spread(ms)

        # ---- the loop with the option ----
        ga = pga.GeneticAlgorithm(p, pop, local_search="one_flip", ls_moves=8, ls_prob=0.05, **kw)
        ga.run(a.warmup)
        r["loop_ms"] = spread(windows(lambda: ga.run(gens) or gens, a.reps, sync))
        del ga

        # ---- quality ----
        off = pga.GeneticAlgorithm(p, pop, **kw)
        on = pga.GeneticAlgorithm(p, pop, local_search="one_flip", ls_moves=8, ls_prob=0.05, **kw)
        first = off.best_score()
        off.run(a.quality_gens)
        on.run(a.quality_gens)
        r["quality"] = {"generations": a.quality_gens, "initial_best": first, "ga": off.best_score(),
                        "ga_one_flip_8_0.05": on.best_score()}
        del off, on
        res["configs"][name] = r
    print(json.dumps(res))

    if a.out:
        f3 = lambda d: f"{d['median']:.3f} ({d['min']:.3f} .. {d['max']:.3f})"  # noqa: E731
        L = ["# One-flip local search stage (QUBO / Max-Cut): cost and effect", "",
             "`python bench/bench_one_flip.py` on one MI355X, elitism 1, the other operators at their defaults.",
             "Times are host clock around work closed by a device synchronise, median (min .. max) in ms;",
             f"generation windows are the configuration's step count after {a.warmup} warm-up generations.", ""]
        for name, r in res["configs"].items():
            g, gh, q = r["generation_ms"], r["generation_here_ms"], r["quality"]
            L += [f"## {name}: {r['bits']} bits, population {r['pop']}", "",
                  "### The generation alone (option off)", "",
                  f"| Tree | ms per generation, {g['n']} windows of {r['gens_per_window']} generations in {a.rounds} "
                  "fresh processes |", "|---|---|", f"| this commit | {f3(g)} |"]
            if "generation_parent_ms" in r:
                gp = r["generation_parent_ms"]
                noise = gp["max"] - gp["min"]
                diff = g["median"] - gp["median"]
                L += [f"| parent commit | {f3(gp)} |", "",
                      f"The margin: the parent's own windows spread over {noise:.3f} ms "
                      f"({100 * noise / gp['median']:.1f} % of its median).  The medians differ by {diff:+.3f} ms "
                      f"({100 * diff / gp['median']:+.2f} %): " +
                      ("this commit is SLOWER than the parent by more than that spread."
                       if diff > noise else "inside that spread.") + "  The processes alternated (this, parent, ...)."]
            else:
                L += ["", "The parent commit was not measured in this run (no --parent)."]
            L += ["", "### The stage alone", "",
                  "One `local_search(moves, prob)` on a freshly initialised (random) population, "
                  f"{a.stage_reps} populations each; the plain generation in the same process took {f3(gh)} ms.", "",
                  "| moves, prob | ms per stage | generations' worth |", "|---|---|---|"]
            for k, v in r["stage_ms"].items():
                L.append(f"| {k} | {f3(v)} | {v['median'] / gh['median']:.1f} |")
            L += ["", "### The loop with the option", "",
                  f"`run()` with `local_search=\"one_flip\", ls_moves=8, ls_prob=0.05`: {f3(r['loop_ms'])} ms per "
                  f"generation ({r['loop_ms']['median'] / gh['median']:.2f} x the plain generation).", "",
                  "### Quality", "",
                  f"Best score after {q['generations']} generations from the same initial population "
                  f"(initial best {q['initial_best']:.0f}):", "",
                  "| | best score |", "|---|---|",
                  f"| GA | {q['ga']:.0f} |", f"| GA + one-flip (8 moves, prob 0.05) | {q['ga_one_flip_8_0.05']:.0f} |", ""]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(L))


if __name__ == "__main__":
    main()
