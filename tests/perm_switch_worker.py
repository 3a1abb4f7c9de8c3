"""Worker of test_perm_routes.py: the launcher switches PGA_FORCE_GENERIC,
PGA_PERM_NO_FULL and PGA_PERM_PMX_TBL are read once per process, so each is
tried in a process of its own.

    python perm_switch_worker.py CASES.json OUT.npz

CASES.json: a list of {"L", "xo", "S"}.  Builds each TSP island on the GPU,
runs two generations and saves rows<i>, scores<i> and route<i> (Island.route()
as JSON) per case.  run_cases(cases, "cpu") gives the parent the CPU backend's
rows and scores of the same cases.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GENS = 2


def run_cases(cases, device):
    import torch

    import libpga_amd as pga

    out = {}
    for i, case in enumerate(cases):
        p = pga.models.TSP.random_euclidean(case["L"], seed=case["L"])
        ga = pga.GeneticAlgorithm(p, case["S"], seed=11, device=device, crossover=case["xo"], mutation="inversion",
                                  mutation_rate=0.4, elitism=1)
        ga.run(GENS)
        if device != "cpu":
            torch.cuda.synchronize()
        out[f"rows{i}"] = ga.rows.cpu().numpy().copy()
        out[f"scores{i}"] = ga.scores.cpu().numpy().copy()
        out[f"route{i}"] = np.array(json.dumps(ga.island.route()))
    return out


def main(argv):
    with open(argv[1]) as f:
        cases = json.load(f)
    np.savez(argv[2], **run_cases(cases, "cuda:0"))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
