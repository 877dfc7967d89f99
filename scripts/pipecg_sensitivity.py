#!/usr/bin/env python3
"""How far the pipelined-CG restatement (tests/pipecg_restatement.py) moves when every inner
product, norm and mean is summed in another order: each case of tests/pipecg_cases.py under numpy's
pairwise sums, left-to-right sums and exactly rounded sums (CPU only). Per case:

  d_hist        the largest history difference between two variants (fgmres_cases.hist_diff)
  d_x           the largest solution difference, relative to max |x|
  resid         ||b - A x|| / ||b|| of the pairwise run
  same_outcome  whether all variants ended with the same reason and iteration count

Pipelined CG's recurrences (r, u, w are never recomputed from x) are more sensitive to the
summation order than CG's deep into a solve, so the GPU tests take their bars from these numbers
(100 x d, never below the CG bars). Writes profiles/ksp_pipecg/sensitivity.json.

  python scripts/pipecg_sensitivity.py [case-id-prefix ...]
"""
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import pipecg_cases as F  # noqa: E402

VARIANTS = ("pairwise", "sequential", "exact")


def measure(cid):
    prob, b, _ = F.setup(cid)
    runs = {s: F.restated(cid, s) for s in VARIANTS}
    d_hist = d_x = 0.0
    same = len({(r[1], r[2]) for r in runs.values()}) == 1
    for a, c in itertools.combinations(VARIANTS, 2):
        ra, rc = runs[a], runs[c]
        n = min(len(ra[3]), len(rc[3]))
        d_hist = max(d_hist, F.hist_diff(prob, ra[3][:n], rc[3][:n]))
        d_x = max(d_x, F.x_diff(ra[0], rc[0]))
    x, reason, its, _, _ = runs["pairwise"]
    nranks = F.CASES[cid][2].get("nranks", 1)
    return {"d_hist": d_hist, "d_x": d_x, "resid": F.true_residual(prob, b, x, nranks),
            "same_outcome": same, "reason": int(reason), "its": int(its)}


def main():
    want = sys.argv[1:]
    out = {}
    if want and os.path.exists(F.SENSITIVITY):
        out = json.load(open(F.SENSITIVITY))["cases"]
    for cid in F.CASES:
        if want and not any(cid.startswith(w) for w in want):
            continue
        out[cid] = measure(cid)
        print(cid, json.dumps(out[cid]), flush=True)
    os.makedirs(os.path.dirname(F.SENSITIVITY), exist_ok=True)
    with open(F.SENSITIVITY, "w") as f:
        json.dump({"variants": list(VARIANTS),
                   "about": "scripts/pipecg_sensitivity.py: spread of the pipelined-CG restatement "
                            "between summation orders, per case of tests/pipecg_cases.py",
                   "cases": out}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
