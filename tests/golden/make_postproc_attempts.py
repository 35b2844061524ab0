"""Regenerates tests/golden/postproc_attempts.json: for every committed case of tests/postproc_ref.py, how often each head row had to be
redrawn until the fp64 reference alone finds every decision of the case decided (with 5 % of reserve over the tests' margin).  Minutes of
CPU; the tests load the table and prove decidedness again in one evaluation.  Prints the tightest pair margin per threshold."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import postproc_ref as R  # noqa: E402

if __name__ == "__main__":
    R.SEARCH["on"] = True
    R.all_cases()
    with open(R.ATTEMPTS, "w") as f:
        json.dump(R.SEARCH["found"], f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    tight = {t: (float("inf"), None) for t in R.THRESHOLDS}
    for key, val in R._CACHE.items():
        if key.startswith("matrix"):
            for b, c in enumerate(val[1]):
                for t in R.THRESHOLDS:
                    m = R.pair_report(c, t)["margin"]
                    if m < tight[t][0]:
                        tight[t] = (m, f"{key} image {b}")
    for t, (m, where) in tight.items():
        print(f"iou {t}: tightest pair margin {m:.2f} ({where})")
