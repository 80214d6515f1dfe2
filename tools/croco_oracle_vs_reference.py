#!/usr/bin/env python
"""The C oracle's CROCO kernels (oracle/parcels_oracle.c) against the live reference over the seeded cases of oracle/croco_cases.py, bit for
bit: the record behind profiles/croco_oracle_vs_reference.txt.

    python tools/croco_oracle_vs_reference.py FIRST_SEED N_SEEDS [N_POINT_SEEDS]
"""

import collections
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import c_oracle, croco_cases as cc  # noqa: E402


def main(first, count, npoints):
    t0 = time.time()
    tally = collections.Counter()
    bad = []
    for seed in range(first, first + count):
        case = cc.draw_case(seed)
        ref, err = cc.run_reference(case)
        with c_oracle.numpy_trig():
            res = cc.run_oracle(case)
        diff = cc.differences(case, res, ref, err)
        tally["key %d" % cc.launch_key(case)] += 1
        tally["err %s" % err] += 1
        tally["nw %d" % len(case["coords"]["s_w"])] += 1
        tally["particles"] += len(case["x"])
        tally["deleting runs"] += int(len(ref["x"]) < len(case["x"]))
        if diff:
            bad.append(seed)
            print(f"seed {seed}: {diff}", flush=True)
    print(f"trajectories: seeds {first} .. {first + count - 1}: {count - len(bad)} of {count} equal to the bit; different: {bad}")
    pbad = []
    for seed in range(npoints):
        case = cc.draw_points(seed)
        want, _ = cc.run_reference(case)
        got = cc.run_oracle(case)["sigma"]
        tally["points"] += len(got)
        if not cc.same_bits(got, want["sigma"]):
            pbad.append(seed)
            print(f"point seed {seed}: {int(np.sum(~((got == want['sigma']) | ((got != got) & (want['sigma'] != want['sigma'])))))} of {len(got)} differ", flush=True)
    print(f"points: seeds 0 .. {npoints - 1}: {npoints - len(pbad)} of {npoints} equal to the bit; different: {pbad}")
    for k in sorted(tally):
        print(f"  {k}: {tally[k]}")
    print(f"{time.time() - t0:.0f} s")


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 0)
