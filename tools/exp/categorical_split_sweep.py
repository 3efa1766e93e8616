"""Sweep of the lanes that share one sub-pixel's classes (S) in csrc/categorical.hip, on the MI355X.

usage: PG_VARIANT=ab python pytorch-generative_amd/build.py     # lib/libpg_hip_ab.so: the A/B switches are live
       python tools/exp/categorical_split_sweep.py [--out profiles/categorical_split_sweep.txt]

The planner keeps at least PG_CAT_CLASSES_PER_LANE classes per lane (64 in the production library, which does not read
the variable): S is the largest power of two with S * that <= K. One child process per setting (the switch is read
once), each timing the forward and the backward launch alone with tools/categorical_bench.py's method (one launch per
buffer set in a graph, sets rotated past the Infinity Cache, median of 3 rounds of 10 ms windows) at the bench's three
shapes and at one K = 1024 shape. One JSON line per setting: per shape the S the planner chose and the two times in us."""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
AB_LIB = os.path.join(ROOT, "pytorch-generative_amd", "pytorch_generative_amd", "lib", "libpg_hip_ab.so")
EXTRA_SHAPES = [(64, 1024, 1, 28, 28)]
SETTINGS = (1024, 512, 256, 128, 64, 32, 16, 8, 4)


def child():
    import torch

    import categorical_bench as cb

    dev = torch.device("cuda:0")
    out = {"classes_per_lane": int(os.environ["PG_CAT_CLASSES_PER_LANE"])}
    for shape in cb.SHAPES + EXTRA_SHAPES:
        row = cb.loss_row(shape, dev, 3, 10.0)
        out["x".join(map(str, shape))] = {"S": row["plan"]["lanes_per_pixel"], "fwd_us": round(row["fwd"]["ms"] * 1e3, 1),
                                          "bwd_us": round(row["bwd"]["ms"] * 1e3, 1)}
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "categorical_split_sweep.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child()
        return
    assert os.path.exists(AB_LIB), f"{AB_LIB} missing: PG_VARIANT=ab python pytorch-generative_amd/build.py"
    lines = ["# tools/exp/categorical_split_sweep.py on one MI355X: classes kept per lane -> S per shape N x K x C x H x W, "
             "forward / backward launch in us (buffer sets rotated past the Infinity Cache)"]
    for per_lane in SETTINGS:
        env = dict(os.environ, PG_HIP_LIB=AB_LIB, PG_CAT_CLASSES_PER_LANE=str(per_lane))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                           timeout=180)
        got = [line[7:] for line in r.stdout.splitlines() if line.startswith("RESULT ")]
        if r.returncode != 0 or not got:  # nothing more on the GPU after a failure
            sys.exit(f"classes per lane {per_lane}: exit {r.returncode}: {r.stderr[-400:]}")
        print(got[0], flush=True)
        lines.append(got[0])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
