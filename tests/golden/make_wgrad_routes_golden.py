"""Generates tests/golden/wgrad_routes.json: the route `pg_conv2d_wgrad_route` (csrc/conv_wgrad.hip: wgrad_route) gives every
convolution of the eight bench workloads at every resolution its model runs it, at batch 1 and 64 (`_wgrad_cases.bench_routes`).
tests/test_wgrad_route_cpu.py compares the current routes with it: a change of kernel, grid, tile or LDS size of a bench layer shows
as a diff of this file. Run from the repository root with the library built:

    python tests/golden/make_wgrad_routes_golden.py
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-generative_amd"), os.path.dirname(HERE)]

import _wgrad_cases as W  # noqa: E402


def main():
    from pytorch_generative_amd import _lib

    rows = W.bench_routes(_lib.load())
    path = os.path.join(HERE, "wgrad_routes.json")
    with open(path, "w") as f:
        f.write('{\n "fields": ' + json.dumps(W.FIELDS) + ',\n "families": ' + json.dumps(list(W.FAMILIES)) + ',\n "routes": [\n')
        f.write(",\n".join("  " + json.dumps(row, separators=(",", ":")) for row in rows) + "\n ]\n}\n")
    print(f"wrote {path}: {len(rows)} routes, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
