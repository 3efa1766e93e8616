"""Generates tests/golden/conv_b3_routes.json: what the bf16x3 convolution launched BEFORE its host side was rewritten around one
route function (csrc/conv_b3.hip: b3_route) — recorded from commit 5403a78, the last one whose `pg_b3_conv` decided kernel, grid and
LDS layout inline.

That commit has no `pg_conv_b3_route`, so the record comes from a build of it with a capture hook in `pg_b3_conv`: an extra export
`pg_b3_capture(int* buf)`; while a buffer is set, every dispatch site copies the `B3Launch` and the geometry fields of `B3Args` into it
in the order of `_conv_b3_routes.FIELDS` (plus one trailing int, the W9 flag that commit still had) and returns 0 instead of launching;
and `pg_b3_plan_w9(Kc, M, T)` = 0 / 1 / 2 for no plan / a plan / a W9 plan of its format planner. The hook is thirty lines and is not part of the tree; run this script with the package of that commit on the path:

    PG_HIP_LIB=<capture build of 5403a78> PYTHONPATH=<checkout of 5403a78>/pytorch-generative_amd:<its root> \
        python tests/golden/make_conv_b3_routes_golden.py

The file holds (1) a readable table: every bf16x3-routed convolution of the eight bench workloads (see
`_conv_b3_routes.bench_problems`; one entry per convolution and orientation with the route of its plain launch at batch 1, and under
`then` what every other form / batch changes in it: `_conv_b3_routes.pack_table`), and (2) the SHA-256 of the canonical dump over the random problems of
test_routing_never_promises_a_shape_the_launch_refuses (`_conv_b3_routes.sweep_digest`). The W9 flag was 0 in every captured launch
and is not part of either; `w9_plans` records the CPU enumeration of the format planner that confirms no plan could set it.
"""

import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _conv_b3_routes as R  # noqa: E402

COMMIT = "5403a78"


def main():
    from pytorch_generative_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_int * (len(R.FIELDS) + 1))()
    lib.pg_b3_capture.restype = None
    lib.pg_b3_capture.argtypes = [ctypes.POINTER(ctypes.c_int)]
    lib.pg_b3_capture(buf)
    keep = np.zeros(1 << 12, dtype=np.float32)  # fake operands: never dereferenced, the hook returns before the launch
    p = ctypes.c_void_p((keep.ctypes.data + 255) // 256 * 256)
    p2 = ctypes.c_void_p(p.value + 256)
    w9_seen = []

    def capture(_lib_unused, pr):
        ia = ctypes.c_int * len(pr["dr"])
        dr, dc, t = ia(*pr["dr"]), ia(*pr["dc"]), len(pr["dr"])
        shape = (pr["n"], pr["kc"], pr["ih"], pr["iw"], pr["m"], pr["oh"], pr["ow"], t, dr, dc)
        for i in range(len(buf)):
            buf[i] = -12345
        if pr["form"] == "gate":
            rc = lib.pg_conv2d_mfma_gate(p, p, None, None, p, *shape, pr["in_act"], pr["gate"] - 1, None, p, None)
        elif pr["form"] == "dual":
            rc = lib.pg_conv2d_mfma_dual(p, p, p, p, pr["n"], pr["kc"], pr["oh"], pr["ow"], pr["m"], p, pr["dact"], p, None)
        else:
            res = p if pr["flags"] & R.RES else None
            res2 = None if not pr["flags"] & R.RES2 else (p if pr["flags"] & R.RES2_SAME else p2)
            rc = lib.pg_conv2d_mfma_ex(p, p, None, res, p, *shape, pr["in_act"], None, 0, pr["out_act"], 2, res2, 0, 0, None)
        if rc == 0:
            w9_seen.append(buf[len(R.FIELDS)])
        return rc, list(buf)[:len(R.FIELDS)]

    rows = []
    for label, pr in R.bench_problems(lib):
        rc, r = capture(lib, pr)
        assert rc == 0, (label, rc, lib.pg_last_error())
        rows.append((label, pr, r))
    table = R.pack_table(rows)
    assert [(a, c) for a, _, c in R.unpack_table(table)] == [(a, c) for a, _, c in rows]
    digest, routed = R.sweep_digest(lib, capture)
    assert not any(w9_seen), "a captured launch used the W9 instantiation"
    # the format planner over Kc (multiples of 8, 16..1024) x M (16..1024) x T (1..64): 0 = no plan, 1 = a plan, 2 = a W9 plan
    lib.pg_b3_plan_w9.restype = ctypes.c_int
    w9 = [(kc, m, t) for kc in range(16, 1025, 8) for m in range(16, 1025) for t in range(1, 65) if lib.pg_b3_plan_w9(kc, m, t) == 2]
    out = {"commit": COMMIT, "fields": R.FIELDS, "kernels": R.KERNELS, "table": table,
           "sweep": {"sha256": digest, "bf16x3_problems": routed, "seeds": 4}, "w9_plans": w9}
    path = os.path.join(HERE, "conv_b3_routes.json")
    with open(path, "w") as f:
        f.write("{\n")
        for k in ("commit", "fields", "kernels", "sweep", "w9_plans"):
            f.write(f" {json.dumps(k)}: {json.dumps(out[k])},\n")
        f.write(' "table": [\n' + ",\n".join("  " + json.dumps(row, separators=(",", ":")) for row in table) + "\n ]\n}\n")
    print(f"wrote {path}: {len(table)} table rows, {routed} swept bf16x3 problems, sha256 {digest}, {len(w9)} W9 plans, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
