"""The problems and the canonical dump behind tests/golden/conv_b3_routes.json (shared by tests/test_conv_b3_route_cpu.py, the
per-family GPU test and tests/golden/make_conv_b3_routes_golden.py).

A problem is a dict of the integers `pg_conv_b3_route` takes (csrc/conv_b3.hip: b3_route): batch, K channels / input size, M channels /
output size, tap offsets, activation ids, gate id and the PG_B3R_* flag mask. A route is the list of ints the export fills, named by
FIELDS: which kernel instantiation takes the launch, its grid / block / LDS bytes, and every geometry field of the kernel's arguments.
"""

import hashlib
import json
import random

# include/pg_hip.h: PG_B3R_*
RES, RES2, RES2_SAME, RES_STRIDED, DACT_SRC, DUAL, IN_MISALIGNED = 1, 2, 4, 8, 16, 32, 64
KERNELS = {0: "staged", 1: "1x1", 2: "pipelined", 3: "overlapped"}
MAXG = 20
FIELDS = (["kernel", "gelu", "MT", "NT", "CG", "MS", "GT", "waves", "xslots_per_thread", "two_tiles", "grid_x", "grid_y", "block",
           "lds_bytes", "TR", "tile_h", "tile_w", "plane16", "tiles_per_img", "CIB", "cgs", "groups", "ksteps", "wslab4", "xslots",
           "dump16", "w_off16", "ep_off", "b_off", "res_scale", "res2_folded", "min_dr", "min_dc"]
          + [f"g_tapoff{g}" for g in range(MAXG)] + [f"g_cg{g}" for g in range(MAXG)])
ACT_ELU = 2
FORMS = {  # epilogue form -> (flags, gate id + 1, dact)
    "plain": (0, 0, 0),
    "two_residuals": (RES | RES2, 0, 0),
    "same_residual_twice": (RES | RES2 | RES2_SAME, 0, 0),
    "gate": (0, 1, 0),
    "dual": (RES | DACT_SRC | DUAL, 0, ACT_ELU),
}


# One small convolution per kernel family, batch 2: (what, case of tests/test_gpu_ops.py's CONV_CASES layout — N, Cin, H, W, Cout, kh,
# kw, ph, pw, crop, active taps, in_act, residual, bias —, route fields the FORWARD launch must show). The data gradient of the last
# row (320 -> 16) lands on the narrow staged kernel. (These eight run the plain epilogue through the Python layer against an fp32 oracle:
# tests/test_gpu_ops.py::test_conv_b3_kernel_families. The table of every instantiation and epilogue form, compared with float64 through
# the C ABI, is tests/_conv_cases.py / tests/test_gpu_conv_families.py.)
FAMILY_CASES = [
    ("staged narrow, two output tiles", (2, 32, 8, 8, 32, 3, 3, 1, 1, None, None, None, False, True), {"kernel": 0, "MT": 2, "CG": 1}),
    ("staged narrow, four output tiles", (2, 64, 8, 8, 64, 3, 3, 1, 1, None, None, None, False, True), {"kernel": 0, "MT": 4, "CG": 1}),
    ("staged wide", (2, 64, 8, 8, 128, 3, 3, 1, 1, None, None, None, False, True), {"kernel": 0, "CG": 2}),
    ("1x1, one output tile", (2, 16, 8, 8, 16, 1, 1, 0, 0, None, None, None, False, True), {"kernel": 1, "MT": 1}),
    ("1x1, four output tiles", (2, 64, 8, 8, 64, 1, 1, 0, 0, None, None, None, False, True), {"kernel": 1, "MT": 4}),
    ("pipelined, one pixel group per wave", (2, 64, 8, 8, 64, 2, 2, 1, 1, "hw", None, None, False, True),
     {"kernel": 2, "waves": 8, "NT": 1}),
    ("pipelined, two pixel groups per wave", (2, 64, 16, 16, 64, 2, 2, 1, 1, "hw", None, None, False, True),
     {"kernel": 2, "waves": 8, "NT": 2}),
    ("overlapped, two tiles per workgroup", (2, 16, 16, 32, 320, 2, 3, 1, 1, "hw", None, None, False, True),
     {"kernel": 3, "two_tiles": 1}),
]


def family_problem(case):
    """The forward problem of a FAMILY_CASES / CONV_CASES tuple (all taps active)."""
    n, cin, h, w, cout, kh, kw, ph, pw, crop = case[:10]
    oh, ow = (h, w) if crop == "hw" else (h + 2 * ph - kh + 1, w + 2 * pw - kw + 1)
    taps = [(u, v) for u in range(kh) for v in range(kw)]
    return problem(n, cin, h, w, cout, oh, ow, [u - ph for u, _ in taps], [v - pw for _, v in taps])


def problem(n, kc, ih, iw, m, oh, ow, dr, dc, form="plain", in_act=0, out_act=0):
    flags, gate, dact = FORMS[form]
    return {"n": n, "kc": kc, "ih": ih, "iw": iw, "m": m, "oh": oh, "ow": ow, "dr": list(dr), "dc": list(dc), "in_act": in_act,
            "dact": dact, "out_act": out_act, "gate": gate, "flags": flags, "form": form}


def route(lib, pr):
    """(status, route as a list of len(FIELDS) ints) from pg_conv_b3_route."""
    import ctypes

    out = (ctypes.c_int * len(FIELDS))()
    ia = ctypes.c_int * len(pr["dr"])
    rc = lib.pg_conv_b3_route(pr["n"], pr["kc"], pr["ih"], pr["iw"], pr["m"], pr["oh"], pr["ow"], len(pr["dr"]), ia(*pr["dr"]),
                              ia(*pr["dc"]), pr["in_act"], pr["dact"], pr["out_act"], pr["gate"], pr["flags"], out, len(FIELDS))
    return rc, list(out)


def named(r):
    return dict(zip(FIELDS, r))


def fmt_of(lib, pr):
    hr, hc = max(pr["dr"]) - min(pr["dr"]), max(pr["dc"]) - min(pr["dc"])
    return lib.pg_conv_mfma_supported(pr["kc"], pr["m"], len(pr["dr"]), pr["oh"], pr["ow"], pr["iw"], hr, hc)


def dual_ok(lib, pr):
    return lib.pg_conv_dual_ok(pr["kc"], pr["m"], pr["oh"], pr["ow"])


def gate_fusable(lib, pr):
    import ctypes

    ia = ctypes.c_int * len(pr["dr"])
    return lib.pg_conv_gate_fusable(pr["kc"], pr["m"], pr["oh"], pr["ow"], len(pr["dr"]), ia(*pr["dr"]), ia(*pr["dc"]))


def bench_problems(lib):
    """Every bf16x3-routed convolution of the eight bench workloads at every resolution its model runs it (collected like
    test_weight_gradient_planner_takes_every_layer_of_the_bench_workloads), forward and data gradient, batch 1 and 64: the plain
    epilogue everywhere, and the two-residual / gate / dual forms wherever the Python layer's own predicates allow them
    (ops.conv_two_residuals_ok: >= 64 output channels; ops.conv_gate_ok: pg_conv_gate_fusable; ops.conv_dual_ok: the data gradient
    of a 1x1 convolution with pg_conv_dual_ok). Returns [(label, problem)]."""
    import bench
    import pytorch_generative_amd as pg

    rows, seen = [], set()
    for name, w in bench.WORKLOADS.items():
        model = getattr(pg.models, w["ctor"])(**w["kw"])
        side = w["chw"][1]
        sides = [side] if name in ("image_gpt", "image_gpt_repro", "pixel_snail", "gated_pixel_cnn", "pixel_cnn") else \
            [s for s in (64, 32, 16, 8, 4, 2, 1) if s <= side]
        for label, mod in model.named_modules():
            if not hasattr(mod, "_conv_spec") or getattr(mod, "weight", None) is None or mod.weight.dim() != 4:
                continue
            sp = mod._conv_spec()
            cout, cin = (int(v) for v in mod.weight.shape[:2])
            f_dr, f_dc, f_ndr, f_ndc = list(sp.f_dr), list(sp.f_dc), list(sp.f_ndr), list(sp.f_ndc)
            for s in sides:
                oh, ow = sp.full_out(s, s)
                oh, ow = min(oh, s), min(ow, s)  # the causal layers crop their output back to the input size
                if oh < 1 or ow < 1:
                    continue
                for orient, geo in (("fwd", (cin, s, s, cout, oh, ow, f_dr, f_dc)), ("dgrad", (cout, oh, ow, cin, s, s, f_ndr, f_ndc))):
                    key = (orient,) + geo[:6] + (tuple(geo[6]), tuple(geo[7]))
                    if key in seen:
                        continue
                    seen.add(key)
                    plain = problem(1, *geo)
                    if fmt_of(lib, plain) != 2:
                        continue
                    forms = ["plain"]
                    if geo[3] >= 64:
                        forms += ["two_residuals", "same_residual_twice"]
                    if orient == "fwd" and gate_fusable(lib, plain):
                        forms.append("gate")
                    if orient == "dgrad" and (sp.kh, sp.kw) == (1, 1) and f_dr == [0] and f_dc == [0] and dual_ok(lib, plain):
                        forms.append("dual")
                    for form in forms:
                        for n in (1, 64):
                            rows.append((f"{name} {label} {s}x{s} {orient} {form} N={n}", problem(n, *geo, form=form)))
    return rows


GEOMETRY = ("kc", "ih", "iw", "m", "oh", "ow", "dr", "dc")


def pack_table(rows):
    """[(label, problem, route)] in the order of bench_problems -> one entry per convolution and orientation: its geometry, the route
    of the plain launch at batch 1 (trailing zeros dropped), and under `then` what each further form / batch changes in it."""
    groups = []
    for label, pr, r in rows:
        what, form, n = label.rsplit(" ", 2)
        if not groups or groups[-1]["what"] != what:
            assert (form, n) == ("plain", "N=1"), label
            base = list(r)
            keep = max((i + 1 for i, v in enumerate(base) if v), default=0)
            groups.append({"what": what, "problem": [pr[k] for k in GEOMETRY], "route": base[:keep], "then": {}})
        else:
            groups[-1]["then"][f"{form} {n}"] = {FIELDS[i]: v for i, (v, b) in enumerate(zip(r, base)) if v != b}
    return groups


def unpack_table(groups):
    """The inverse: [(label, geometry, route)]."""
    out = []
    for g in groups:
        base = g["route"] + [0] * (len(FIELDS) - len(g["route"]))
        out.append((g["what"] + " plain N=1", g["problem"], base))
        for key, diff in g["then"].items():
            r = list(base)
            for k, v in diff.items():
                r[FIELDS.index(k)] = v
            out.append((f"{g['what']} {key}", g["problem"], r))
    return out


def random_problems(seed):
    """The problems of test_routing_never_promises_a_shape_the_launch_refuses (tests/test_host_cpu.py), same generator, same order:
    forward then data gradient of each drawn convolution."""
    r = random.Random(seed)
    kernels = [(1, 1), (2, 2), (3, 3), (2, 3), (1, 3), (3, 1), (2, 1), (1, 2), (5, 5), (4, 4), (7, 7), (3, 5)]
    out = []
    for _ in range(1500):
        kh, kw = r.choice(kernels)
        ph, pw = r.choice([(0, 0), (kh // 2, kw // 2), (kh - 1, kw - 1), (kh - 1, kw // 2)])
        taps = [(u, v) for u in range(kh) for v in range(kw)]
        mode = r.choice(["all", "A", "B", "random"])
        if mode == "A":
            taps = [(u, v) for u, v in taps if u < kh // 2 or (u == kh // 2 and v < kw // 2)] or taps
        elif mode == "B":
            taps = [(u, v) for u, v in taps if u < kh // 2 or (u == kh // 2 and v <= kw // 2)]
        elif mode == "random":
            taps = [t for t in taps if r.random() < 0.6] or taps
        cin = r.choice([1, 2, 3, 4, 5, 7, 8, 12, 16, 24, 32, 33, 40, 48, 64, 66, 69, 96, 100, 128, 160, 192, 256, 320, 512])
        cout = r.choice([1, 2, 3, 8, 10, 16, 24, 32, 36, 40, 56, 64, 72, 96, 100, 128, 160, 192, 256, 320, 512])
        ih = r.choice([1, 2, 3, 4, 5, 7, 8, 12, 14, 16, 20, 28, 32, 33, 48, 64, 100, 128])
        iw = r.choice([1, 2, 3, 4, 6, 8, 12, 14, 16, 20, 28, 32, 36, 48, 64, 100, 128, 256, 300])
        n = r.choice([1, 2, 3, 7, 16, 33])
        oh, ow = ih + 2 * ph - kh + 1, iw + 2 * pw - kw + 1
        if oh < 1 or ow < 1:
            continue
        out.append(problem(n, cin, ih, iw, cout, oh, ow, [u - ph for u, _ in taps], [v - pw for _, v in taps]))
        out.append(problem(n, cout, oh, ow, cin, ih, iw, [ph - u for u, _ in taps], [pw - v for _, v in taps]))
    return out


def sweep_digest(lib, route_fn):
    """SHA-256 over one line per random problem (four seeds, both orientations): the three routing queries, and for every problem the
    format query sends to bf16x3 the status and the full route of `route_fn(lib, problem)`. Returns (digest, bf16x3 problems)."""
    h = hashlib.sha256()
    routed = 0
    for seed in range(4):
        for i, pr in enumerate(random_problems(seed)):
            fmt = fmt_of(lib, pr)
            line = [seed, i, fmt, dual_ok(lib, pr), gate_fusable(lib, pr)]
            if fmt == 2:
                rc, r = route_fn(lib, pr)
                line += [rc, r if rc == 0 else []]
                routed += 1
            h.update((json.dumps(line, separators=(",", ":")) + "\n").encode())
    return h.hexdigest(), routed
