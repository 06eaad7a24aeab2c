#!/usr/bin/env python3
"""Times of the sphere-model kernels with a point-cloud world (csrc/mp_cloud.h) on one GPU, beside the same points entered as M
sphere obstacles of the primitive table - what a user had to do before - and beside the launch without a cloud.

    python tools/cloud_bench.py [--B 131072] [--N 100] [--edges 65536] [--reps 3] [--robots xarm6,panda] [--sizes 64,497,4096,100000]
                                [--table-limit 4096] [--out FILE] [--parent-json FILE] [--pmc-dir DIR]
    python tools/cloud_bench.py --no-cloud-only --root PARENT_CHECKOUT --out FILE      (the same launches on another checkout)
    python tools/cloud_bench.py --merge-into RESULT [--parent-json FILE] [--pmc-dir DIR] --out FILE      (no launches)

Prints one JSON line and writes it to --out (profiles/r17_cloud_bench.json unless given).  Per robot (the case of
tests/collision_cases.py: from_urdf spheres of radius 0.06, 12 primitive obstacles, q uniform in the joint limits; the edges and
their sphere model - the same spheres, pairs chosen with pair_clearance - by the recipe of tests/collision_edge_cases.py; the cloud
or the table entries are laid over both), device arrays:
  no_cloud        mp_collision_f64 on B N rows without a cloud, distances only ("dist": the instance without gradients) and with all
                  eight outputs ("grad"); mp_collision_edges_f64 on --edges edges ("edges")
  cloud[M]        the same three launches with a cloud of M points: the surfaces of tests/cloud_cases.py (a table top, a post) at the
                  pitch that gives M points, 60 loose points, radius = pitch sqrt(3) / 2, d_max = 0.2; "cell": the default
                  d_max + radius, and a quarter of it from 4096 points on (recorded per entry)
  table[M]        the same points as M sphere obstacles appended to the primitive table (skipped above --table-limit)
Every time is the median of single launches timed one by one with HIP events after a warm-up launch; *_min_ms / *_max_ms /
*_launches give the spread of the launches of one process.  "crossover": the smallest M measured at which the cloud is faster than
the table, per launch kind.
  parent_no_cloud / no_cloud_agrees   with --parent-json (the output of a --no-cloud-only run whose --root is a built checkout of the
                  parent commit, same sizes, same device): the parent's three launches, and per launch whether this commit's median
                  lies within the parent's own min..max spread widened by the same width on either side
  counters        with --pmc-dir (the output directory of `rocprofv3 --pmc ... -- python tools/cloud_bench.py ...`, a run of its
                  own with no tracing): the counters summed over the dispatches of each kernel
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_hip = None  # the package of --root, imported by main()

D_MAX = 0.2


def cloud_of(M):
    """(points (M, 3), radius): the table top [0.25, 0.85] x [-0.5, 0.5] at z = 0.1 and the post at (0.5, 0.3), z = 0.1 .. 0.9, at the
    largest pitch that gives at least M - 60 points, thinned evenly to M - 60, and 60 loose points from default_rng(5)."""
    loose = min(60, M // 2)
    need = M - loose
    pitch = 0.04
    while True:
        nx, ny, nz = int(round(0.6 / pitch)) + 1, int(round(1.0 / pitch)) + 1, int(round(0.8 / pitch)) + 1
        if nx * ny + nz >= need:
            break
        pitch *= 0.97
    x, y = 0.25 + pitch * np.arange(nx), -0.5 + pitch * np.arange(ny)
    top = np.stack(np.meshgrid(x, y, [0.1], indexing="ij"), axis=-1).reshape(-1, 3)
    post = np.column_stack([np.full(nz, 0.5), np.full(nz, 0.3), 0.1 + pitch * np.arange(nz)])
    surf = np.concatenate([top, post])
    surf = surf[np.linspace(0, len(surf) - 1, need).round().astype(int)]
    rng = np.random.default_rng(5)
    pts = np.concatenate([surf, np.column_stack([rng.uniform(-0.9, 0.9, (loose, 2)), rng.uniform(0.0, 1.2, loose)])])
    return np.ascontiguousarray(pts), pitch * np.sqrt(3.0) / 2.0


def _time(ctx, fn, reps, window_ms=300.0, cap=20):
    a, b = _hip.HipEvent(ctx), _hip.HipEvent(ctx)

    def once():
        a.record()
        fn()
        b.record()
        ctx.synchronize()
        return b.elapsed_ms_since(a)

    first = once()  # the warm-up launch
    n = int(min(cap, max(reps, np.ceil(window_ms / max(first, 1e-3)))))
    t = np.array([once() for _ in range(n)])
    a.destroy(); b.destroy()
    return {"ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4), "launches": n}


def read_counters(folder):
    """{kernel: {counter: sum over its dispatches}} from the counter-collection CSVs below `folder`."""
    import csv
    import glob
    import re

    out = {}
    for path in glob.glob(os.path.join(folder, "**", "*counter_collection.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                kernel = row.get("Kernel_Name") or row.get("Kernel Name") or "?"
                m = re.search(r"k_\w+<[^>]*>", kernel)      # the instance, without its namespace and argument list
                kernel = m.group(0) if m else kernel.split("(")[0]
                name, value = row.get("Counter_Name") or row.get("Counter Name"), row.get("Counter_Value") or row.get("Counter Value")
                if name is None or value is None:
                    continue
                k = out.setdefault(kernel, {})
                k[name] = k.get(name, 0.0) + float(value)
                k["dispatch_rows"] = k.get("dispatch_rows", 0) + 1
    return out


def main():
    global _hip
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=131072)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--edges", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--robots", default="xarm6,panda")
    ap.add_argument("--sizes", default="64,497,4096,100000")
    ap.add_argument("--table-limit", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_cloud_bench.json"))
    ap.add_argument("--root", default=ROOT, help="the built checkout whose package and test cases are used")
    ap.add_argument("--no-cloud-only", action="store_true", help="only the launches without a cloud (works on the parent commit)")
    ap.add_argument("--parent-json", default="")
    ap.add_argument("--pmc-dir", default="")
    ap.add_argument("--merge-into", default="", help="no launches: add --parent-json / --pmc-dir to this earlier result and write --out")
    args = ap.parse_args()
    if args.merge_into:
        return finish(json.load(open(args.merge_into)), args)
    sys.path.insert(0, args.root)
    sys.path.insert(0, os.path.join(args.root, "tests"))
    import collision_cases as cc
    import collision_edge_cases as ec
    from manipulapy_amd import _hip as hip
    from manipulapy_amd.collision import SphereCollisionModel

    _hip = hip
    ctx = _hip.HipContext(0)
    rows = args.B * args.N
    sizes = [int(s) for s in args.sizes.split(",")]
    res = {"B": args.B, "N": args.N, "rows": rows, "edges": args.edges, "d_max": D_MAX,
           "device": (ctx.properties().get("name") or "unknown").strip("() "), "robots": {}}
    for name in args.robots.split(","):
        case = cc.make_case(name, rows=4096)
        base = case["cm"]
        cm = SphereCollisionModel(base.model, base.links, base.centres, base.radii, base.pairs)
        cm.set_world_table(base.kinds, base.params)
        n = cm.n
        q = np.random.default_rng(1).uniform(case["q"].min(axis=0), case["q"].max(axis=0), (rows, n))
        ebase, S_list, lim = ec.make_model(name)
        em = SphereCollisionModel(ebase.model, ebase.links, ebase.centres, ebase.radii, ebase.pairs)
        em.set_world_table(ebase.kinds, ebase.params)
        qa, qb = ec.draw_edges(em, S_list, lim, 7, 4096)
        pick = np.random.default_rng(2).integers(0, 4096, args.edges)
        qa, qb = np.ascontiguousarray(qa[pick]), np.ascontiguousarray(qb[pick])
        bufs = []

        def keep(b):
            bufs.append(b)
            return b

        d_q, d_qa, d_qb = keep(ctx.to_device(q)), keep(ctx.to_device(qa)), keep(ctx.to_device(qb))
        col, vec = rows * 8, rows * n * 8
        d = {"dist_world": keep(ctx.alloc(col)), "arg_world": keep(ctx.alloc(col)), "dist_self": keep(ctx.alloc(col)),
             "arg_self": keep(ctx.alloc(col)), "cost": keep(ctx.alloc(col)), "grad_dist_world": keep(ctx.alloc(vec)),
             "grad_dist_self": keep(ctx.alloc(vec)), "grad": keep(ctx.alloc(vec))}
        E = args.edges
        de = {"status": keep(ctx.alloc(E * 4)), "t": keep(ctx.alloc(E * 8)), "steps": keep(ctx.alloc(E * 4)),
              "clearance": keep(ctx.alloc(E * 8)), "witness": keep(ctx.alloc(E * 12))}
        lean = ("dist_world", "arg_world", "dist_self", "arg_self", "cost")

        def three():
            cm.sync_world(ctx)
            em.sync_world(ctx)
            run = lambda keys: ctx.collision(cm.model, cm.handle, d_q, rows, cc.EPS_WORLD, cc.EPS_SELF, **{"d_" + k: d[k] for k in keys})  # noqa: E731
            out = {"dist": _time(ctx, lambda: run(lean), args.reps), "grad": _time(ctx, lambda: run(tuple(d)), args.reps)}
            out["edges"] = _time(ctx, lambda: ctx.collision_edges(em.model, em.handle, d_qa, d_qb, E, ec.MARGIN, ec.TOL, ec.MAX_STEPS,
                                                                  **{"d_" + k: b for k, b in de.items()}), args.reps)
            steps = de["steps"].download((E,), np.int32)
            out["edge_evaluations"] = int(steps.sum())
            return out

        r = {"n": n, "spheres": int(len(cm.links)), "pairs": int(len(cm.pairs)), "obstacles": int(len(cm.kinds)), "no_cloud": three(),
             "cloud": {}, "table": {}}
        for M in ([] if args.no_cloud_only else sizes):
            pts, radius = cloud_of(M)
            cell = (D_MAX + radius) / 4 if M >= 4096 else D_MAX + radius
            cm.set_cloud(pts, radius, D_MAX, cell)
            em.set_cloud(pts, radius, D_MAX, cell)
            r["cloud"][str(M)] = dict(three(), radius=round(radius, 6), cell=round(cell, 6), dims=cm.handle.cloud_info()["dims"])
            cm.clear_cloud()
            em.clear_cloud()
            if M <= args.table_limit:
                cm.set_world_table(np.concatenate([base.kinds, np.zeros(M, dtype=np.int32)]),
                                   np.concatenate([base.params, np.column_stack([pts, np.full(M, radius), np.zeros((M, 12))])]))
                em.set_world_table(np.concatenate([ebase.kinds, np.zeros(M, dtype=np.int32)]),
                                   np.concatenate([ebase.params, np.column_stack([pts, np.full(M, radius), np.zeros((M, 12))])]))
                r["table"][str(M)] = three()
                cm.set_world_table(base.kinds, base.params)
                em.set_world_table(ebase.kinds, ebase.params)
        r["crossover"] = {k: next((M for M in sizes if str(M) in r["table"] and r["cloud"][str(M)][k]["ms"] < r["table"][str(M)][k]["ms"]), None)
                          for k in ("dist", "grad", "edges")}
        res["robots"][name] = r
        for b in bufs:
            b.free()
    finish(res, args)


def finish(res, args):
    if args.parent_json:
        par = json.load(open(args.parent_json))
        res["parent_sizes"] = {k: par[k] for k in ("B", "N", "rows", "edges", "device")}
        for name, r in res["robots"].items():
            pn = par["robots"][name]["no_cloud"]
            r["parent_no_cloud"] = pn
            r["no_cloud_agrees"] = {}
            for k in ("dist", "grad", "edges"):
                width = pn[k]["max_ms"] - pn[k]["min_ms"]
                r["no_cloud_agrees"][k] = bool(pn[k]["min_ms"] - width <= r["no_cloud"][k]["ms"] <= pn[k]["max_ms"] + width)
    if args.pmc_dir:
        res["counters"] = read_counters(args.pmc_dir) or None
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
