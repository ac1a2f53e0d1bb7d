"""VALU instructions per wavefront-step of the rollout kernels, from a rocprofv3 PMC run of tools/rollout_grad_bench.py:

    rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU --output-format csv -d OUT -- \\
        python tools/rollout_grad_bench.py --reps 1 --warmup 0 --no-chain
    python tools/rollout_grad_pmc.py OUT [--steps 64] [--out profiles/rollout_grad_pmc.json]

That run dispatches, per configuration (65 536 then 1 048 576 envs; substeps 1 then 10), rollout_states_kernel twice
(the tape, then the timed call) and rollout_vjp_kernel once, so the dispatches of a grid size map to the configurations
in order.  valu_per_wavefront_step = SQ_INSTS_VALU / SQ_WAVES / K (the convention of profiles/pmc_counts.json); the
forward figure is the mean of its two dispatches.  tools/rollout_grad_bench.py turns it into the issue bound."""
import argparse
import collections
import csv
import glob
import hashlib
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS, SUBSTEPS = (65536, 1048576), (1, 10)


def dispatches(out_dir):
    """[(dispatch id, kernel name, grid size, {counter: value})] in dispatch order"""
    rows = collections.defaultdict(dict)
    meta = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                d = int(r["Dispatch_Id"])
                rows[d][r["Counter_Name"]] = rows[d].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
                meta[d] = (r["Kernel_Name"], int(r["Grid_Size"]))
    return [(d, meta[d][0], meta[d][1], rows[d]) for d in sorted(rows)]


def kernel_source_sha16():
    """of the sources the two kernels are built from (this TU and its adjoint header)"""
    h = hashlib.sha256()
    for f in ("copterstep_rollout_grad.hip", "rollout_adjoint.h"):
        with open(os.path.join(ROOT, "gym_copter_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_grad_pmc.json"))
    args = ap.parse_args()
    per = collections.defaultdict(lambda: {"fwd": [], "bwd": []})
    seen = collections.Counter()
    for _, name, grid, c in dispatches(args.out_dir):
        kind = "fwd" if "rollout_states_kernel" in name else "bwd" if "rollout_vjp_kernel" in name else None
        if kind is None or grid not in ENVS:
            continue
        idx = seen[(grid, kind)] // (2 if kind == "fwd" else 1)
        seen[(grid, kind)] += 1
        key = "lander3d_%d_substeps%d" % (grid, SUBSTEPS[idx])
        per[key][kind].append(c["SQ_INSTS_VALU"] / c["SQ_WAVES"] / args.steps)
    counts = {k: {p: round(sum(v) / len(v), 1) for p, v in d.items() if v} for k, d in sorted(per.items())}
    doc = {"valu_per_wavefront_step": counts, "K": args.steps, "kernel_source_sha16": kernel_source_sha16(),
           "note": "rocprofv3 PMC: SQ_INSTS_VALU / SQ_WAVES / K per dispatch of rollout_states_kernel (fwd, mean of 2) "
                   "and rollout_vjp_kernel (bwd), Lander3D, float32 storage; tools/rollout_grad_pmc.py"}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(counts, indent=1))


if __name__ == "__main__":
    main()
