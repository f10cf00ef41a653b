#!/usr/bin/env python3
"""16-bit float pixels against f32 on the fused path: step time and per-kernel times, alternating in ONE process.

    python tools/probes/half_probe.py [--shape 16384 16384] [--order 2] [--steps 50] [--warmup 10] [--rounds 5] [--staged] [--kinds f32,f16,bf16]
    python tools/probes/half_probe.py --volume 512 1024 512 [--staged] [--steps 10] ...

For the Gaussian of the given order (+x -x +y -y, clamped; cfg3 is order 2 at 16384^2) it builds an f32, an f16 and a bf16 plan
(--staged: also the f16 plan staged through f32 planes, RF_PLAN_STAGE_HALF), warms every plan up, then runs `rounds` rounds;
each round times every plan in turn -- `steps` executes between two HIP events -- and takes one execute_timed() per plan
for the per-kernel times.  Printed: per plan the median / min / max ms per step over the rounds, the median per-kernel
times, and the ratios t16 / t32 for the step and per kernel.  A library other than the built one (e.g. one compiled with
-DRF_HALF_PACKED_STORES for the store-form A/B) is selected with RECFILTER_AMD_LIB, one process per library.

--volume DEPTH ROWS WIDTH: the same Gaussian along x, y and z of a volume.  The plans: "f32" with two first passes
(RF_PLAN_STAGED_PASS1: launch for launch what the native 16-bit volume runs), "f32_walk" (the f32 plan's default, the one-read
pass 1 where it applies), the native f16 / bf16 volumes, and with --staged the f16 volume staged through f32 planes
(RF_PLAN_STAGE_HALF).  The ratios are taken against "f32"; the last lines give native / staged and native / f32_walk."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import recfilter_amd as rfa
from recfilter_amd import capi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, default=[16384, 16384], metavar=("ROWS", "WIDTH"))
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--staged", action="store_true")
    ap.add_argument("--kinds", default="f32,f16,bf16", help="comma-separated subset of f32,f16,bf16 (a profiler run takes one)")
    ap.add_argument("--volume", type=int, nargs=3, default=None, metavar=("DEPTH", "ROWS", "WIDTH"), help="a volume, filtered along z too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("half_probe: needs a GPU")
    shape = tuple(a.volume) if a.volume else tuple(a.shape)
    w = rfa.gaussian_weights(5.0, a.order)
    scans = [(0, True, w), (0, False, w), (1, True, w), (1, False, w)]
    if a.volume:
        scans += [(2, True, w), (2, False, w)]
    if a.volume:        # (up to 2^30 samples: drawn on the device; the 2-D mode keeps its host generator and its data)
        base = torch.rand(shape, dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    else:
        base = torch.from_numpy(np.random.default_rng(9).random(shape, dtype=np.float32)).cuda()
    f32_flags = capi.RF_PLAN_STAGED_PASS1 if a.volume else 0
    kinds = [k for k in (("f32", torch.float32, f32_flags), ("f16", torch.float16, 0), ("bf16", torch.bfloat16, 0)) if k[0] in a.kinds.split(",")]
    if a.volume and "f32" in a.kinds.split(","):
        kinds.insert(1, ("f32_walk", torch.float32, 0))
    if a.staged:
        kinds.append(("f16_staged", torch.float16, capi.RF_PLAN_STAGE_HALF))
    plans = {}
    for name, tdt, flags in kinds:
        x = base.to(tdt)
        staged = bool(flags & capi.RF_PLAN_STAGE_HALF)
        plans[name] = (rfa.Plan(shape, scans, dtype=tdt, clamped=True, path=capi.RF_PATH_AUTO if staged else capi.RF_PATH_TILED_FUSED,
                                flags=flags), x, torch.empty_like(x))
    print(f"half_probe: shape {shape} order {a.order} steps {a.steps} warmup {a.warmup} rounds {a.rounds} lib {os.environ.get('RECFILTER_AMD_LIB', '(built)')}")
    for name, (plan, x, out) in plans.items():
        for _ in range(a.warmup):
            plan.execute([x], [out])
        _, timed = plan.execute_timed([x], [out])
        print(f"  {name:10s} path {plan.path_name} tiles {plan.tiles} launches {[n for n, _ in timed]} workspace {plan.workspace_bytes / 2**20:.1f} MiB")
    torch.cuda.synchronize()
    step = {n: [] for n in plans}
    kern = {n: {} for n in plans}
    for _ in range(a.rounds):
        for name, (plan, x, out) in plans.items():
            plan.execute([x], [out])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                plan.execute([x], [out])
            e1.record()
            e1.synchronize()
            step[name].append(e0.elapsed_time(e1) / a.steps)
            _, timed = plan.execute_timed([x], [out])
            for i, (k, ms) in enumerate(timed):
                kern[name].setdefault((i, k), []).append(ms)
    med = {n: statistics.median(v) for n, v in step.items()}
    for name in plans:
        ks = " ".join(f"{k}={statistics.median(v) * 1e3:.1f}us" for (_, k), v in sorted(kern[name].items()))
        print(f"  {name:10s} ms_per_step median {med[name]:.4f} min {min(step[name]):.4f} max {max(step[name]):.4f} | {ks}")
    for name in plans:
        if name == "f32" or "f32" not in plans:
            continue
        line = f"  {name:10s} / f32: step {med[name] / med['f32']:.3f}"
        for (i, k), v in sorted(kern[name].items()):
            ref = kern["f32"].get((i, k))
            if ref:
                line += f" {k} {statistics.median(v) / statistics.median(ref):.3f}"
        print(line)
    for name in ("f16", "bf16"):
        if name in plans and "f16_staged" in plans:
            print(f"  {name:10s} / f16_staged: step {med[name] / med['f16_staged']:.3f}")
        if name in plans and "f32_walk" in plans:
            print(f"  {name:10s} / f32_walk: step {med[name] / med['f32_walk']:.3f}")
    for plan, _, _ in plans.values():
        plan.close()


if __name__ == "__main__":
    main()
