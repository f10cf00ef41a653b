#!/usr/bin/env python3
"""Byte images end to end (rf_input_dtype RF_IO_U8) against the route a caller had before: step time and per-kernel times,
alternating in ONE process.

    python tools/probes/u8_probe.py [--shape 16384 16384] [--order 2] [--steps 50] [--warmup 10] [--rounds 7] [--packed-lib PATH]

For the Gaussian of the given order (+x -x +y -y, clamped; cfg3 is order 2 at 16384^2) on random bytes, with the usual round
trip x' = in / 255, out = 255 F, it builds
    staged    the RF_IN_U8 f32 plan followed by one sat8 conversion: the staged form (RF_PLAN_STAGE_HALF) -- what a caller
              ran before byte output planes existed, with the library's kernel in the place of the caller's
    staged_2  the same plan again: the spread of `staged` against a copy of itself in the same run
    in_u8     the RF_IN_U8 plan alone, f32 output (no conversion): what the final pass costs with 4-byte stores
    native    byte output planes natively: the final pass stores the bytes
warms every plan up, then runs `rounds` rounds; each round times every plan in turn -- `steps` executes between two HIP
events -- and takes one execute_timed() per plan for the per-kernel times.  Printed: per plan the median / min / max ms per
step over the rounds and the median per-kernel times; then native / staged, staged_2 / staged and the verdict: native is ahead
when its median is below staged's by more than |staged_2 - staged|.

The store form of the native final pass is a compile-time choice (scan_device.h, RF_U8_PACKED_STORES).  --packed-lib PATH names
a library built with -DRF_U8_PACKED_STORES: the probe then starts itself once more as a fresh child process with
RECFILTER_AMD_LIB=PATH after its own run, and the two outputs are the A/B of the two store forms on the same box."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def run(a):
    import numpy as np
    import torch
    import recfilter_amd as rfa
    from recfilter_amd import capi
    if not torch.cuda.is_available():
        sys.exit("u8_probe: needs a GPU")
    shape = tuple(a.shape)
    w = rfa.gaussian_weights(5.0, a.order)
    scans = [(0, True, w), (0, False, w), (1, True, w), (1, False, w)]
    x = torch.from_numpy(np.random.default_rng(9).integers(0, 256, size=shape).astype(np.uint8)).cuda()
    pw = dict(prologue=(1.0 / 255.0, 0.0), epilogue=(255.0, 0.0, 0.0))
    io = dict(dtype=np.float32, input_dtype=np.uint8, output_dtype=np.uint8, clamped=True, **pw)
    specs = [("staged", dict(io, path=capi.RF_PATH_AUTO, flags=capi.RF_PLAN_STAGE_HALF), torch.uint8),
             ("staged_2", dict(io, path=capi.RF_PATH_AUTO, flags=capi.RF_PLAN_STAGE_HALF), torch.uint8),
             ("in_u8", dict(dtype=np.float32, input_dtype=np.uint8, clamped=True, path=capi.RF_PATH_TILED_FUSED, flags=0, **pw), torch.float32),
             ("native", dict(io, path=capi.RF_PATH_TILED_FUSED, flags=0), torch.uint8)]
    plans = {name: (rfa.Plan(shape, scans, **kw), torch.empty(shape, dtype=tdt, device="cuda")) for name, kw, tdt in specs}
    print(f"u8_probe: shape {shape} order {a.order} steps {a.steps} warmup {a.warmup} rounds {a.rounds} lib {os.environ.get('RECFILTER_AMD_LIB', '(built)')}")
    for name, (plan, out) in plans.items():
        for _ in range(a.warmup):
            plan.execute([x], [out])
        _, timed = plan.execute_timed([x], [out])
        print(f"  {name:9s} path {plan.path_name} tiles {plan.tiles} launches {[n for n, _ in timed]} workspace {plan.workspace_bytes / 2**20:.1f} MiB")
    torch.cuda.synchronize()
    same = torch.equal(plans["native"][1], plans["staged"][1])
    diff = (plans["native"][1].to(torch.int16) - plans["staged"][1].to(torch.int16)).abs()
    print(f"  native against staged: identical {same}, max byte difference {int(diff.max())}, differing samples {int((diff != 0).sum())}")
    step = {n: [] for n in plans}
    kern = {n: {} for n in plans}
    for _ in range(a.rounds):
        for name, (plan, out) in plans.items():
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
        print(f"  {name:9s} ms_per_step median {med[name]:.4f} min {min(step[name]):.4f} max {max(step[name]):.4f} | {ks}")
    spread = abs(med["staged_2"] - med["staged"])
    gain = med["staged"] - med["native"]
    print(f"  native / staged: step {med['native'] / med['staged']:.3f}   staged_2 / staged: {med['staged_2'] / med['staged']:.3f}   "
          f"native / in_u8: {med['native'] / med['in_u8']:.3f}")
    print(f"  verdict: staged - native = {gain * 1e3:.1f} us, spread of staged against its copy {spread * 1e3:.1f} us: "
          f"native is {'AHEAD' if gain > spread else 'NOT ahead'}")
    for plan, _ in plans.values():
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, default=[16384, 16384], metavar=("ROWS", "WIDTH"))
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--packed-lib", default=None, help="a library built with -DRF_U8_PACKED_STORES: run again on it, in a fresh child process")
    a = ap.parse_args()
    if a.packed_lib is None:
        return run(a)
    # (one process per library: the library is chosen when recfilter_amd loads it.  This parent opens no GPU itself.)
    args = [sys.executable, os.path.abspath(__file__), "--shape", str(a.shape[0]), str(a.shape[1]), "--order", str(a.order),
            "--steps", str(a.steps), "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
    for lib in (None, os.path.abspath(a.packed_lib), None, os.path.abspath(a.packed_lib)):       # alternating: plain, packed, plain, packed
        env = dict(os.environ)
        env.pop("RECFILTER_AMD_LIB", None)
        if lib:
            env["RECFILTER_AMD_LIB"] = lib
        print(f"---- {'packed stores: ' + lib if lib else 'plain stores (the built library)'}", flush=True)
        rc = subprocess.run(args, env=env, timeout=900).returncode
        if rc != 0:
            sys.exit(rc)      # (a failed run ends the probe: nothing more is started on the GPU)


if __name__ == "__main__":
    main()
