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
RECFILTER_AMD_LIB=PATH after its own run, and the two outputs are the A/B of the two store forms on the same box.

    python tools/probes/u8_probe.py --volume [--sizes 128,128,128 128,256,256 ...] [--order 2] [--rounds 7] [--packed-lib PATH]

Byte VOLUMES: the Gaussian along +x -x +y -y +z -z, clamped, with the same round trip.  Per size (default 128^3, 128 x 256 x 256,
256^3, 512^3, 1024^3; z y x), one after the other in one process, it builds
    native    the native byte plan (RF_PATH_TILED_FUSED): the x/y result waits in an f32 volume, the final z pass stores bytes
    staged    the staged byte plan (RF_PLAN_STAGE_HALF): the RF_IN_U8 plan into an f32 volume, then one sat8 conversion
    staged_2  the same plan again: the noise floor
    f32       the f32 plan of the same filter on f32 volumes (RF_PATH_AUTO)
and alternates them as above (the steps per timing scale with the size).  Printed per size: the table above, the per-kernel
times of the native plan, native / staged beside the byte model's 15 / 23 = 0.652, and the verdict.  The parity check of a run
is native against staged: at most one byte apart (the two round the same f32 value where the f32 plans agree bit for bit)."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def lib_name():
    """the library this process loads, relative to the repository"""
    lib = os.environ.get("RECFILTER_AMD_LIB")
    return os.path.relpath(lib, ROOT) if lib else "(built)"


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
    print(f"u8_probe: shape {shape} order {a.order} steps {a.steps} warmup {a.warmup} rounds {a.rounds} lib {lib_name()}")
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


def run_volume(a):
    import numpy as np
    import torch
    import recfilter_amd as rfa
    from recfilter_amd import capi
    if not torch.cuda.is_available():
        sys.exit("u8_probe: needs a GPU")
    w = rfa.gaussian_weights(5.0, a.order)
    scans = [(d, c, w) for d in (0, 1, 2) for c in (True, False)]
    pw = dict(prologue=(1.0 / 255.0, 0.0), epilogue=(255.0, 0.0, 0.0))
    io = dict(dtype=np.float32, input_dtype=np.uint8, output_dtype=np.uint8, clamped=True, **pw)
    print(f"u8_probe --volume: order {a.order} warmup {a.warmup} rounds {a.rounds} lib {lib_name()}")
    summary = []
    for size in a.sizes:
        shape = tuple(int(v) for v in size.split(","))
        samples = shape[0] * shape[1] * shape[2]
        steps = max(5, min(a.steps, (1 << 28) // samples))
        xb = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
        xf = xb.float()
        specs = [("native", dict(io, path=capi.RF_PATH_TILED_FUSED, flags=0), torch.uint8),
                 ("staged", dict(io, path=capi.RF_PATH_AUTO, flags=capi.RF_PLAN_STAGE_HALF), torch.uint8),
                 ("staged_2", dict(io, path=capi.RF_PATH_AUTO, flags=capi.RF_PLAN_STAGE_HALF), torch.uint8),
                 ("f32", dict(dtype=np.float32, clamped=True, path=capi.RF_PATH_AUTO, flags=0, **pw), torch.float32)]
        plans = {name: (rfa.Plan(shape, scans, **kw), torch.empty(shape, dtype=tdt, device="cuda"), xf if name == "f32" else xb)
                 for name, kw, tdt in specs}
        print(f"size {shape} = 2^{np.log2(samples):.1f} samples, steps {steps}")
        for name, (plan, out, x) in plans.items():
            for _ in range(a.warmup):
                plan.execute([x], [out])
            _, timed = plan.execute_timed([x], [out])
            print(f"  {name:9s} path {plan.path_name} tiles {plan.tiles} launches {[n for n, _ in timed]} workspace {plan.workspace_bytes / 2**20:.1f} MiB")
        torch.cuda.synchronize()
        diff = (plans["native"][1].to(torch.int16) - plans["staged"][1].to(torch.int16)).abs()
        worst = int(diff.max())
        print(f"  native against staged: max byte difference {worst}, differing samples {int((diff != 0).sum())} of {samples}")
        if worst > 1:
            sys.exit("u8_probe: the native plan is more than one byte from the staged one")
        del diff
        step = {n: [] for n in plans}
        kern = {}
        for _ in range(a.rounds):
            for name, (plan, out, x) in plans.items():
                plan.execute([x], [out])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    plan.execute([x], [out])
                e1.record()
                e1.synchronize()
                step[name].append(e0.elapsed_time(e1) / steps)
                if name == "native":
                    _, timed = plan.execute_timed([x], [out])
                    for i, (k, ms) in enumerate(timed):
                        kern.setdefault((i, k), []).append(ms)
        med = {n: statistics.median(v) for n, v in step.items()}
        for name in plans:
            print(f"  {name:9s} ms_per_step median {med[name]:.4f} min {min(step[name]):.4f} max {max(step[name]):.4f}")
        print("  native kernels: " + " ".join(f"{k}={statistics.median(v) * 1e3:.1f}us" for (_, k), v in sorted(kern.items())))
        spread = abs(med["staged_2"] - med["staged"])
        gain = med["staged"] - med["native"]
        ahead = gain > spread
        print(f"  native / staged: {med['native'] / med['staged']:.3f} (byte model 15 / 23 = 0.652)   staged_2 / staged: "
              f"{med['staged_2'] / med['staged']:.3f}   native / f32: {med['native'] / med['f32']:.3f}")
        print(f"  verdict: staged - native = {gain * 1e3:.1f} us, noise floor {spread * 1e3:.1f} us: native is {'AHEAD' if ahead else 'NOT ahead'}")
        summary.append((shape, med["native"], med["staged"], med["staged_2"], med["f32"], ahead))
        for plan, _, _ in plans.values():
            plan.close()
        del plans, xb, xf
        torch.cuda.empty_cache()
    print("summary: size native staged staged_2 f32 (ms per step) native/staged ahead")
    for shape, n, st, s2, f, ahead in summary:
        print(f"  {'x'.join(map(str, shape)):>14s} {n:.4f} {st:.4f} {s2:.4f} {f:.4f} {n / st:.3f} {'yes' if ahead else 'no'}")


VOLUME_SIZES = ["128,128,128", "128,256,256", "256,256,256", "512,512,512", "1024,1024,1024"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", action="store_true", help="byte volumes (x, y and z scans) over --sizes instead of one image")
    ap.add_argument("--sizes", nargs="+", default=VOLUME_SIZES, metavar="Z,Y,X")
    ap.add_argument("--shape", type=int, nargs=2, default=[16384, 16384], metavar=("ROWS", "WIDTH"))
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--packed-lib", default=None, help="a library built with -DRF_U8_PACKED_STORES: run again on it, in a fresh child process")
    ap.add_argument("--child-timeout", type=int, default=900, help="seconds a child process of --packed-lib may take")
    a = ap.parse_args()
    if a.packed_lib is None:
        return run_volume(a) if a.volume else run(a)
    # (one process per library: the library is chosen when recfilter_amd loads it.  This parent opens no GPU itself.)
    args = [sys.executable, os.path.abspath(__file__), "--shape", str(a.shape[0]), str(a.shape[1]), "--order", str(a.order),
            "--steps", str(a.steps), "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
    if a.volume:
        args += ["--volume", "--sizes"] + list(a.sizes)
    for lib in (None, os.path.abspath(a.packed_lib), None, os.path.abspath(a.packed_lib)):       # alternating: plain, packed, plain, packed
        env = dict(os.environ)
        env.pop("RECFILTER_AMD_LIB", None)
        if lib:
            env["RECFILTER_AMD_LIB"] = lib
        print(f"---- {'packed stores: ' + os.path.relpath(lib, ROOT) if lib else 'plain stores (the built library)'}", flush=True)
        rc = subprocess.run(args, env=env, timeout=a.child_timeout).returncode
        if rc != 0:
            sys.exit(rc)      # (a failed run ends the probe: nothing more is started on the GPU)


if __name__ == "__main__":
    main()
