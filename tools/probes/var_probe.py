#!/usr/bin/env python3
"""Spatially varying first-order scans (rf_var_plan_*): per-kernel and whole-step times of the `+x -x +y -y` plan beside the
measured copy ceiling and beside the constant-coefficient order-1 plan of the same shape, alternating in ONE process.

    python tools/probes/var_probe.py [--sizes 4096 16384] [--planes 1 3] [--steps 10] [--rounds 5]

Per size (square images) and plane count it builds
    varying   VarPlan: +x -x on weight plane 0, +y -y on weight plane 1 (two fused stages, six launches)
    constant  Plan: the order-1 recursive Gaussian (sigma 5) +x -x +y -y, zero border, automatic path
warms both up with rf_stream_copy, then runs `rounds` rounds; each round times rf_stream_copy of one plane, `steps` executes of
each plan between two HIP events, and one execute_timed() of the varying plan for the per-kernel times.  Printed: medians over
the rounds; per kernel the bytes of the byte model (a tails pass reads image and weights, 8 B per sample and
plane, and writes 2 tails per plane + 3 per weight plane; the carry pass reads those and the causal carries and writes 2 carries
per plane; a final pass reads image and weights and writes the image, 12 B per sample and plane, and reads the carries), the
rate they give and that rate as a fraction of the copy's (8 B per sample over its time); the whole step against the constant
plan's."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

TILE = 64


def kernel_bytes(name, n, planes):
    """bytes of the byte model for one launch on an n x n image"""
    slots = n * ((n + TILE - 1) // TILE) * 4          # one f32 per line and tile
    if name.startswith("var_tails"):
        return 8 * n * n * planes + slots * (2 * planes + 3)
    if name == "var_carry":
        return slots * ((2 * planes + 3) + planes + 2 * planes)
    return 12 * n * n * planes + slots * 2 * planes


def timed(fn, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def probe(n, planes, steps, rounds):
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(15)
    ins = [torch.rand((n, n), device="cuda", generator=gen) * 2 - 1 for _ in range(planes)]
    outs = [torch.empty_like(t) for t in ins]
    ws = [torch.rand((n, n), device="cuda", generator=gen) ** 0.25 for _ in range(2)]
    g = rfa.gaussian_weights(5.0, 1)
    var_scans = [(0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1)]
    const_scans = [(0, True, g), (0, False, g), (1, True, g), (1, False, g)]
    with rfa.VarPlan((n, n), var_scans, planes=planes, n_weights=2) as var, \
            rfa.Plan((n, n), const_scans, planes=planes, flags=0) as const:
        run_var = lambda: var.execute(ins, ws, outs)              # noqa: E731
        run_const = lambda: const.execute(ins, outs)              # noqa: E731
        for _ in range(3):
            rfa.stream_copy_ms(ins[0], outs[0], reps=2)
            run_var()
            run_const()
        torch.cuda.synchronize()
        copy, step_var, step_const, kernels = [], [], [], {}
        for _ in range(rounds):
            copy.append(rfa.stream_copy_ms(ins[0], outs[0], reps=steps))
            step_var.append(timed(run_var, steps))
            step_const.append(timed(run_const, steps))
            _, times = var.execute_timed(ins, ws, outs)
            for i, (name, ms) in enumerate(times):
                kernels.setdefault((i, name), []).append(ms)
        med = statistics.median
        copy_ms = med(copy)
        copy_rate = 8.0 * n * n / (copy_ms * 1e-3)
        print(f"== {n} x {n}, {planes} plane(s): workspace {var.workspace_bytes / 2**20:.1f} MiB, constant plan on path {const.path_name} "
              f"({const.num_kernels} launches)")
        print(f"   rf_stream_copy of one plane      {copy_ms:8.4f} ms   {copy_rate / 1e12:6.3f} TB/s   (min {min(copy):.4f}, max {max(copy):.4f})")
        for (i, name), ms in sorted(kernels.items()):
            b = kernel_bytes(name, n, planes)
            rate = b / (med(ms) * 1e-3)
            print(f"   {i} {name:<14} {med(ms):8.4f} ms   {b / 2**20:9.1f} MiB   {rate / 1e12:6.3f} TB/s   {rate / copy_rate:5.2f} of the copy rate")
        print(f"   varying step (6 launches)        {med(step_var):8.4f} ms   (min {min(step_var):.4f}, max {max(step_var):.4f})")
        print(f"   constant order-1 step            {med(step_const):8.4f} ms   (min {min(step_const):.4f}, max {max(step_const):.4f})")
        print(f"   varying / constant               {med(step_var) / med(step_const):8.2f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--planes", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("var_probe: needs a GPU")
    print(f"var_probe: {torch.cuda.get_device_name(0)}; steps {a.steps}, rounds {a.rounds}; medians over the rounds")
    for n in a.sizes:
        for planes in a.planes:
            probe(n, planes, a.steps, a.rounds)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
