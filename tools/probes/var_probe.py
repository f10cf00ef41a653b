#!/usr/bin/env python3
"""Spatially varying first-order scans (rf_var_plan_*): per-kernel and whole-step times of the `+x -x +y -y` plan beside the
measured copy ceiling and beside the constant-coefficient order-1 plan of the same shape, alternating in ONE process.

    python tools/probes/var_probe.py [--sizes 4096 16384] [--planes 1 3] [--steps 10] [--rounds 5] [--report scans|power]

Per size (square images) and plane count it builds
    varying   VarPlan: +x -x on weight plane 0, +y -y on weight plane 1 (two fused stages, six launches)
    constant  Plan: the order-1 recursive Gaussian (sigma 5) +x -x +y -y, zero border, automatic path
warms both up with rf_stream_copy, then runs `rounds` rounds; each round times rf_stream_copy of one plane, `steps` executes of
each plan between two HIP events, and one execute_timed() of the varying plan for the per-kernel times.  Printed: medians over
the rounds; per kernel the bytes of the byte model (a tails pass reads image and weights, 8 B per sample and
plane, and writes 2 tails per plane + 3 per weight plane; the carry pass reads those and the causal carries and writes 2 carries
per plane; a final pass reads image and weights and writes the image, 12 B per sample and plane, and reads the carries), the
rate they give and that rate as a fraction of the copy's (8 B per sample over its time); the whole step against the constant
plan's.

--report power: the power form (rf_var_plan_execute_power: exponent planes, w = a^d formed in the kernels) beside the plane form
of the SAME plan, alternating in the same process, medians over the rounds with the rounds' min and max:
    forms    per round `steps` executes of each form between two events and one timed execute of each for the per-kernel times;
             exponents 1 + 30 u^4 with base 0.9, weight planes 0.9^d: the two forms compute the same filter
    filter   the whole domain-transform filter at K = 3 on an image that guides itself, both ways: domain_transform_weights
             (torch, 2 K weight planes) + K executes against domain_transform_distances (rf_var_distances, 2 planes) + K
             execute_power; with torch's peak device memory during one filter, above what the image and its output hold."""
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


def spread(v):
    return f"(min {min(v):.4f}, max {max(v):.4f})"


def probe_forms(n, planes, steps, rounds):
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(16)
    base = 0.9
    ins = [torch.rand((n, n), device="cuda", generator=gen) * 2 - 1 for _ in range(planes)]
    outs = [torch.empty_like(t) for t in ins]
    ds = [1 + 30 * torch.rand((n, n), device="cuda", generator=gen) ** 4 for _ in range(2)]
    ws = [torch.pow(base, d) for d in ds]
    scans = [(0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1)]
    med = statistics.median
    with rfa.VarPlan((n, n), scans, planes=planes, n_weights=2) as plan:
        run_planes = lambda: plan.execute(ins, ws, outs)                          # noqa: E731
        run_power = lambda: plan.execute_power(ins, ds, [base, base], outs)       # noqa: E731
        for _ in range(3):
            rfa.stream_copy_ms(ins[0], outs[0], reps=2)
            run_planes()
            run_power()
        torch.cuda.synchronize()
        step = {"planes": [], "power": []}
        kernels = {"planes": {}, "power": {}}
        for _ in range(rounds):
            step["planes"].append(timed(run_planes, steps))
            step["power"].append(timed(run_power, steps))
            for form, times in (("planes", plan.execute_timed(ins, ws, outs)[1]), ("power", plan.execute_power_timed(ins, ds, [base, base], outs)[1])):
                for i, (name, ms) in enumerate(times):
                    kernels[form].setdefault((i, name), []).append(ms)
        print(f"== forms, {n} x {n}, {planes} plane(s)")
        print(f"   {'launch':<18} {'planes ms':>10} {'power ms':>10} {'power/planes':>13}   planes (min, max)    power (min, max)")
        for key in sorted(kernels["planes"]):
            a, b = kernels["planes"][key], kernels["power"][key]
            print(f"   {key[0]} {key[1]:<16} {med(a):10.4f} {med(b):10.4f} {med(b) / med(a):13.3f}   {spread(a)}   {spread(b)}")
        a, b = step["planes"], step["power"]
        print(f"   {'step (6 launches)':<18} {med(a):10.4f} {med(b):10.4f} {med(b) / med(a):13.3f}   {spread(a)}   {spread(b)}")


def probe_filter(n, planes, steps, rounds, K=3, sigma_s=60.0, sigma_r=0.4):
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(17)
    image = torch.rand((planes, n, n), device="cuda", generator=gen)
    out = torch.empty_like(image)
    src0 = [image[c] for c in range(planes)]
    outs = [out[c] for c in range(planes)]
    scans = [(0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1)]
    bases = rfa.domain_transform_bases(sigma_s, K)
    med = statistics.median
    with rfa.VarPlan((n, n), scans, planes=planes, n_weights=2) as plan:
        def filter_planes():
            src = src0
            for wx, wy in rfa.domain_transform_weights(image, sigma_s, sigma_r, K):
                plan.execute(src, [wx, wy], outs)
                src = outs

        def filter_power():
            src = src0
            d = list(rfa.domain_transform_distances(image, sigma_s, sigma_r))
            for a in bases:
                plan.execute_power(src, d, [a, a], outs)
                src = outs

        def weights_only():
            rfa.domain_transform_weights(image, sigma_s, sigma_r, K)

        def distances_only():
            rfa.domain_transform_distances(image, sigma_s, sigma_r)
        peak = {}
        for name, fn in (("planes", filter_planes), ("power", filter_power)):
            fn()                                                   # (warm: code objects, torch's allocator)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            floor = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - floor
        t = {"planes": [], "power": [], "weights": [], "distances": []}
        for _ in range(rounds):
            t["planes"].append(timed(filter_planes, steps))
            t["power"].append(timed(filter_power, steps))
            t["weights"].append(timed(weights_only, steps))
            t["distances"].append(timed(distances_only, steps))
        print(f"== filter, K = {K}, {n} x {n}, {planes} plane(s), {steps} filter(s) per window: image and output {2 * image.numel() * 4 / 2**30:.2f} GiB, workspace {plan.workspace_bytes / 2**20:.1f} MiB")
        print(f"   planes form: weights (torch) + {K} executes      {med(t['planes']):9.3f} ms   {spread(t['planes'])}   peak above the images {peak['planes'] / 2**30:6.2f} GiB")
        print(f"   power form: distances (HIP) + {K} execute_power  {med(t['power']):9.3f} ms   {spread(t['power'])}   peak above the images {peak['power'] / 2**30:6.2f} GiB")
        print(f"   power / planes                                  {med(t['power']) / med(t['planes']):9.3f}")
        print(f"   domain_transform_weights alone                  {med(t['weights']):9.3f} ms   {spread(t['weights'])}")
        print(f"   domain_transform_distances alone                {med(t['distances']):9.3f} ms   {spread(t['distances'])}")
    del image, out
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--planes", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--report", choices=["scans", "power"], default="scans")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("var_probe: needs a GPU")
    print(f"var_probe: {torch.cuda.get_device_name(0)}; report {a.report}; steps {a.steps}, rounds {a.rounds}; medians over the rounds")
    for n in a.sizes:
        for planes in a.planes:
            if a.report == "scans":
                probe(n, planes, a.steps, a.rounds)
            else:
                probe_forms(n, planes, a.steps, a.rounds)
                torch.cuda.empty_cache()
                probe_filter(n, planes, max(1, int(a.steps * (4096 / n) ** 2)), a.rounds)      # (whole filters per timed window)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
