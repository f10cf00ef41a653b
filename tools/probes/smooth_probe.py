#!/usr/bin/env python3
"""The smoothing plan (rf_smooth_plan_*, recfilter_amd.SmoothPlan) beside what a caller has without it, alternating in ONE
process; medians over the rounds with the rounds' min and max.

    python tools/probes/smooth_probe.py [--sizes 4096 16384] [--planes 1 3] [--steps 10] [--rounds 5] [--iterations 3]

Per size (square images) and plane count, on an image that guides itself, sigma_s 60, sigma_r 0.4:
    f32      SmoothPlan on an f32 image  against  edge_aware_smooth(form="power") on the same image
    bytes    SmoothPlan on a uint8 image  against  the route a caller of edge_aware_smooth(form="power") has for a byte image:
             image.float() -> edge_aware_smooth(form="power", guide=image) -> round().clamp(0, 255).to(uint8);
             with torch's peak device memory during one filter, above what the byte image and its byte output hold
    kernels  execute_timed of the byte plan beside execute_timed of the f32 plan, launch by launch: the three byte instances
             (iteration 0: var_tails_x and var_pass2_x read bytes; iteration K-1: var_pass2_y stores bytes) against their f32
             twins in the other plan, and every other launch as the control (the same kernel in both plans)
Each round times `steps` filters of each route between two events (steps scaled down with the area) and one execute_timed of
each plan."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SIGMA_S, SIGMA_R = 60.0, 0.4


def timed(fn, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def spread(v):
    return f"(min {min(v):.4f}, max {max(v):.4f})"


def peak_above(fn):
    """torch's peak device memory during one fn(), above what is allocated when it starts"""
    import torch
    fn()                                                   # (warm: code objects, torch's allocator, the cached plans)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    floor = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    result = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - floor
    del result
    return peak


def probe(n, planes, steps, rounds, K):
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(18)
    med = statistics.median
    img8 = torch.randint(0, 256, (planes, n, n), device="cuda", generator=gen, dtype=torch.uint8)
    out8 = torch.empty_like(img8)
    img32 = img8.float() / 255.0
    out32 = torch.empty_like(img32)
    with rfa.SmoothPlan((n, n), planes=planes, image_dtype=torch.uint8, iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R) as p8, \
            rfa.SmoothPlan((n, n), planes=planes, iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R) as p32:
        plan32 = lambda: p32.execute(img32, None, out32)                                                                   # noqa: E731
        power32 = lambda: rfa.edge_aware_smooth(img32, sigma_s=SIGMA_S, sigma_r=SIGMA_R, iterations=K, form="power")        # noqa: E731
        plan8 = lambda: p8.execute(img8, None, out8)                                                                       # noqa: E731
        route8 = lambda: rfa.edge_aware_smooth(img8.float(), guide=img8, sigma_s=SIGMA_S, sigma_r=SIGMA_R, iterations=K,   # noqa: E731
                                               form="power").round().clamp(0, 255).to(torch.uint8)
        for fn in (plan32, power32, plan8, route8):
            fn()
        torch.cuda.synchronize()
        t = {"plan32": [], "power32": [], "plan8": [], "route8": []}
        kernels = {"u8": {}, "f32": {}}
        for _ in range(rounds):
            t["plan32"].append(timed(plan32, steps))
            t["power32"].append(timed(power32, steps))
            t["plan8"].append(timed(plan8, steps))
            t["route8"].append(timed(route8, steps))
            for kind, times in (("u8", p8.execute_timed(img8, None, out8)[1]), ("f32", p32.execute_timed(img32, None, out32)[1])):
                for i, (name, ms) in enumerate(times):
                    kernels[kind].setdefault((i, name), []).append(ms)
        ws8, ws32 = p8.workspace_bytes, p32.workspace_bytes
        print(f"== {n} x {n}, {planes} plane(s), K = {K}, {steps} filter(s) per window: byte image and output {2 * img8.numel() / 2**30:.3f} GiB, "
              f"f32 image and output {2 * img32.numel() * 4 / 2**30:.3f} GiB")
        print(f"   workspace: byte plan {ws8 / 2**30:.3f} GiB, f32 plan {ws32 / 2**30:.3f} GiB")
        a, b = t["plan32"], t["power32"]
        print(f"   f32    SmoothPlan                               {med(a):9.3f} ms   {spread(a)}")
        print(f"   f32    edge_aware_smooth(form=\"power\")          {med(b):9.3f} ms   {spread(b)}")
        print(f"   f32    plan / power                             {med(a) / med(b):9.3f}")
        a, b = t["plan8"], t["route8"]
        print(f"   bytes  SmoothPlan                               {med(a):9.3f} ms   {spread(a)}")
        print(f"   bytes  float() -> form=\"power\" -> round/clamp/u8 {med(b):9.3f} ms   {spread(b)}")
        print(f"   bytes  plan / route                             {med(a) / med(b):9.3f}")
        print(f"   bytes plan / f32 plan                           {med(t['plan8']) / med(t['plan32']):9.3f}")
        print(f"   {'launch':<20} {'byte plan ms':>12} {'f32 plan ms':>12} {'byte/f32':>9}   byte (min, max)      f32 (min, max)")
        last = max(i for i, _ in kernels["u8"])
        for key in sorted(kernels["u8"]):
            x, y = kernels["u8"][key], kernels["f32"][key]
            byte_instance = key[0] in (1, 3) or key[0] == last
            print(f"   {key[0]:>2} {key[1]:<17} {med(x):12.4f} {med(y):12.4f} {med(x) / med(y):9.3f}   {spread(x)}   {spread(y)}"
                  f"{'   <- byte instance' if byte_instance else ''}")
    # peak memory of one filter of each byte route, with nothing else of this probe alive but the byte image and its output
    del img32, out32
    torch.cuda.empty_cache()
    with rfa.SmoothPlan((n, n), planes=planes, image_dtype=torch.uint8, iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R) as p8:
        peak_plan = peak_above(lambda: p8.execute(img8, None, out8))
        print(f"   bytes  SmoothPlan: peak above image and output  {(peak_plan + p8.workspace_bytes) / 2**30:9.3f} GiB   "
              f"(the plan's workspace, allocated by the library: {p8.workspace_bytes / 2**30:.3f} GiB; torch's own peak {peak_plan / 2**30:.3f} GiB)")
    route = lambda: rfa.edge_aware_smooth(img8.float(), guide=img8, sigma_s=SIGMA_S, sigma_r=SIGMA_R, iterations=K,      # noqa: E731
                                          form="power").round().clamp(0, 255).to(torch.uint8)
    peak_route = peak_above(route)
    var_ws = 0
    for plan in rfa.varscan._smooth_plans.values():
        if plan.shape == (n, n) and plan.planes == planes:
            var_ws = plan.workspace_bytes
    print(f"   bytes  route: peak above image and output       {(peak_route + var_ws) / 2**30:9.3f} GiB   "
          f"(torch's peak {peak_route / 2**30:.3f} GiB + the cached varying plan's workspace {var_ws / 2**30:.3f} GiB)")
    for plan in list(rfa.varscan._smooth_plans.values()):
        plan.close()
    rfa.varscan._smooth_plans.clear()
    del img8, out8
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--planes", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("smooth_probe: needs a GPU")
    print(f"smooth_probe: {torch.cuda.get_device_name(0)}; steps {a.steps} at 4096^2 (scaled with the area), rounds {a.rounds}; medians over the rounds")
    for n in a.sizes:
        for planes in a.planes:
            probe(n, planes, max(1, int(a.steps * (4096 / n) ** 2)), a.rounds, a.iterations)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
