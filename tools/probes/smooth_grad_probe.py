#!/usr/bin/env python3
"""The differentiable smoothing plan (rf_smooth_plan_backward): whole-step and per-kernel times of the plan's forward, of its backward
with the distances held constant (edges = 0) and through them (edges = 1), and beside them the only differentiable route there
was before it -- edge_aware_smooth(form="planes") forward plus .backward() with image and guide requiring gradients -- with the
peak device memory of both routes.  Everything alternates in ONE process.

    python tools/probes/smooth_grad_probe.py [--cases 1024x3 4096x1] [--iterations 3] [--steps 10] [--rounds 5]

Per case (square images, SIZExPLANES; a separate f32 guide of as many planes) it builds one SmoothPlan, warms everything up, then
runs `rounds` rounds; each round times `steps` plan executes, `steps` backward calls of each kind, `steps` forward-plus-backward
passes of each autograd route (SmoothPlan.apply and form="planes"), each between two HIP events, and one timed call of each kind for
the per-kernel times.  Printed: medians over the rounds with the rounds' min and max, ratios, and the byte model's figures
(per sample, tails aside).  With P image planes, G guide planes and K iterations:
    var_distances 4 G + 8;  a fused forward stage 20 P, an iteration 40 P;  an adjoint stage 20 P, an iteration's four 80 P;
    with exponent gradients an iteration adds per scan the recompute's 20 P, the state's 4 P, var_grad's 12 P + 4 (the exponent
    plane) and the gradient plane, 4 where it is stored (the first two launches of the whole call) and 8 where it is added to;
    var_distances_grad 8 + 8 G (12 G where it adds: the image guiding itself).
Peak memory: torch.cuda.max_memory_allocated over one forward-plus-backward pass, to which the plan's own allocations (its
workspace and backward workspace, which torch's allocator does not see) are added for the plan's route."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SIGMA_S, SIGMA_R = 40.0, 0.5


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


def model_bytes(P, G, K):
    """(forward, backward edges = 0, backward edges = 1) bytes per sample of the byte model"""
    distances = 4 * G + 8
    forward = distances + 40 * P * K
    held = distances + 80 * P * K
    per_scan = 20 * P + 4 * P + 12 * P + 4
    through = distances + 40 * P * (K - 1) + K * (80 * P + 4 * per_scan) + (2 * 4 + (4 * K - 2) * 8) + 8 + 8 * G
    return forward, held, through


def probe(n, planes, K, steps, rounds):
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(19)
    rand = lambda *shape: torch.rand(shape, device="cuda", generator=gen)      # noqa: E731
    image, guide, g = rand(planes, n, n), rand(planes, n, n), rand(planes, n, n) * 2 - 1
    out, gim, ggd = torch.empty_like(image), torch.empty_like(image), torch.empty_like(guide)
    med = statistics.median
    MiB = 2.0 ** 20
    with rfa.SmoothPlan((n, n), planes=planes, guide_planes=planes, iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R) as plan:
        def autograd_plan():
            im, gd = image.detach().requires_grad_(True), guide.detach().requires_grad_(True)
            plan.apply(im, gd).backward(g)

        def autograd_planes():
            im, gd = image.detach().requires_grad_(True), guide.detach().requires_grad_(True)
            rfa.edge_aware_smooth(im, guide=gd, sigma_s=SIGMA_S, sigma_r=SIGMA_R, iterations=K, form="planes").backward(g)
        run = {"forward": lambda: plan.execute(image, guide, out),
               "backward edges=0": lambda: plan.backward(None, guide, g, gim, None, edges=False),
               "backward edges=1": lambda: plan.backward(image, guide, g, gim, ggd, edges=True),
               "autograd, plan": autograd_plan,
               "autograd, planes": autograd_planes}
        for _ in range(2):
            for fn in run.values():
                fn()
        torch.cuda.synchronize()
        peak = {}
        for k in ("autograd, plan", "autograd, planes"):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            run[k]()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
        own = plan.workspace_bytes + plan.backward_workspace_bytes(True)
        step = {k: [] for k in run}
        kernels = {"forward": {}, "backward edges=0": {}, "backward edges=1": {}}
        for _ in range(rounds):
            for k, fn in run.items():
                step[k].append(timed(fn, steps if k.startswith(("forward", "backward")) else max(1, steps // 3)))
            for k, times in (("forward", plan.execute_timed(image, guide, out)[1]),
                             ("backward edges=0", plan.backward_timed(None, guide, g, gim, None, edges=False)[2]),
                             ("backward edges=1", plan.backward_timed(image, guide, g, gim, ggd, edges=True)[2])):
                for i, (name, ms) in enumerate(times):
                    kernels[k].setdefault((i, name), []).append(ms)
        print(f"== {n} x {n}, {planes} plane(s), K = {K}: workspace {plan.workspace_bytes / MiB:.1f} MiB, "
              f"+ {plan.backward_workspace_bytes(True) / MiB:.1f} MiB for edges = 1")
        for k in kernels:
            print(f"   -- {k}: {len(kernels[k])} launches")
            by_name = {}
            for (i, name), ms in sorted(kernels[k].items()):
                print(f"   {i:3d} {name:<20} {med(ms):8.4f} ms   {spread(ms)}")
                by_name[name] = by_name.get(name, 0.0) + med(ms)
            print("       by name: " + ", ".join(f"{name} {ms:.4f}" for name, ms in by_name.items()))
        model = dict(zip(kernels, model_bytes(planes, planes, K)))
        for k in run:
            tail = f"   byte model {model[k]:5d} B per sample" if k in model else ""
            print(f"   {k + ' step':<24} {med(step[k]):9.4f} ms   {spread(step[k])}{tail}")
        f = med(step["forward"])
        for k in ("backward edges=0", "backward edges=1"):
            print(f"   {k} / forward: measured {med(step[k]) / f:5.2f}, byte model {model[k] / model['forward']:5.2f}")
        print(f"   forward + backward through autograd, plan / planes: {med(step['autograd, plan']) / med(step['autograd, planes']):5.2f} "
              f"({med(step['autograd, plan']):.4f} ms against {med(step['autograd, planes']):.4f} ms)")
        print(f"   peak device memory of one such pass: plan {peak['autograd, plan'] / MiB:.1f} MiB in torch + {own / MiB:.1f} MiB the plan's own "
              f"= {(peak['autograd, plan'] + own) / MiB:.1f} MiB; planes {peak['autograd, planes'] / MiB:.1f} MiB in torch "
              f"(+ the varying plan's workspace and its backward planes, which torch does not see)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="+", default=["1024x3", "4096x1"], help="SIZExPLANES")
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("smooth_grad_probe: needs a GPU")
    print(f"smooth_grad_probe: {torch.cuda.get_device_name(0)}; K {a.iterations}, steps {a.steps}, rounds {a.rounds}; medians over the rounds")
    for case in a.cases:
        n, planes = (int(v) for v in case.split("x"))
        probe(n, planes, a.iterations, a.steps, a.rounds)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
