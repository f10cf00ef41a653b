#!/usr/bin/env python3
"""The differentiable smoothing plan on volumes (RF_SMOOTH_VOLUME_BACKWARD; rf_var_distances_volume_backward): whole-step times of the
plan's forward, of its backward with the distances held constant (edges = 0) and through them (edges = 1) beside the byte model,
var_distances_volume_grad alone as a rate of its byte model beside rf_stream_copy, and forward plus backward through autograd against
the only differentiable route there was before -- the distances and the weights a_k ** d as torch expressions, then K
var_scan_volume calls -- with the peak device memory of both routes.  Everything alternates in ONE process.

    python tools/probes/smooth_volume_grad_probe.py [--section plan|distances|all] [--cases 128x1 128x3 256x1 256x3]
                                                    [--distance-cases 256x1 256x3 512x1 512x3] [--iterations 3] [--steps 10]
                                                    [--rounds 5] [--out FILE]

plan: per case (cubes, EDGExPLANES; a separate f32 guide of as many volumes) one SmoothPlan.volume(..., differentiable=True), warmed
up, then `rounds` rounds; each round times `steps` executes, `steps` backward calls of each kind and a third as many
forward-plus-backward passes of each autograd route, each between two HIP events, and one timed backward of each kind for the times
by kernel name.  Printed: medians over the rounds with the rounds' min and max, ratios, and the byte model's figures.
distances: per case (EDGExCHANNELS) var_distances_volume_grad storing and adding, and rf_stream_copy of one volume, alternating.

The byte model, per sample, tails and carries aside (7/64 of a stage), with P volumes, G guide volumes and K iterations, from the
launch lists of DESIGN.md 5.20:
    var_distances_volume 4 G + 12;  a pair stage reads P + 1 volumes twice and writes P: 12 P + 8, an iteration's three 36 P + 24;
    an adjoint stage (a single scan) 12 P + 8, an iteration's six 72 P + 48                       edges = 0: 4 G + 12 + K (72 P + 48)
    with exponent gradients an iteration adds per scan the recompute's 12 P + 8, the state's 4 P and var_grad's 12 P + 4 (the
    exponent volume) plus the gradient volume, 4 where it is stored (the first three launches of the whole call) and 8 where it
    is added to; the checkpointed forward (K - 1)(36 P + 24); var_distances_volume_grad 12 + 8 G (12 + 12 G where it adds).
Peak memory: torch.cuda.max_memory_allocated over one forward-plus-backward pass, plus what torch's allocator does not see: the
smoothing plan's workspace and backward workspace on the plan's route, the cached volume plan's on the other."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SIGMA_S, SIGMA_R, SPACING_Z = 40.0, 0.5, 2.5
FULL = [(0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1), (2, True, 2), (2, False, 2)]
med = statistics.median
MiB = 2.0 ** 20
OUT = None


def say(line=""):
    print(line, flush=True)
    if OUT is not None:
        OUT.write(line + "\n")
        OUT.flush()


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
    distances = 4 * G + 12
    forward = distances + K * (36 * P + 24)
    held = distances + K * (72 * P + 48)
    per_scan = (12 * P + 8) + (12 * P + 8 + 4 * P) + (12 * P + 4)      # the recompute, the adjoint stage with its state, var_grad
    through = distances + (K - 1) * (36 * P + 24) + K * 6 * per_scan + (3 * 4 + (6 * K - 3) * 8) + 12 + 8 * G
    return forward, held, through


def torch_route(image, guide, bases, g):
    """forward plus backward of the filter with the distances and the weights as torch expressions and K var_scan_volume calls"""
    import torch
    import recfilter_amd as rfa
    scale = SIGMA_S / SIGMA_R
    im, gd = image.detach().requires_grad_(True), guide.detach().requires_grad_(True)
    dx = torch.cat([torch.ones_like(gd[0, :, :, :1]), 1 + scale * (gd[:, :, :, 1:] - gd[:, :, :, :-1]).abs().sum(0)], dim=2)
    dy = torch.cat([torch.ones_like(gd[0, :, :1, :]), 1 + scale * (gd[:, :, 1:, :] - gd[:, :, :-1, :]).abs().sum(0)], dim=1)
    dz = torch.cat([torch.full_like(gd[0, :1], SPACING_Z), SPACING_Z + scale * (gd[:, 1:] - gd[:, :-1]).abs().sum(0)], dim=0)
    volumes = [im[c] for c in range(im.shape[0])]
    for a in bases:
        volumes = rfa.var_scan_volume(volumes, [torch.pow(a, d).contiguous() for d in (dx, dy, dz)], FULL)
    torch.stack(list(volumes)).backward(g)
    return im.grad, gd.grad


def probe_plan(n, planes, K, steps, rounds):
    import torch
    import recfilter_amd as rfa
    from recfilter_amd import varscan
    gen = torch.Generator(device="cuda").manual_seed(27)
    rand = lambda *shape: torch.rand(shape, device="cuda", generator=gen)      # noqa: E731
    image, guide, g = rand(planes, n, n, n), rand(planes, n, n, n), rand(planes, n, n, n) * 2 - 1
    out, gim, ggd = torch.empty_like(image), torch.empty_like(image), torch.empty_like(guide)
    with rfa.SmoothPlan.volume((n, n, n), planes=planes, guide_planes=planes, iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R, spacing_z=SPACING_Z,
                               differentiable=True) as plan:
        bases = plan.bases

        def autograd_plan():
            im, gd = image.detach().requires_grad_(True), guide.detach().requires_grad_(True)
            plan.apply(im, gd).backward(g)
        run = {"forward": lambda: plan.execute(image, guide, out),
               "backward edges=0": lambda: plan.backward(None, guide, g, gim, None, edges=False),
               "backward edges=1": lambda: plan.backward(image, guide, g, gim, ggd, edges=True),
               "autograd, plan": autograd_plan,
               "autograd, torch + var_scan_volume": lambda: torch_route(image, guide, bases, g)}
        for _ in range(2):
            for fn in run.values():
                fn()
        torch.cuda.synchronize()
        peak = {}
        for k in ("autograd, plan", "autograd, torch + var_scan_volume"):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            run[k]()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
        own = plan.workspace_bytes + plan.backward_workspace_bytes(True)
        other = sum(p.workspace_bytes + p.backward_workspace_bytes(True) for key, p in varscan._volume_plans.items() if key[0] == (n, n, n) and key[2] == planes)
        step = {k: [] for k in run}
        kernels = {"backward edges=0": {}, "backward edges=1": {}}
        for _ in range(rounds):
            for k, fn in run.items():
                step[k].append(timed(fn, steps if k.startswith(("forward", "backward")) else max(1, steps // 3)))
            for k, times in (("backward edges=0", plan.backward_timed(None, guide, g, gim, None, edges=False)[2]),
                             ("backward edges=1", plan.backward_timed(image, guide, g, gim, ggd, edges=True)[2])):
                by_name = {}
                for name, ms in times:
                    by_name[name] = by_name.get(name, 0.0) + ms
                for name, ms in by_name.items():
                    kernels[k].setdefault(name, []).append(ms)
        say(f"== {n}^3, {planes} volume(s), K = {K}: workspace {plan.workspace_bytes / MiB:.1f} MiB, + {plan.backward_workspace_bytes(True) / MiB:.1f} MiB for edges = 1; "
            f"launches {plan.num_kernels}, {plan.backward_num_kernels(False)}, {plan.backward_num_kernels(True)}")
        for k in kernels:
            say(f"   -- {k}, by kernel name (sum of its launches): " + ", ".join(f"{name} {med(ms):.4f}" for name, ms in kernels[k].items()))
        model = dict(zip(("forward", "backward edges=0", "backward edges=1"), model_bytes(planes, planes, K)))
        for k in run:
            tail = f"   byte model {model[k]:5d} B per sample -> {model[k] * n ** 3 / med(step[k]) / 1e6:7.1f} GB/s" if k in model else ""
            say(f"   {k + ' step':<40} {med(step[k]):9.4f} ms   {spread(step[k])}{tail}")
        f = med(step["forward"])
        for k in ("backward edges=0", "backward edges=1"):
            say(f"   {k} / forward: measured {med(step[k]) / f:5.2f}, byte model {model[k] / model['forward']:5.2f}")
        a, b = step["autograd, plan"], step["autograd, torch + var_scan_volume"]
        say(f"   forward + backward through autograd, plan / torch + var_scan_volume: {med(a) / med(b):5.2f} ({med(a):.4f} ms against {med(b):.4f} ms)")
        pa, pb = peak["autograd, plan"], peak["autograd, torch + var_scan_volume"]
        say(f"   peak device memory of one such pass: plan {pa / MiB:.1f} MiB in torch + {own / MiB:.1f} MiB the plan's own = {(pa + own) / MiB:.1f} MiB; "
            f"torch + var_scan_volume {pb / MiB:.1f} MiB in torch + {other / MiB:.1f} MiB the volume plan's own = {(pb + other) / MiB:.1f} MiB")


def probe_distances(n, channels, steps, rounds):
    import torch
    import recfilter_amd as rfa
    from recfilter_amd import capi
    gen = torch.Generator(device="cuda").manual_seed(28)
    guide = torch.rand((channels, n, n, n), device="cuda", generator=gen)
    gds = [torch.rand((n, n, n), device="cuda", generator=gen) * 2 - 1 for _ in range(3)]
    grad = torch.zeros_like(guide)
    copy_dst = torch.empty_like(gds[0])

    def stream_copy():
        capi.check(capi.lib().rf_stream_copy(ctypes.c_void_p(gds[0].data_ptr()), ctypes.c_void_p(copy_dst.data_ptr()), 1024, gds[0].numel() // 1024,
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    run = {"store": lambda: rfa.domain_transform_distances_volume_backward(guide, SIGMA_S, SIGMA_R, *gds, grad_guide=grad),
           "add": lambda: rfa.domain_transform_distances_volume_backward(guide, SIGMA_S, SIGMA_R, *gds, grad_guide=grad, accumulate=True),
           "rf_stream_copy": stream_copy}
    for fn in run.values():
        fn()
    torch.cuda.synchronize()
    step = {k: [] for k in run}
    for _ in range(rounds):
        for k, fn in run.items():
            step[k].append(timed(fn, steps))
    samples = n ** 3
    model = {"store": 12 + 8 * channels, "add": 12 + 12 * channels, "rf_stream_copy": 8}
    say(f"== var_distances_volume_grad, {n}^3, {channels} guide volume(s)")
    for k in run:
        say(f"   {k:<16} {med(step[k]):9.4f} ms   {spread(step[k])}   byte model {model[k]:4d} B per sample -> {model[k] * samples / med(step[k]) / 1e6:7.1f} GB/s")
    copy_rate = 8 * samples / med(step["rf_stream_copy"])
    for k in ("store", "add"):
        say(f"   {k}: {model[k] * samples / med(step[k]) / copy_rate:5.2f} of rf_stream_copy's rate")


def main():
    global OUT
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--section", choices=["plan", "distances", "all"], default="all")
    ap.add_argument("--cases", nargs="+", default=["128x1", "128x3", "256x1", "256x3"], help="EDGExPLANES")
    ap.add_argument("--distance-cases", nargs="+", default=["256x1", "256x3", "512x1", "512x3"], help="EDGExCHANNELS")
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("smooth_volume_grad_probe: needs a GPU")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        OUT = open(a.out, "a")
    say(f"smooth_volume_grad_probe --section {a.section}: {torch.cuda.get_device_name(0)}; K {a.iterations}, steps {a.steps}, rounds {a.rounds}; "
        f"medians over the rounds, everything alternating in one process")
    if a.section in ("plan", "all"):
        for case in a.cases:
            n, planes = (int(v) for v in case.split("x"))
            probe_plan(n, planes, a.iterations, a.steps, a.rounds)
            torch.cuda.empty_cache()
    if a.section in ("distances", "all"):
        for case in a.distance_cases:
            n, channels = (int(v) for v in case.split("x"))
            probe_distances(n, channels, a.steps, a.rounds)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
