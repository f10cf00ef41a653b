#!/usr/bin/env python3
"""The adjoint of the varying scans (rf_var_plan_backward): per-kernel and whole-step times of the backward of the `+x -x +y -y`
plan, without and with weight gradients, beside the forward step of the SAME plan, alternating in ONE process.

    python tools/probes/var_grad_probe.py [--cases 1024x3 4096x1] [--steps 10] [--rounds 5]

Per case (square images, SIZExPLANES) it builds one VarPlan (+x -x on weight plane 0, +y -y on weight plane 1), warms everything
up, then runs `rounds` rounds; each round times `steps` forward executes, `steps` backward calls without weight gradients and
`steps` with them, each between two HIP events, and one backward_timed() of each kind for the per-kernel times.  Printed: medians
over the rounds with the rounds' min and max, the two backward / forward ratios, and beside them the ratios of the byte model
(per sample and plane, tails aside): the forward's two fused stages move 40 B; an adjoint stage 20 B, so four of
them 80 B; with weight gradients every scan adds the recompute's 20 B, 4 B for the state, 12 B in var_grad and, once per scan and
not per plane, 4 B of gradient plane (8 B where var_grad adds to it)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SCANS = [(0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1)]


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


def model_bytes(planes):
    """(forward, backward, backward with weight gradients) bytes per sample of the byte model, all planes"""
    forward = 40 * planes
    backward = 4 * 20 * planes
    # per scan: recompute + state + var_grad's three reads per plane; the gradient plane stored by the first scan of a weight
    # plane and read and stored by the second
    with_weights = backward + 4 * (20 + 4 + 12) * planes + 2 * (4 + 8)
    return forward, backward, with_weights


def probe(n, planes, steps, rounds):
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(18)
    rand = lambda: torch.rand((n, n), device="cuda", generator=gen)      # noqa: E731
    ins = [rand() * 2 - 1 for _ in range(planes)]
    outs = [torch.empty_like(t) for t in ins]
    g = [rand() * 2 - 1 for _ in range(planes)]
    gin = [torch.empty_like(t) for t in ins]
    ws = [rand() ** 0.25 for _ in range(2)]
    gws = [torch.empty_like(t) for t in ws]
    med = statistics.median
    with rfa.VarPlan((n, n), SCANS, planes=planes, n_weights=2) as plan:
        run = {"forward": lambda: plan.execute(ins, ws, outs),
               "backward": lambda: plan.backward(None, ws, g, gin),
               "backward+w": lambda: plan.backward(ins, ws, g, gin, gws)}
        for _ in range(3):
            for fn in run.values():
                fn()
        torch.cuda.synchronize()
        step = {k: [] for k in run}
        kernels = {"backward": {}, "backward+w": {}}
        for _ in range(rounds):
            for k, fn in run.items():
                step[k].append(timed(fn, steps))
            for k, times in (("backward", plan.backward_timed(None, ws, g, gin)[2]), ("backward+w", plan.backward_timed(ins, ws, g, gin, gws)[2])):
                for i, (name, ms) in enumerate(times):
                    kernels[k].setdefault((i, name), []).append(ms)
        print(f"== {n} x {n}, {planes} plane(s): workspace {plan.workspace_bytes / 2**20:.1f} MiB, "
              f"+ {plan.backward_workspace_bytes(True) / 2**20:.1f} MiB for weight gradients")
        for k in ("backward", "backward+w"):
            print(f"   -- {k}: {len(kernels[k])} launches")
            for (i, name), ms in sorted(kernels[k].items()):
                print(f"   {i:2d} {name:<16} {med(ms):8.4f} ms   {spread(ms)}")
        model = dict(zip(run, model_bytes(planes)))
        for k in run:
            print(f"   {k + ' step':<18} {med(step[k]):8.4f} ms   {spread(step[k])}   byte model {model[k]:4d} B per sample")
        for k in ("backward", "backward+w"):
            print(f"   {k} / forward: measured {med(step[k]) / med(step['forward']):5.2f}, byte model {model[k] / model['forward']:5.2f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="+", default=["1024x3", "4096x1"], help="SIZExPLANES")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("var_grad_probe: needs a GPU")
    print(f"var_grad_probe: {torch.cuda.get_device_name(0)}; steps {a.steps}, rounds {a.rounds}; medians over the rounds")
    for case in a.cases:
        n, planes = (int(v) for v in case.split("x"))
        probe(n, planes, a.steps, a.rounds)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
