"""Times rf_plan_backward beside the forward step on one GPU (profiles/r*/plan_grad.txt).

Per case -- cfg3's scans (xy_pm(GAUSS2), 1 plane) and cfg4b's (xy_pm(GAUSS3), 3 planes), zero and clamped border, 4096^2 and
16384^2 -- windows of `--steps` calls timed with events, the variants alternating inside every round, medians over `--rounds`:
    forward        the plan's execute
    forward^T      the execute of a forward plan of the transposed scan list (zero border): the yardstick of route 1, which runs
                   exactly those launches
    backward       route 1 (zero border) or route 2 (clamped)
    backward+c     route 3, with the coefficient gradients
and the per-launch medians of the adjoint kernels (rf_plan_backward_timed) with the bytes coeff_grad moves (16 per sample: mu, u, y
read once, c0 mu stored).

    python tools/probes/plan_grad_probe.py [--sizes 4096 16384] [--steps 10] [--rounds 5]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))

import torch

import recfilter_amd as rfa
import ref_cases as rc

FILTERS = [("cfg3 xy_pm(GAUSS2)", rc.xy_pm(rc.GAUSS2), 1), ("cfg4b xy_pm(GAUSS3)", rc.xy_pm(rc.GAUSS3), 3)]


def window(call, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def line(label, samples, extra=""):
    print(f"   {label:<22s} {statistics.median(samples):9.4f} ms   (min {min(samples):.4f}, max {max(samples):.4f}){extra}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(f"plan_grad_probe: {torch.cuda.get_device_name(0)}; steps {a.steps}, rounds {a.rounds}; medians over the rounds")
    for n in a.sizes:
        for label, scans, planes in FILTERS:
            shape = (n, n)
            x = [torch.rand(shape, device="cuda") for _ in range(planes)]
            g = [torch.rand(shape, device="cuda") - 0.5 for _ in range(planes)]
            out = [torch.empty_like(t) for t in x]
            gin = [torch.empty_like(t) for t in x]
            transposed = [(d, not c, w) for d, c, w in reversed(scans)]
            for clamped in (False, True):
                with rfa.Plan(shape, scans, clamped=clamped, planes=planes) as plan, rfa.Plan(shape, transposed, planes=planes) as tplan:
                    variants = {
                        "forward": lambda: plan.execute(x, out),
                        "forward^T (zero)": lambda: tplan.execute(g, gin),
                        "backward": lambda: plan.backward(g, gin),
                        "backward+c": lambda: plan.backward(g, gin, inputs=x, coeff_grads=True),
                    }
                    n1, n3 = plan.backward_num_kernels(False), plan.backward_num_kernels(True)
                    print(f"== {n} x {n}, {planes} plane(s), {label}, {'clamped' if clamped else 'zero'} border: route "
                          f"{2 if clamped else 1} {n1} launches, route 3 {n3} launches, + "
                          f"{plan.backward_workspace_bytes(True) / 2 ** 20:.1f} MiB for coefficient gradients", flush=True)
                    for call in variants.values():          # builds, allocations, first launches
                        call()
                    torch.cuda.synchronize()
                    times = {k: [] for k in variants}
                    for _ in range(a.rounds):
                        for k, call in variants.items():
                            times[k].append(window(call, a.steps))
                    for k in variants:
                        line(k + " step", times[k])
                    f = statistics.median(times["forward"])
                    ft = statistics.median(times["forward^T (zero)"])
                    print(f"   backward / forward: {statistics.median(times['backward']) / f:5.2f};  backward / forward^T: "
                          f"{statistics.median(times['backward']) / ft:5.2f};  backward+c / forward: "
                          f"{statistics.median(times['backward+c']) / f:5.2f}")
                    per = {}
                    for _ in range(a.rounds):
                        _, _, launches = plan.backward_timed(g, gin, inputs=x, coeff_grads=True)
                        for i, (name, ms) in enumerate(launches):
                            if name in ("coeff_grad", "coeff_grad_sum", "adjoint_border"):
                                per.setdefault((i, name), []).append(ms)
                    for (i, name), ms in sorted(per.items()):
                        extra = ""
                        if name == "coeff_grad":
                            extra = f"   {16.0 * n * n * planes / (statistics.median(ms) * 1e-3) / 1e9:7.0f} GB/s at 16 B per sample"
                        line(f"{i:3d} {name}", ms, extra)
            del x, g, out, gin
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
