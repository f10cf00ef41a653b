#!/usr/bin/env python3
"""Varying scans on long 1-D signals (rf_var_plan_create_signal, kernels_var_signal.hip): whole-step and per-kernel times beside
the measured copy rate and beside what a caller had before, everything alternating in ONE process (the protocol of var_probe.py:
medians of `rounds` rounds of `steps` steps, with the rounds' min and max).

    python tools/probes/var_signal_probe.py [--lengths ...] [--planes 1 3] [--steps 10] [--rounds 5] [--out FILE]

Per length, plane count P and scan list (+x; +x -x, one fused stage), the plane form and the power form (base 0.9) of one plan:
the step between two HIP events and the three kernels from execute_timed.  Byte model of a stage: var_tails_1d reads the signals
and the weights, (4 P + 4) B per sample, and writes 5 floats per tile (2 per plane + 3) and per group; var_pass2_1d reads both and
writes the signals, (8 P + 4) B per sample, and reads the maps; var_carry_1d moves the groups' tuples and carries only.  Each rate
is given as a fraction of (a) rf_stream_copy's on a 4096 x 4096 plane, 8 B per sample.  Beside them, none of it the code under test:
  (b) at 2^24 samples the 2-D twins var_tails_x / var_pass2_x of the same scan list on a 4096 x 4096 image (the same bytes);
  (c) at 2^21 the 2-D plan on the (1, 2^21) image, the only route there was;
  (d) the constant-coefficient order-1 plan on the same signal, the floor.
At 2^24 also the backward, without and with the weight gradient."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

TILE, GROUP = 64, 64
LISTS = {"+x": [(0, True, 0)], "+x-x": [(0, True, 0), (0, False, 0)]}
med = statistics.median
out_file = None


def say(line=""):
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n")


def spread(v):
    return f"(min {min(v):.4f}, max {max(v):.4f})"


def timed(fn, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def kernel_bytes(name, n, planes, scans):
    tiles = -(-n // TILE)
    groups = -(-tiles // GROUP)
    per_slot = (2 * planes + 3) if scans == 2 else (planes + 1)
    if "tails" in name:
        return (4 * planes + 4) * n + 4 * per_slot * (tiles + groups)
    if "carry" in name:
        return 4 * groups * (per_slot + (scans * planes) + (planes if scans == 2 else 0))
    return (8 * planes + 4) * n + 4 * per_slot * tiles + 4 * scans * planes * groups


def probe(n, planes, steps, rounds, copy_planes):
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(25)
    base = 0.9
    ins = [torch.rand(n, device="cuda", generator=gen) * 2 - 1 for _ in range(planes)]
    outs = [torch.empty_like(t) for t in ins]
    d = 1 + 30 * torch.rand(n, device="cuda", generator=gen) ** 4
    w = torch.pow(base, d)
    g1 = rfa.gaussian_weights(5.0, 1)
    say(f"== {n} samples, {planes} plane(s)")
    for name, scans in LISTS.items():
        const_scans = [(0, c, g1) for _, c, _ in scans]
        twin = n == 1 << 24
        only_route = n == 1 << 21
        with rfa.VarPlan.signal(n, scans, planes=planes) as plan, rfa.Plan((n,), const_scans, planes=planes, flags=0) as const:
            image = None
            if twin:
                image = rfa.VarPlan((4096, 4096), scans, planes=planes)
            if only_route:
                image = rfa.VarPlan((1, n), scans, planes=planes)
            shape2 = (4096, 4096) if twin else (1, n)
            ins2, outs2, w2 = [t.view(shape2) for t in ins], [t.view(shape2) for t in outs], w.view(shape2)
            runs = {"planes": lambda: plan.execute(ins, [w], outs), "power": lambda: plan.execute_power(ins, [d], [base], outs),
                    "constant": lambda: const.execute(ins, outs)}
            if image is not None:
                runs["image"] = lambda: image.execute(ins2, [w2], outs2)
            for _ in range(3):
                rfa.stream_copy_ms(*copy_planes, reps=2)
                for fn in runs.values():
                    fn()
            torch.cuda.synchronize()
            copy, step, kernels = [], {k: [] for k in runs}, {"planes": {}, "power": {}, "image": {}}
            for _ in range(rounds):
                copy.append(rfa.stream_copy_ms(*copy_planes, reps=steps))
                for k, fn in runs.items():
                    step[k].append(timed(fn, steps))
                reports = [("planes", plan.execute_timed(ins, [w], outs)[1]), ("power", plan.execute_power_timed(ins, [d], [base], outs)[1])]
                if image is not None:
                    reports.append(("image", image.execute_timed(ins2, [w2], outs2)[1]))
                for form, times in reports:
                    for i, (kname, ms) in enumerate(times):
                        kernels[form].setdefault((i, kname), []).append(ms)
            copy_rate = 8.0 * copy_planes[0].numel() / (med(copy) * 1e-3)
            say(f" - {name}: {plan.num_kernels} launches, workspace {plan.workspace_bytes / 2**20:.2f} MiB; constant plan on path {const.path_name} "
                f"({const.num_kernels} launches); rf_stream_copy {copy_rate / 1e12:.3f} TB/s {spread(copy)} ms")
            for form in ("planes", "power"):
                for (i, kname), ms in sorted(kernels[form].items()):
                    b = kernel_bytes(kname, n, planes, len(scans))
                    rate = b / (med(ms) * 1e-3)
                    say(f"     {form:<6} {kname:<13} {med(ms):9.4f} ms {spread(ms)}   {b / 2**20:10.2f} MiB   {rate / 1e12:6.3f} TB/s   {rate / copy_rate:5.2f} of the copy rate")
                say(f"     {form:<6} step          {med(step[form]):9.4f} ms {spread(step[form])}")
            say(f"     (d) constant order-1 step {med(step['constant']):9.4f} ms {spread(step['constant'])}   signal (planes) / constant {med(step['planes']) / med(step['constant']):.2f}")
            if image is not None:
                what = "(b) 4096 x 4096 image, 2-D twins" if twin else "(c) the (1, 2^21) image"
                for (i, kname), ms in sorted(kernels["image"].items()):
                    say(f"     {what}: {kname:<12} {med(ms):9.4f} ms {spread(ms)}")
                say(f"     {what}: step {med(step['image']):9.4f} ms {spread(step['image'])}   signal step / image step {med(step['planes']) / med(step['image']):.3f}")
                image.close()
            if twin:
                g = [torch.rand(n, device="cuda", generator=gen) * 2 - 1 for _ in range(planes)]
                gin = [torch.empty_like(t) for t in g]
                gw = [torch.empty_like(w)]
                back = {"image gradient": lambda: plan.backward(None, [w], g, gin), "with the weight gradient": lambda: plan.backward(ins, [w], g, gin, gw)}
                for fn in back.values():
                    fn()
                torch.cuda.synchronize()
                t = {k: [] for k in back}
                for _ in range(rounds):
                    for k, fn in back.items():
                        t[k].append(timed(fn, steps))
                for k in back:
                    say(f"     backward, {k:<24} {med(t[k]):9.4f} ms {spread(t[k])}")
                del g, gin, gw
    del ins, outs, d, w
    torch.cuda.empty_cache()


def main():
    global out_file
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", type=int, nargs="+", default=[1 << 20, 1 << 21, 10_000_000, 1 << 24, 1 << 26, 1 << 28])
    ap.add_argument("--planes", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("var_signal_probe: needs a GPU")
    if a.out:
        out_file = open(a.out, "w")
    say(f"var_signal_probe: {torch.cuda.get_device_name(0)}; steps {a.steps}, rounds {a.rounds}; medians over the rounds (min, max)")
    copy_planes = (torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda"))
    for n in a.lengths:
        for planes in a.planes:
            probe(n, planes, a.steps, a.rounds, copy_planes)
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
