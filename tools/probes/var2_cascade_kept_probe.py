#!/usr/bin/env python3
"""The cascade for training (rf_var2_plan_execute_cascade_keep / _backward_cascade_kept; var2_adj_link_1d, var2_adj_link_keep_1d
and var2_biquad_coef_1d of kernels_var2_signal.hip) beside the route that reruns the forward and beside K chained sections under
autograd, everything alternating in ONE process (the protocol of var2_cascade_probe.py: medians of `rounds` rounds of `steps`
steps, with the rounds' min and max, rf_stream_copy on a 4096 x 4096 plane beside every round).

    python tools/probes/var2_cascade_kept_probe.py [--cases N:LINES ...] [--sections 2 4 8] [--steps 10] [--rounds 5] [--out FILE]

Per case (default: 10^7, 2^24 and 2^28 samples on one line, 4096 lines of 4096 samples) and per K, a causal plan.  Every section
owns its five coefficient signals (clones of one set) where the device's free memory holds them, as a caller's sections do;
where it does not the sections share one set and the report says so.  Byte models per sample:
    var2_adj_link_1d       reads g, a1, a2, b0, b1, b2 of section k and a1, a2 of section k - 1, writes g: 36 B
    var2_adj_link_keep_1d  the same and lam stored: 40 B          var2_biquad_coef_1d  reads lam, x, y, writes five gradients: 32 B
    kept forward 40 K + 4 against execute_cascade's 36 K + 8;  kept backward 72 K + 4 with coefficient gradients (the rerunning
    one 116 K - 36) and 36 K + 12 without;  the training step 112 K + 8 against 120 K of K chained sections.
The report:
  per kernel   the three new kernels as a fraction of the copy rate under their byte models;
  forward      execute_cascade_keep against execute_cascade;
  backward     backward_cascade_kept against backward_cascade, with and without coefficient gradients;
  headline     forward plus backward through biquad_cascade(keep=True) against K chained biquad_scan calls under autograd and
               against biquad_cascade(keep=False), every signal requiring a gradient, measured in this process;
  memory       the peak of torch's device memory above what the leaves hold for the three, the plan's own bytes beside."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

TILE, GROUP = 64, 64
NEW_KERNELS = {"var2_adj_link_1d": 36, "var2_adj_link_keep_1d": 40, "var2_biquad_coef_1d": 32}
med = statistics.median
out_file = None


def say(line=""):
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n")
        out_file.flush()


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


def kernel_bytes(name, n, lines):
    """a new kernel under its byte model: the signals, and for the links the maps and carries read and the maps and aggregates written"""
    tiles = -(-n // TILE)
    groups = -(-tiles // GROUP)
    slots = 0 if "coef" in name else 4 * 6 * (tiles + groups) + 4 * 6 * tiles + 4 * 2 * groups
    return lines * (NEW_KERNELS[name] * n + slots)


def peak_of(fn, prepare):
    """the peak of torch's allocated device memory above what was held before, in bytes, over one call of fn"""
    import torch
    prepare()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def probe(n, lines, counts, steps, rounds, copy_planes):
    import math
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(32)
    shape = (n,) if lines == 1 else (lines, n)
    span = 4 * lines * n
    rand = lambda: torch.rand(shape, device="cuda", generator=gen)      # noqa: E731
    x = rand() * 2 - 1
    theta, r = 0.2 + (math.pi - 0.4) * rand(), 0.5 + 0.48 * rand()
    a1, a2 = (-2 * r * torch.cos(theta)).contiguous(), (r * r).contiguous()
    phi, q, k = 0.2 + (math.pi - 0.4) * rand(), 0.3 + 0.7 * rand(), 0.5 + 0.5 * rand()
    b0, b1, b2 = k.contiguous(), (-2 * k * q * torch.cos(phi)).contiguous(), (k * q * q).contiguous()
    del theta, r, phi, q, k
    section = (b0, b1, b2, a1, a2)
    g = rand() * 2 - 1
    say(f"== {n} samples x {lines} line(s)")
    with rfa.Var2Plan(n, lines=lines) as plan:
        for K in counts:
            torch.cuda.empty_cache()
            free, _ = torch.cuda.mem_get_info()
            own = (17 * K + 12) * span < 0.8 * free      # 5 K coefficients, their gradients twice (the plan's calls, autograd), what is saved
            coefficients = [tuple(t.clone() for t in section) if own else section for _ in range(K)]
            # ---- the plan's calls -----------------------------------------------------------------------------------------------
            out, gin = torch.empty_like(x), torch.empty_like(x)
            kept = [torch.empty_like(x) for _ in range(K - 1)]
            grads = [tuple(torch.empty_like(x) for _ in range(5)) for _ in range(K)]
            runs = {"execute_cascade": lambda: plan.execute_cascade(x, coefficients, out),
                    "execute_cascade_keep": lambda: plan.execute_cascade_keep(x, coefficients, out, kept),
                    "backward_cascade": lambda: plan.backward_cascade(x, coefficients, out, g, gin, grads),
                    "backward_cascade_kept": lambda: plan.backward_cascade_kept(x, coefficients, kept, out, g, gin, grads),
                    "backward_cascade, grad_x only": lambda: plan.backward_cascade(x, coefficients, None, g, gin),
                    "backward_cascade_kept, grad_x only": lambda: plan.backward_cascade_kept(None, coefficients, None, None, g, gin)}
            for _ in range(2):
                rfa.stream_copy_ms(*copy_planes, reps=2)
                for fn in runs.values():
                    fn()
            torch.cuda.synchronize()
            copy, step, kernels = [], {name: [] for name in runs}, {}
            for _ in range(rounds):
                copy.append(rfa.stream_copy_ms(*copy_planes, reps=steps))
                for name, fn in runs.items():
                    step[name].append(timed(fn, steps))
                plan.execute_cascade_keep(x, coefficients, out, kept)
                for times in (plan.backward_cascade_kept_timed(x, coefficients, kept, out, g, gin, grads)[2],
                              plan.backward_cascade_kept_timed(None, coefficients, None, None, g, gin)[2]):
                    for kname, ms in times:
                        if kname in NEW_KERNELS:
                            kernels.setdefault(kname, []).append(ms)
            copy_rate = 8.0 * copy_planes[0].numel() / (med(copy) * 1e-3)
            say(f" - K = {K}: coefficient signals {'of its own per section' if own else 'SHARED by the sections (memory)'}; kept forward {plan.cascade_num_kernels(K)} launches, "
                f"kept backward {plan.backward_cascade_kept_num_kernels(K, True)} / {plan.backward_cascade_kept_num_kernels(K, False)} (rerunning: "
                f"{plan.backward_cascade_num_kernels(K)}); the plan's signals {plan.backward_cascade_kept_bytes(K) / 2**20:.1f} MiB (rerunning: "
                f"{plan.backward_cascade_bytes(K) / 2**20:.1f} MiB); rf_stream_copy {copy_rate / 1e12:.3f} TB/s {spread(copy)} ms")
            for kname in NEW_KERNELS:
                ms = kernels[kname]
                b = kernel_bytes(kname, n, lines)
                rate = b / (med(ms) * 1e-3)
                say(f"     {kname:<22} {med(ms):9.4f} ms {spread(ms)}   {b / 2**20:10.2f} MiB   {rate / 1e12:6.3f} TB/s   {rate / copy_rate:5.2f} of the copy rate"
                    f"   ({NEW_KERNELS[kname]} B per sample; median of {len(ms)} launches)")
            m = {name: med(v) for name, v in step.items()}
            say(f"     forward    execute_cascade_keep {m['execute_cascade_keep']:9.4f} ms {spread(step['execute_cascade_keep'])}   execute_cascade {m['execute_cascade']:9.4f} ms "
                f"{spread(step['execute_cascade'])}   keep / plain {m['execute_cascade_keep'] / m['execute_cascade']:.3f}   (byte model {(40 * K + 4) / (36 * K + 8):.3f})")
            say(f"     backward   with coefficient gradients: kept {m['backward_cascade_kept']:9.4f} ms {spread(step['backward_cascade_kept'])}   rerunning {m['backward_cascade']:9.4f} ms "
                f"{spread(step['backward_cascade'])}   kept / rerunning {m['backward_cascade_kept'] / m['backward_cascade']:.3f}   (byte model {(72 * K + 4) / (116 * K - 36):.3f})")
            kx, rx = m["backward_cascade_kept, grad_x only"], m["backward_cascade, grad_x only"]
            say(f"                grad_x only: kept {kx:9.4f} ms {spread(step['backward_cascade_kept, grad_x only'])}   rerunning {rx:9.4f} ms "
                f"{spread(step['backward_cascade, grad_x only'])}   kept / rerunning {kx / rx:.3f}")
            del out, gin, kept, grads, runs
            torch.cuda.empty_cache()
            # ---- the headline: a training step under autograd -----------------------------------------------------------------
            xl = x.detach().requires_grad_()
            leaves = [[t.detach().requires_grad_() for t in s] for s in coefficients] if own else [[t.detach().requires_grad_() for t in section]] * K

            def drop():
                xl.grad = None
                for s in leaves:
                    for t in s:
                        t.grad = None

            def kept_route():
                drop()
                rfa.biquad_cascade(xl, leaves, keep=True).backward(g)

            def rerunning_route():
                drop()
                rfa.biquad_cascade(xl, leaves).backward(g)

            def chained():
                drop()
                t = xl
                for s in leaves:
                    t = rfa.biquad_scan(t, *s)
                t.backward(g)
            routes = {"keep=True": kept_route, "keep=False": rerunning_route, "chained": chained}
            for _ in range(2):
                for fn in routes.values():
                    fn()
            torch.cuda.synchronize()
            whole = {name: [] for name in routes}
            for _ in range(rounds):
                for name, fn in routes.items():
                    whole[name].append(timed(fn, steps))
            w = {name: med(v) for name, v in whole.items()}
            say(f"     forward+backward   biquad_cascade(keep=True) {w['keep=True']:9.4f} ms {spread(whole['keep=True'])}   biquad_cascade(keep=False) {w['keep=False']:9.4f} ms "
                f"{spread(whole['keep=False'])}   {K} chained biquad_scan {w['chained']:9.4f} ms {spread(whole['chained'])}")
            say(f"     HEADLINE   keep=True / chained {w['keep=True'] / w['chained']:.3f} (byte model {(112 * K + 8) / (120 * K):.3f})   keep=False / chained "
                f"{w['keep=False'] / w['chained']:.3f}   keep=True / keep=False {w['keep=True'] / w['keep=False']:.3f}")
            peaks = {name: peak_of(fn, drop) for name, fn in routes.items()}
            drop()
            signals = lambda b: f"{b / 2**20:.1f} MiB = {b / span:.1f} signals"      # noqa: E731
            say(f"     memory     peak above the leaves: keep=True {signals(peaks['keep=True'])} (+ the plan's {plan.backward_cascade_kept_bytes(K) // span});  keep=False "
                f"{signals(peaks['keep=False'])} (+ the plan's {plan.backward_cascade_bytes(K) // span});  chained {signals(peaks['chained'])} (+ the plan's 1)")
            del xl, leaves, coefficients, routes
            torch.cuda.empty_cache()
    del x, a1, a2, b0, b1, b2, g, section
    torch.cuda.empty_cache()


def main():
    global out_file
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="+", default=["10000000:1", f"{1 << 24}:1", f"{1 << 28}:1", "4096:4096"], help="LENGTH:LINES")
    ap.add_argument("--sections", nargs="+", type=int, default=[2, 4, 8])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("var2_cascade_kept_probe: needs a GPU")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out_file = open(a.out, "w")
    say(f"var2_cascade_kept_probe: {torch.cuda.get_device_name(0)}; steps {a.steps}, rounds {a.rounds}; medians over the rounds (min, max)")
    copy_planes = (torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda"))
    for case in a.cases:
        n, lines = (int(v) for v in case.split(":"))
        probe(n, lines, a.sections, a.steps, a.rounds, copy_planes)
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
