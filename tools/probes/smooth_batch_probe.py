#!/usr/bin/env python3
"""The batched smoothing plan (rf_smooth_plan_create_batched, SmoothPlan(batch=N)): ONE call on (N, C, H, W) against the loop of
N single-image plan calls it replaces, on the same tensors, alternating in ONE process.

    python tools/probes/smooth_batch_probe.py [--cases 16x3x256 16x3x512 8x3x1024 4x3x2048] [--iterations 3] [--steps 5] [--rounds 5]
                                              [--parent-lib PATH]

Per case NxCxSIZE (square images; self-guided, the common call of a training loop) and per kind -- forward f32, forward uint8,
backward with the distances held constant (edges = 0) and through them (edges = 1) -- each round times `steps` batched calls and
`steps` loops of N single-image calls.  Two clocks: WALL time between two stream synchronisations (what a caller waits: host time
per call is part of what the batch removes) and the time between two HIP events on the stream.  Printed: medians over the rounds
with the rounds' min and max, batched / loop, and whether that ratio lies inside the rounds' own min-to-max spread of the loop.
Then the per-kernel lines of the batched plan's execute_timed / backward_timed beside N times the single-image plan's, and the
device memory of both routes: the plans' own workspaces (forward, and what edges = 1 adds), which torch's allocator does not see,
plus torch's peak over one backward call.

--parent-lib PATH: another build of the library (the parent commit's; it need not have the batched entry point) is loaded beside
the built one, and the same LOOP runs on it in the same rounds -- the baseline for "did the existing kernels get slower": per kind
new / parent of the loop, and per kernel new / parent of the single-image plan's timed forms."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SIGMA_S, SIGMA_R = 40.0, 0.5
med = statistics.median
MiB = 2.0 ** 20


def load_beside(path):
    """a second build of the library in this process (dlopen keeps the two apart); entry points it lacks stay unbound"""
    from recfilter_amd import capi
    built = capi.lib()

    class _Absent:
        argtypes = restype = None

    class OlderBuild(ctypes.CDLL):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if name == "rf_smooth_plan_create_batched":
                    return _Absent()
                raise
    keep = (capi.LIB_PATH, ctypes.CDLL)
    capi.LIB_PATH, capi._lib, ctypes.CDLL = path, None, OlderBuild
    try:
        other = capi.lib()
    finally:
        capi.LIB_PATH, ctypes.CDLL = keep
        capi._lib = built
    return other


class using:
    """the calls inside go to `library` (None: the built one)"""

    def __init__(self, library):
        self.library = library

    def __enter__(self):
        from recfilter_amd import capi
        self.keep = capi._lib
        if self.library is not None:
            capi._lib = self.library

    def __exit__(self, *exc):
        from recfilter_amd import capi
        capi._lib = self.keep


def timed(fn, steps):
    """(wall ms, event ms) per call of `steps` calls between two synchronisations"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    return wall, e0.elapsed_time(e1) / steps


def spread(v):
    return f"(min {min(v):.4f}, max {max(v):.4f})"


def probe(N, C, n, K, steps, rounds, parent):
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(20)
    image = torch.rand((N, C, n, n), device="cuda", generator=gen)
    g = torch.rand((N, C, n, n), device="cuda", generator=gen) * 2 - 1
    image8 = (image * 255).to(torch.uint8)
    out, out8, gim = torch.empty_like(image), torch.empty_like(image8), torch.empty_like(image)
    make = lambda dtype, batch: rfa.SmoothPlan((n, n), planes=C, image_dtype=dtype, iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R, batch=batch)      # noqa: E731
    batched, batched8 = make(torch.float32, N), make(torch.uint8, N)
    single, single8 = make(torch.float32, None), make(torch.uint8, None)
    routes = {"batched": (None, batched, batched8), "loop": (None, single, single8)}
    if parent is not None:
        with using(parent):
            routes["parent loop"] = (parent, make(torch.float32, None), make(torch.uint8, None))

    def call(route, kind):
        library, p32, p8 = routes[route]
        whole = route == "batched"

        def fn():
            with using(library):
                for b in ([slice(None)] if whole else range(N)):
                    if kind == "forward f32":
                        p32.execute(image[b], None, out[b])
                    elif kind == "forward uint8":
                        p8.execute(image8[b], None, out8[b])
                    else:
                        p32.backward(image[b], None, g[b], gim[b], None, edges=kind.endswith("1"))
        return fn
    kinds = ["forward f32", "forward uint8", "backward edges=0", "backward edges=1"]
    run = {(r, k): call(r, k) for k in kinds for r in routes}
    for _ in range(2):
        for fn in run.values():
            fn()
    torch.cuda.synchronize()
    wall, event = {k: [] for k in run}, {k: [] for k in run}
    for _ in range(rounds):
        for k, fn in run.items():
            w, e = timed(fn, steps)
            wall[k].append(w)
            event[k].append(e)
    print(f"== {N} x {C} x {n} x {n}, K = {K}: launches per call {batched.num_kernels} forward, {batched.backward_num_kernels(False)} / "
          f"{batched.backward_num_kernels(True)} backward -- the loop issues {N} times as many")
    for k in kinds:
        for r in routes:
            print(f"   {k:<17} {r:<12} wall {med(wall[r, k]):9.4f} ms {spread(wall[r, k])}   events {med(event[r, k]):9.4f} ms {spread(event[r, k])}")
        lo, hi = min(wall["loop", k]), max(wall["loop", k])
        ratio = med(wall["batched", k]) / med(wall["loop", k])
        verdict = "inside the loop's spread" if lo <= med(wall["batched", k]) <= hi else ("FASTER" if ratio < 1 else "SLOWER than the loop beyond its spread")
        print(f"   {k:<17} batched / loop: wall {ratio:5.3f}, events {med(event['batched', k]) / med(event['loop', k]):5.3f}   -> {verdict}")
        if parent is not None:
            r = med(wall["loop", k]) / med(wall["parent loop", k])
            plo, phi = min(wall["parent loop", k]) / med(wall["parent loop", k]), max(wall["parent loop", k]) / med(wall["parent loop", k])
            print(f"   {k:<17} loop, new / parent: wall {r:5.3f}, events {med(event['loop', k]) / med(event['parent loop', k]):5.3f} "
                  f"(the parent's rounds span {plo:5.3f} .. {phi:5.3f} of their median)")
    # per kernel: the batched plan beside N single-image launches, and the single-image plan new / parent
    for what in ("forward f32", "backward edges=1"):
        lists = {}
        for _ in range(rounds):
            for r, (library, p32, _) in routes.items():
                with using(library):
                    if what == "forward f32":
                        times = p32.execute_timed(image if r == "batched" else image[0], None, out if r == "batched" else out[0])[1]
                    else:
                        times = p32.backward_timed(image if r == "batched" else image[0], None, g if r == "batched" else g[0],
                                                   gim if r == "batched" else gim[0], None, edges=True)[2]
                for i, (name, ms) in enumerate(times):
                    lists.setdefault(r, {}).setdefault((i, name), []).append(ms)
        print(f"   -- per kernel, {what}: batched (one launch, {N} images) | single image | {N} x single" + (" | single, new / parent" if parent is not None else ""))
        for key in sorted(lists["batched"]):
            i, name = key
            b, s = med(lists["batched"][key]), med(lists["loop"][key])
            line = f"   {i:3d} {name:<20} {b:8.4f} ms {spread(lists['batched'][key])} | {s:8.4f} ms {spread(lists['loop'][key])} | {N * s:8.4f} ms"
            if parent is not None:
                p = lists["parent loop"][key]
                line += f" | {s / med(p):5.3f} (parent {med(p):.4f} ms {spread(p)})"
            print(line)
    # memory: the plans' own allocations and torch's peak over one backward call through the distances
    peak = {}
    for r in ("batched", "loop"):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        run[r, "backward edges=1"]()
        torch.cuda.synchronize()
        peak[r] = torch.cuda.max_memory_allocated()
    for r, plan in (("batched", batched), ("loop", single)):
        own, own_b = plan.workspace_bytes, plan.backward_workspace_bytes(True)
        print(f"   memory, {r:<8} plan workspace {own / MiB:8.1f} MiB + {own_b / MiB:8.1f} MiB for edges = 1; torch's peak {peak[r] / MiB:8.1f} MiB "
              f"(the tensors of the probe); together {(own + own_b + peak[r]) / MiB:8.1f} MiB")
    for library, p32, p8 in routes.values():
        with using(library):      # (a plan goes back to the build that made it)
            p32.close()
            p8.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="+", default=["16x3x256", "16x3x512", "8x3x1024", "4x3x2048"], help="NxCxSIZE")
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="another build of librecfilter_amd.so: the same loop on it, in the same rounds")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("smooth_batch_probe: needs a GPU")
    parent = load_beside(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    print(f"smooth_batch_probe: {torch.cuda.get_device_name(0)}; K {a.iterations}, steps {a.steps}, rounds {a.rounds}; medians over the rounds"
          + (f"; parent library {os.path.basename(a.parent_lib)}" if parent is not None else ""))
    for case in a.cases:
        N, C, n = (int(v) for v in case.split("x"))
        probe(N, C, n, a.iterations, a.steps, a.rounds, parent)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
