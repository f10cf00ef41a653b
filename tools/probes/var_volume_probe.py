#!/usr/bin/env python3
"""The varying scans and the smoothing plan on volumes (rf_var_plan_create_volume, rf_var_distances_volume,
rf_smooth_plan_create_volume): per-kernel and whole-step times against the byte model, the z kernels beside their y twins, and the
volume step against the composite route a caller had before -- everything alternating in ONE process.

    python tools/probes/var_volume_probe.py [--sizes 128 256 512] [--composite 128 256] [--steps 10] [--rounds 5] [--out FILE]

Per cube n^3, planes 1 and 3, plane form and power form: the step +x -x +y -y +z -z (three pair stages, nine launches) timed
between two HIP events, medians over `rounds` rounds of `steps` steps; the nine launches from execute_timed; rf_stream_copy on a
tensor of the volume's size beside them.  Byte model of a pair stage on P planes: the tails pass reads P volumes and the weight
volume, the final pass reads them again and writes P: (3 P + 2) * 4 bytes per sample (tails and carries, 7/64 of that, left out).
The z stage is set beside +y -y of a 2-D plan on an image of the same sample count.  var_distances_volume on C guide volumes:
(4 C + 12) bytes per sample (C + 12 for bytes).  The smoothing plan at K = 3, f32 and bytes.
The composite route (what a caller had before the volume plan): x scans as a 2-D plan on (H D, W), y scans as D calls of a
single-slice plan, z scans as the y scans of a 2-D plan on (D, W H).  Wall time between two synchronisations (launch overhead is
what the volume plan removes) and event time."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

med = statistics.median
PX, MX, PY, MY, PZ, MZ = (0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1), (2, True, 2), (2, False, 2)
FULL = [PX, MX, PY, MY, PZ, MZ]
BASES = [0.9, 0.9, 0.9]
OUT = None


def say(line=""):
    print(line, flush=True)
    if OUT is not None:
        OUT.write(line + "\n")
        OUT.flush()


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
    return (time.perf_counter() - t0) * 1e3 / steps, e0.elapsed_time(e1) / steps


def stream_copy(src, dst):
    """rf_stream_copy of a volume as rows of 1024 samples (whole 256 x 128 tiles), on torch's current stream"""
    import ctypes
    import torch
    from recfilter_amd import capi
    capi.check(capi.lib().rf_stream_copy(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), 1024, src.numel() // 1024,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def rounds_of(fns, steps, rounds):
    """{name: ([wall], [event])}, the callables alternating inside every round"""
    for fn in fns.values():
        fn()
    got = {k: ([], []) for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            w, e = timed(fn, steps)
            got[k][0].append(w)
            got[k][1].append(e)
    return got


def line(name, wall, event, model_bytes=None):
    text = f"   {name:<34} wall {med(wall):9.4f} ms (min {min(wall):.4f}, max {max(wall):.4f})   events {med(event):9.4f} ms (min {min(event):.4f}, max {max(event):.4f})"
    if model_bytes is not None:
        text += f"   model {model_bytes / 2 ** 20:9.1f} MiB -> {model_bytes / med(event) / 1e6:7.1f} GB/s"
    say(text)


def cube(n, steps, rounds, composite):
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(26)
    samples = n ** 3
    twin = (2 ** ((3 * (n.bit_length() - 1)) // 2), samples // 2 ** ((3 * (n.bit_length() - 1)) // 2))      # a 2-D image of n^3 samples
    for P in (1, 3):
        ins = [torch.rand((n, n, n), device="cuda", generator=gen) * 2 - 1 for _ in range(P)]
        outs = [torch.empty_like(t) for t in ins]
        ws = [torch.rand((n, n, n), device="cuda", generator=gen) ** 0.25 for _ in range(3)]
        ds = [1 + 30 * torch.rand((n, n, n), device="cuda", generator=gen) ** 4 for _ in range(3)]
        stage_bytes = (3 * P + 2) * 4 * samples
        with rfa.VarPlan.volume((n, n, n), FULL, planes=P, n_weights=3) as plan, \
                rfa.VarPlan(twin, [PY, MY], planes=P, n_weights=3) as flat:
            flat_of = lambda ts: [t.view(twin) for t in ts]      # noqa: E731
            fns = {"volume step, plane form": lambda: plan.execute(ins, ws, outs),
                   "volume step, power form": lambda: plan.execute_power(ins, ds, BASES, outs),
                   f"+y-y on {twin[0]} x {twin[1]}, plane form": lambda: flat.execute(flat_of(ins), flat_of(ws), flat_of(outs)),
                   "rf_stream_copy of one volume": lambda: stream_copy(ins[0], outs[0])}
            got = rounds_of(fns, steps, rounds)
            say(f"== {n}^3 x {P} plane(s): workspace {plan.workspace_bytes / 2 ** 20:.1f} MiB ({plan.workspace_bytes / (P * 4 * samples):.4f} of the planes)")
            for k, (w, e) in got.items():
                model = 3 * stage_bytes if k.startswith("volume") else stage_bytes if k.startswith("+y-y") else 8 * samples
                line(k, w, e, model)
            for form in ("plane", "power"):
                lists = {}
                for _ in range(rounds):
                    report = plan.execute_timed(ins, ws, outs)[1] if form == "plane" else plan.execute_power_timed(ins, ds, BASES, outs)[1]
                    twin_report = flat.execute_timed(flat_of(ins), flat_of(ws), flat_of(outs))[1] if form == "plane" else \
                        flat.execute_power_timed(flat_of(ins), flat_of(ds), BASES, flat_of(outs))[1]
                    for i, (name, ms) in enumerate(report):
                        lists.setdefault((i, name), []).append(ms)
                    for i, (name, ms) in enumerate(twin_report):
                        lists.setdefault((9 + i, name + " (2-D twin)"), []).append(ms)
                say(f"   -- per kernel, {form} form (tails pass: {(P + 1) * 4 * samples / 2 ** 20:.0f} MiB read; final pass: {(2 * P + 1) * 4 * samples / 2 ** 20:.0f} MiB)")
                for (i, name), v in sorted(lists.items()):
                    model = (P + 1) * 4 * samples if "tails" in name else (2 * P + 1) * 4 * samples if "pass2" in name else None
                    rate = f"  {model / med(v) / 1e6:7.1f} GB/s" if model else ""
                    say(f"   {i:3d} {name:<26} {med(v):8.4f} ms (min {min(v):.4f}, max {max(v):.4f}){rate}")
        if n in composite:
            with rfa.VarPlan.volume((n, n, n), FULL, planes=P, n_weights=3) as plan, \
                    rfa.VarPlan((n * n, n), [PX, MX], planes=P, n_weights=3) as px, rfa.VarPlan((n, n), [PY, MY], planes=P, n_weights=3) as py, \
                    rfa.VarPlan((n, n * n), [(1, True, 2), (1, False, 2)], planes=P, n_weights=3) as pz:
                def route():
                    px.execute_power([t.view(n * n, n) for t in ins], [d.view(n * n, n) for d in ds], BASES, [t.view(n * n, n) for t in outs])
                    for z in range(n):
                        py.execute_power([t[z] for t in outs], [d[z] for d in ds], BASES, [t[z] for t in outs])
                    pz.execute_power([t.view(n, n * n) for t in outs], [d.view(n, n * n) for d in ds], BASES, [t.view(n, n * n) for t in outs])
                want = [t.clone() for t in plan.execute_power(ins, ds, BASES)]
                route()
                torch.cuda.synchronize()
                same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, outs))
                got = rounds_of({"volume step, power form": lambda: plan.execute_power(ins, ds, BASES, outs), "composite route, power form": route}, steps, rounds)
                say(f"   -- the composite route ({3 * (n + 2)} launches; results {'bit-identical' if same else 'DIFFERENT'})")
                for k, (w, e) in got.items():
                    line(k, w, e)
                v, c = got["volume step, power form"], got["composite route, power form"]
                say(f"   volume / composite: wall {med(v[0]) / med(c[0]):5.3f}, events {med(v[1]) / med(c[1]):5.3f}")
        del ins, outs, ws, ds
        torch.cuda.empty_cache()
    # the distances and the smoothing plan
    for C, u8 in ((1, False), (3, False), (3, True)):
        g = torch.rand((C, n, n, n), device="cuda", generator=gen)
        if u8:
            g = (g * 255).to(torch.uint8)
        got = rounds_of({f"var_distances_volume, {C} {'uint8' if u8 else 'f32'} guide volume(s)": lambda: rfa.domain_transform_distances_volume(g, 40.0, 0.5, 2.5)}, steps, rounds)
        for k, (w, e) in got.items():
            line(k, w, e, ((1 if u8 else 4) * C + 12) * samples)
        del g
        torch.cuda.empty_cache()
    image = torch.rand((3, n, n, n), device="cuda", generator=gen)
    image8 = (image * 255).to(torch.uint8)
    out, out8 = torch.empty_like(image), torch.empty_like(image8)
    with rfa.SmoothPlan.volume((n, n, n), planes=3, iterations=3, sigma_s=40.0, sigma_r=0.5) as p32, \
            rfa.SmoothPlan.volume((n, n, n), planes=3, iterations=3, sigma_s=40.0, sigma_r=0.5, image_dtype=torch.uint8) as p8:
        got = rounds_of({"smoothing plan, K = 3, 3 f32 volumes": lambda: p32.execute(image, None, out),
                         "smoothing plan, K = 3, 3 uint8 volumes": lambda: p8.execute(image8, None, out8)}, steps, rounds)
        for k, (w, e) in got.items():
            line(k, w, e)
        say(f"   workspaces: f32 {p32.workspace_bytes / 2 ** 20:.1f} MiB, uint8 {p8.workspace_bytes / 2 ** 20:.1f} MiB; {p32.num_kernels} launches")
    del image, image8, out, out8
    torch.cuda.empty_cache()


def main():
    global OUT
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", type=int, default=[128, 256, 512], help="cube edges (powers of two)")
    ap.add_argument("--composite", nargs="+", type=int, default=[128, 256], help="the sizes at which the composite route is timed")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("var_volume_probe: needs a GPU")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        OUT = open(a.out, "w")
    say(f"var_volume_probe: {torch.cuda.get_device_name(0)}; steps {a.steps}, rounds {a.rounds}; medians over the rounds, everything alternating in one process")
    for n in a.sizes:
        cube(n, a.steps, a.rounds, set(a.composite))


if __name__ == "__main__":
    main()
