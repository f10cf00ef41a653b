#!/usr/bin/env python3
"""Digests of small tiled plans that reach every rule of the final pass's instance selector (recfilter_amd/csrc/pass2_select.h),
for comparing two builds of the library bit for bit.

    RECFILTER_AMD_LIB=/path/to/other/librecfilter_amd.so python tools/probes/pass2_digest.py > other.txt
    python tools/probes/pass2_digest.py > built.txt && cmp other.txt built.txt

With fixed seeds, one line per case:  <case name> <sha256 of every output plane's bytes>  (or ERROR and the library's message: a
shape a type does not take is refused by both builds alike).  The cases, all on RF_PLAN_TILED_ONLY plans of two tiles per dimension:
tile rows 32, 64 and 128 on (2 TY, 512), (2 TY + 5, 512), (2 TY, 516), (2 TY + 5, 518) for every pixel type (f64 asks for 64 rows
only, i16 leaves out the last shape), with one causal scan, the pair, anticausal first and x only; unsigned bytes to f32 and to bytes; a 16-bit volume of two z
tiles (the widening route); an order-5 clamped filter (mod form); a folded 1-D signal whose length is not a whole number of rows;
an affine epilogue and one with an input operand at orders 2 and 3; the neighbour form and the row-scan form at the smallest
size the planner grants them (plan_fused.cpp: any filter that decays within a tile; order 2 on whole 256 x 128 tiles), each
reported with the plan's own "neighbour_carries" / "row_scans" tables.  Under rocprofv3 --kernel-trace the same run gives the
ordered list of kernel instances.  No time is printed: the output of one build is the same from run to run."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402


def from_poles(poles, b=0.25):
    p = np.poly(poles).real
    return [b] + [float(-v) for v in p[1:]]


def main():
    import torch
    import recfilter_amd as rfa
    from recfilter_amd import capi
    if not torch.cuda.is_available():
        sys.exit("pass2_digest: needs a GPU")
    gen = torch.Generator().manual_seed(22)      # on the host: the same numbers whatever the device's generator does

    def planes(shape, dtype, n=1):
        if dtype in (torch.int32, torch.int16):
            return [torch.randint(0, 7, shape, generator=gen).to(dtype).cuda() for _ in range(n)]
        if dtype == torch.uint8:
            return [torch.randint(0, 256, shape, generator=gen).to(dtype).cuda() for _ in range(n)]
        return [torch.rand(shape, generator=gen, dtype=torch.float64).to(dtype).cuda() for _ in range(n)]

    def run(case, shape, scans, dtype=torch.float32, source=None, report=(), n_planes=1, **kw):
        flags = kw.pop("flags", 0) | capi.RF_PLAN_TILED_ONLY
        try:
            with rfa.Plan(shape, scans, dtype=dtype, planes=n_planes, flags=flags, **kw) as plan:
                outs = plan.execute(planes(shape, source or dtype, n_planes))
                torch.cuda.synchronize()
                h = hashlib.sha256()
                for t in outs:
                    h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
                notes = " ".join(f"{name}={[float(v) for v in plan.table(name)][-3:]}" for name in report)
                print(f"{case} {plan.path_name} tiles={plan.tiles} {notes} {h.hexdigest()}", flush=True)
        except Exception as e:       # noqa: BLE001 -- a refusal is part of the output, the same for both builds
            print(f"{case} ERROR {type(e).__name__} {e}", flush=True)

    g2, g3, g1 = rfa.gaussian_weights(3.0, 2), rfa.gaussian_weights(3.0, 3), rfa.gaussian_weights(3.0, 1)
    summed = [1.0, 1.0]      # integer pixels: running sums

    def filters(w):
        return {"one": [(0, True, w), (1, True, w)],
                "pair": [(0, True, w), (0, False, w), (1, True, w), (1, False, w)],
                "anti-first": [(0, False, w), (0, True, w), (1, False, w), (1, True, w)],
                "x-only": [(0, True, w), (0, False, w)]}

    types = [("f32", torch.float32, g2), ("f16", torch.float16, g2), ("bf16", torch.bfloat16, g2), ("i32", torch.int32, summed),
             ("i16", torch.int16, summed), ("f64", torch.float64, g2)]
    for ty in (32, 64, 128):
        rows = capi.RF_PLAN_TILE_ROWS(ty)
        shapes = [(2 * ty, 512), (2 * ty + 5, 512), (2 * ty, 516), (2 * ty + 5, 518)]
        for name, dtype, w in types:
            if name == "f64" and ty != 64:
                continue
            for shape in shapes[:3] if name == "i16" else shapes:      # (2-byte integers: a width of 518 leaves the fused path)
                for fname, scans in filters(w).items():
                    for clamped in ((False, True) if fname == "pair" else (False,)):
                        run(f"ty{ty} {name} {shape[0]}x{shape[1]} {fname} clamped={int(clamped)}", shape, scans, dtype, flags=rows, clamped=clamped)
        # unsigned bytes to f32 and to bytes (the byte planes: widths that are multiples of 4)
        for shape in shapes[:3]:
            for fname in ("one", "pair"):
                scans = filters(g2)[fname]
                run(f"ty{ty} u8>f32 {shape[0]}x{shape[1]} {fname}", shape, scans, source=torch.uint8, input_dtype=np.uint8, flags=rows)
                run(f"ty{ty} u8>u8 {shape[0]}x{shape[1]} {fname}", shape, scans, source=torch.uint8, input_dtype=np.uint8, output_dtype=np.uint8, flags=rows)
                run(f"ty{ty} u8>u8 {shape[0]}x{shape[1]} {fname} affine", shape, scans, source=torch.uint8, input_dtype=np.uint8, output_dtype=np.uint8,
                    flags=rows, epilogue=(0.5, 0.0, 3.0))
                run(f"ty{ty} u8>u8 {shape[0]}x{shape[1]} {fname} operand", shape, scans, source=torch.uint8, input_dtype=np.uint8, output_dtype=np.uint8,
                    flags=rows, epilogue=(0.5, 0.25, 3.0))
        # a 16-bit volume of two z tiles: its x/y stage reads the 16-bit planes and writes the f32 volume
        for name, dtype in (("f16", torch.float16), ("bf16", torch.bfloat16)):
            for shape in ((64, 2 * ty, 512), (64, 2 * ty + 5, 516)):
                xyz = filters(g2)["pair"] + [(2, True, g2), (2, False, g2)]
                run(f"ty{ty} {name} volume {shape}", shape, xyz, dtype, flags=rows | capi.RF_PLAN_TILE_PLANES(32))
                run(f"ty{ty} {name} volume {shape} one", shape, [(0, True, g2), (1, True, g2), (2, True, g2)], dtype, flags=rows | capi.RF_PLAN_TILE_PLANES(32))
        # epilogues, orders 2 and 3
        for kname, w in (("K2", g2), ("K3", g3)):
            for shape in (shapes[0], shapes[3]):
                for fname in ("one", "pair", "anti-first"):
                    for ename, epi in (("affine", (0.5, 0.0, 0.125)), ("operand", (0.5, 0.25, 0.125))):
                        run(f"ty{ty} f32 {kname} {shape[0]}x{shape[1]} {fname} {ename}", shape, filters(w)[fname], flags=rows, epilogue=epi)
                        if ty == 64:
                            run(f"ty{ty} f64 {kname} {shape[0]}x{shape[1]} {fname} {ename}", shape, filters(w)[fname], torch.float64, flags=rows, epilogue=epi)
        run(f"ty{ty} f32 K1 pair", shapes[0], filters(g1)["pair"], flags=rows)
        run(f"ty{ty} f32 K3 pair", shapes[3], filters(g3)["pair"], flags=rows)
        # batched planes
        run(f"ty{ty} f32 3 planes pair", shapes[3], filters(g2)["pair"], flags=rows, n_planes=3)
        # mod form: an order-5 clamped filter runs as sections behind border modifications
        order5 = from_poles([0.8, 0.5 + 0.3j, 0.5 - 0.3j, -0.2 + 0.6j, -0.2 - 0.6j])
        for shape in (shapes[0], (2 * ty, 768)):      # (whole tiles: the planner gives no sections to a partial one)
            run(f"ty{ty} f32 order5 clamped {shape[0]}x{shape[1]}", shape, filters(order5)["pair"], flags=rows, clamped=True, path=capi.RF_PATH_TILED_FUSED)
    # a folded 1-D signal whose length is not a whole number of rows (zero border, causal scans only)
    for n in (32768, 32768 - 100):
        for ty in (32, 64):
            run(f"ty{ty} f32 signal {n}", (n,), [(0, True, g2)], flags=capi.RF_PLAN_TILE_ROWS(ty), path=capi.RF_PATH_TILED_FUSED)
            run(f"ty{ty} f32 signal {n} affine", (n,), [(0, True, g2)], flags=capi.RF_PLAN_TILE_ROWS(ty), path=capi.RF_PATH_TILED_FUSED, epilogue=(0.5, 0.0, 0.125))
    # the neighbour form and the row-scan form (a filter that decays within a tile)
    narrow = rfa.gaussian_weights(1.5, 2)
    tall = capi.RF_PLAN_TILE_ROWS(128)
    for shape in ((256, 512), (261, 516), (384, 768)):
        for fname in ("pair", "one"):
            for label, extra in (("", 0), (" separate", capi.RF_PLAN_SEPARATE_ROW_SCANS), (" full", capi.RF_PLAN_FULL_CARRY_SCAN)):
                run(f"neighbour {shape[0]}x{shape[1]} {fname}{label}", shape, filters(narrow)[fname], flags=tall | extra, report=("neighbour_carries", "row_scans"))
    run("neighbour ty64 256x512 pair", (256, 512), filters(narrow)["pair"], flags=capi.RF_PLAN_TILE_ROWS(64), report=("neighbour_carries", "row_scans"))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
